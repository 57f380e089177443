/*
 * stringkey_loopback.cpp — STRING join/shuffle keys across G ranks on ONE
 * GPU. Ranks run as host threads, each with the loopback implementation of
 * the public Communicator interface (loopback.hpp) that hands device buffers
 * over through an in-process mailbox; upload and read-back are those of
 * host_table.hpp.
 *
 * Global tables: 40 000 x 40 000 rows of (key STRING, payload INT64); the
 * key is a formula of the row (length 0-20, duplicates on both sides).
 *
 * Checks:
 *   1. after shuffle_on on the STRING key, every distinct key string lives
 *      on exactly one rank, and no row is lost;
 *   2. the concatenated G-rank distributed_inner_join has the row count and
 *      the order-insensitive checksum of the 1-rank join of the same global
 *      tables, computed in this program.
 *
 * usage: stringkey_loopback G nvlink_domain_size compression
 * Build/run: tests/test_gpu_string_keys.py::test_stringkey_loopback.
 */
#include "host_table.hpp"
#include "loopback.hpp"

#include "compression.hpp"
#include "distributed_join.hpp"
#include "shuffle_on.hpp"

#include <map>
#include <string>
#include <vector>

/* ---------------- tables ---------------- */

constexpr int64_t kRows = 40000;
constexpr uint64_t kDistinct = 12000;

/* key string of a key id: "" for id 0, else 1-20 lowercase bytes */
static std::string key_string(uint64_t id)
{
  const int len = id == 0 ? 0 : 1 + (int)(id % 20);
  std::string s((size_t)len, 'a');
  for (int k = 0; k < len; k++) s[(size_t)k] = (char)('a' + dj_mix64(id * 32 + (uint64_t)k) % 26);
  return s;
}

static uint64_t key_id(int64_t global_row, bool left)
{
  return dj_mix64((uint64_t)global_row + (left ? 0ull : 7777777ull)) % kDistinct;
}

/* rows [row0, row0 + rows) of a global table as (key STRING, payload INT64) */
static std::unique_ptr<cudf::table> make_table(int64_t row0, int64_t rows, bool left)
{
  std::vector<std::string> key((size_t)rows);
  std::vector<int64_t> pay((size_t)rows);
  for (int64_t t = 0; t < rows; t++) {
    key[(size_t)t] = key_string(key_id(row0 + t, left));
    pay[(size_t)t] = (row0 + t) * 2 + (left ? 0 : 1);
  }
  std::vector<std::unique_ptr<cudf::column>> cols;
  cols.push_back(device_strings(key));
  cols.push_back(device_fixed(cudf::type_id::INT64, pay.data(), rows, 8));
  return std::make_unique<cudf::table>(std::move(cols));
}

/* order-insensitive checksum over (STRING, INT64, STRING, INT64) join rows */
static void checksum(const cudf::table& t, uint64_t* sum, int64_t* rows)
{
  if (t.num_columns() != 4 || t.get_column(0).type().id() != cudf::type_id::STRING ||
      t.get_column(2).type().id() != cudf::type_id::STRING)
    FAIL("JOIN OUTPUT SCHEMA WRONG");
  const HTable h = from_device(t);
  const auto &lk = h[0].s, &rk = h[2].s;
  const auto &lp = h[1].v, &rp = h[3].v;
  uint64_t s = 0;
  for (size_t i = 0; i < lk.size(); i++) {
    if (lk[i] != rk[i]) FAIL("JOIN ROW WITH UNEQUAL KEYS");
    s += dj_mix64(fold(lk[i]) ^ dj_mix64((uint64_t)lp[i] ^
                                         dj_mix64((fold(rk[i]) + 1) ^ dj_mix64((uint64_t)rp[i]))));
  }
  *sum = s;
  *rows = t.num_rows();
}

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int nvl = argc > 2 ? atoi(argv[2]) : G;
  const bool compress = argc > 3 && atoi(argv[3]) != 0;
  if (G < 1 || kRows % G != 0) {
    printf("G must divide %lld\n", (long long)kRows);
    return 1;
  }
  CHECK(hipSetDevice(0));

  /* single-rank reference on the global tables */
  uint64_t want_sum = 0;
  int64_t want_rows = 0;
  {
    auto left = make_table(0, kRows, true);
    auto right = make_table(0, kRows, false);
    Mailbox mb;
    LoopbackComm comm(0, 1, &mb);
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, &comm, lo, ro, 1,
                                      false, nullptr, 1);
    checksum(*res, &want_sum, &want_rows);
  }
  if (want_rows < kRows) {
    printf("reference join suspiciously small: %lld rows\n", (long long)want_rows);
    return 1;
  }

  const int64_t per = kRows / G;

  /* 1. shuffle_on placement */
  {
    Mailbox mb;
    std::vector<std::vector<std::string>> keys_on((size_t)G);
    run_ranks(G, &mb, [&](int r, Communicator* comm) {
      auto t = make_table(r * per, per, true);
      auto opts = generate_compression_options_distributed(t->view(), compress);
      auto shuffled = shuffle_on(t->view(), {0}, comm, opts, cudf::hash_id::HASH_MURMUR3,
                                 12345678u);
      keys_on[(size_t)r] = from_device(shuffled->get_column(0)).s;
    });
    std::map<std::string, int> owner;
    int64_t total = 0;
    for (int r = 0; r < G; r++) {
      total += (int64_t)keys_on[(size_t)r].size();
      for (auto& s : keys_on[(size_t)r]) {
        auto it = owner.emplace(s, r).first;
        if (it->second != r) {
          printf("KEY ON TWO RANKS (%d and %d), length %zu\n", it->second, r, s.size());
          return 1;
        }
      }
    }
    std::map<std::string, int> expect;
    for (int64_t i = 0; i < kRows; i++) expect[key_string(key_id(i, true))]++;
    if (total != kRows || owner.size() != expect.size()) {
      printf("SHUFFLE LOST ROWS OR KEYS (%lld rows, %zu of %zu keys)\n", (long long)total,
             owner.size(), expect.size());
      return 1;
    }
    if (G > 1) {
      std::vector<int> used((size_t)G, 0);
      for (auto& kv : owner) used[(size_t)kv.second] = 1;
      for (int r = 0; r < G; r++)
        if (!used[(size_t)r]) {
          printf("RANK %d RECEIVED NO KEY\n", r);
          return 1;
        }
    }
    printf("shuffle placement OK (%zu distinct keys over %d ranks)\n", owner.size(), G);
  }

  /* 2. distributed_inner_join against the single-rank result */
  {
    Mailbox mb;
    std::vector<uint64_t> sums((size_t)G, 0);
    std::vector<int64_t> rows((size_t)G, 0);
    run_ranks(G, &mb, [&](int r, Communicator* comm) {
      auto left = make_table(r * per, per, true);
      auto right = make_table(r * per, per, false);
      auto lo = generate_compression_options_distributed(left->view(), compress);
      auto ro = generate_compression_options_distributed(right->view(), compress);
      auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, comm, lo, ro,
                                        2, false, nullptr, nvl);
      checksum(*res, &sums[(size_t)r], &rows[(size_t)r]);
    });
    uint64_t got_sum = 0;
    int64_t got_rows = 0;
    for (int r = 0; r < G; r++) {
      got_sum += sums[(size_t)r];
      got_rows += rows[(size_t)r];
    }
    printf("single-rank: rows=%lld sum=%llx; %d-rank(nvl=%d, comp=%d): rows=%lld sum=%llx\n",
           (long long)want_rows, (unsigned long long)want_sum, G, nvl, (int)compress,
           (long long)got_rows, (unsigned long long)got_sum);
    if (got_rows != want_rows || got_sum != want_sum) {
      printf("STRINGKEY LOOPBACK MISMATCH\n");
      return 1;
    }
  }
  printf("STRINGKEY LOOPBACK OK\n");
  return 0;
}
