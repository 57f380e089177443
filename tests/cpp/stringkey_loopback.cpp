/*
 * stringkey_loopback.cpp — STRING join/shuffle keys across G ranks on ONE
 * GPU. Ranks run as host threads, each with a small loopback implementation
 * of the public Communicator interface (include/communicator.hpp) that
 * hands device buffers over through an in-process mailbox.
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
#include "communicator.hpp"
#include "compression.hpp"
#include "distributed_join.hpp"
#include "shuffle_on.hpp"

#include "../../distributed_join_amd/csrc/dj_rng.h"

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#define CHECK(c)                                                      \
  do {                                                                \
    hipError_t e = (c);                                               \
    if (e != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

/* ---------------- loopback transport ---------------- */

struct Mailbox {
  struct Msg {
    const void* src;
    size_t bytes;
    bool consumed;
  };
  std::mutex m;
  std::condition_variable cv;
  std::map<std::tuple<int, int, long>, Msg> msgs;  // (src, dst, seq of the pair)
  std::map<std::pair<int, int>, long> send_seq, recv_seq;

  void post(int src, int dst, const void* buf, size_t bytes)
  {
    std::lock_guard<std::mutex> g(m);
    msgs[{src, dst, send_seq[{src, dst}]++}] = Msg{buf, bytes, false};
    cv.notify_all();
  }
  void fetch(int src, int dst, void* out, size_t bytes)
  {
    std::unique_lock<std::mutex> g(m);
    const long seq = recv_seq[{src, dst}]++;
    cv.wait(g, [&] { return msgs.count({src, dst, seq}) != 0; });
    Msg& msg = msgs[{src, dst, seq}];
    if (msg.bytes != bytes) {
      printf("loopback size mismatch %zu vs %zu\n", msg.bytes, bytes);
      exit(1);
    }
    CHECK(hipMemcpy(out, msg.src, bytes, hipMemcpyDeviceToDevice));
    msg.consumed = true;
    cv.notify_all();
  }
  void drain(int src)
  {
    std::unique_lock<std::mutex> g(m);
    cv.wait(g, [&] {
      for (auto& kv : msgs)
        if (std::get<0>(kv.first) == src && !kv.second.consumed) return false;
      return true;
    });
  }
};

class LoopbackComm : public Communicator {
 public:
  LoopbackComm(int rank, int size, Mailbox* mb) : mb_(mb)
  {
    mpi_rank = rank;
    mpi_size = size;
    current_device = 0;
  }
  void initialize() override {}
  void start() override {}
  void stop() override
  {
    mb_->drain(mpi_rank);
    CHECK(hipDeviceSynchronize());
  }
  void send(const void* buf, int64_t count, int element_size, int dest) override
  {
    CHECK(hipDeviceSynchronize());
    mb_->post(mpi_rank, dest, buf, (size_t)count * element_size);
  }
  void recv(void* buf, int64_t count, int element_size, int source) override
  {
    mb_->fetch(source, mpi_rank, buf, (size_t)count * element_size);
  }
  void finalize() override {}
  bool group_by_batch() override { return true; }

 private:
  Mailbox* mb_;
};

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
  std::vector<int32_t> off((size_t)rows + 1, 0);
  std::string chars;
  std::vector<int64_t> pay((size_t)rows);
  for (int64_t t = 0; t < rows; t++) {
    chars += key_string(key_id(row0 + t, left));
    off[(size_t)t + 1] = (int32_t)chars.size();
    pay[(size_t)t] = (row0 + t) * 2 + (left ? 0 : 1);
  }
  auto kcol = std::make_unique<cudf::column>((cudf::size_type)rows, (int64_t)chars.size());
  CHECK(hipMemcpy(kcol->head(), off.data(), off.size() * 4, hipMemcpyHostToDevice));
  if (!chars.empty())
    CHECK(hipMemcpy(kcol->chars(), chars.data(), chars.size(), hipMemcpyHostToDevice));
  auto pcol = std::make_unique<cudf::column>(cudf::data_type(cudf::type_id::INT64),
                                             (cudf::size_type)rows);
  if (rows) CHECK(hipMemcpy(pcol->head(), pay.data(), (size_t)rows * 8, hipMemcpyHostToDevice));
  std::vector<std::unique_ptr<cudf::column>> cols;
  cols.push_back(std::move(kcol));
  cols.push_back(std::move(pcol));
  return std::make_unique<cudf::table>(std::move(cols));
}

static std::vector<std::string> strings_of(const cudf::column& col)
{
  const int64_t n = col.size();
  std::vector<int32_t> off((size_t)n + 1);
  CHECK(hipMemcpy(off.data(), col.head(), ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
  std::string ch((size_t)col.chars_size(), '\0');
  if (col.chars_size())
    CHECK(hipMemcpy(&ch[0], col.chars(), (size_t)col.chars_size(), hipMemcpyDeviceToHost));
  std::vector<std::string> out((size_t)n);
  for (int64_t i = 0; i < n; i++)
    out[(size_t)i] = ch.substr((size_t)off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i]));
  return out;
}

static std::vector<int64_t> i64_of(const cudf::column& col)
{
  std::vector<int64_t> v((size_t)col.size());
  if (col.size())
    CHECK(hipMemcpy(v.data(), col.head(), (size_t)col.size() * 8, hipMemcpyDeviceToHost));
  return v;
}

static uint64_t fold(const std::string& s)
{
  uint64_t h = 1469598103934665603ull ^ s.size();
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

/* order-insensitive checksum over (STRING, INT64, STRING, INT64) join rows */
static void checksum(const cudf::table& t, uint64_t* sum, int64_t* rows)
{
  if (t.num_columns() != 4 || t.get_column(0).type().id() != cudf::type_id::STRING ||
      t.get_column(2).type().id() != cudf::type_id::STRING) {
    printf("JOIN OUTPUT SCHEMA WRONG\n");
    exit(1);
  }
  auto lk = strings_of(t.get_column(0));
  auto rk = strings_of(t.get_column(2));
  auto lp = i64_of(t.get_column(1));
  auto rp = i64_of(t.get_column(3));
  uint64_t s = 0;
  for (size_t i = 0; i < lk.size(); i++) {
    if (lk[i] != rk[i]) {
      printf("JOIN ROW WITH UNEQUAL KEYS\n");
      exit(1);
    }
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
    std::vector<std::thread> th;
    for (int r = 0; r < G; r++) {
      th.emplace_back([&, r] {
        CHECK(hipSetDevice(0));
        LoopbackComm comm(r, G, &mb);
        auto t = make_table(r * per, per, true);
        auto opts = generate_compression_options_distributed(t->view(), compress);
        auto shuffled = shuffle_on(t->view(), {0}, &comm, opts, cudf::hash_id::HASH_MURMUR3,
                                   12345678u);
        keys_on[(size_t)r] = strings_of(shuffled->get_column(0));
      });
    }
    for (auto& t : th) t.join();
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
    std::vector<std::thread> th;
    for (int r = 0; r < G; r++) {
      th.emplace_back([&, r] {
        CHECK(hipSetDevice(0));
        LoopbackComm comm(r, G, &mb);
        auto left = make_table(r * per, per, true);
        auto right = make_table(r * per, per, false);
        auto lo = generate_compression_options_distributed(left->view(), compress);
        auto ro = generate_compression_options_distributed(right->view(), compress);
        auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, &comm, lo, ro,
                                          2, false, nullptr, nvl);
        checksum(*res, &sums[(size_t)r], &rows[(size_t)r]);
      });
    }
    for (auto& t : th) t.join();
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
