/*
 * null_loopback.cpp — validity masks across G ranks on ONE GPU. Ranks run as
 * host threads over a loopback implementation of the public Communicator
 * interface (loopback.hpp), which counts its send/recv calls and bytes; the
 * host tables and the host join are those of host_table.hpp.
 *
 * usage: null_loopback G rows_per_rank
 *
 * Checks (global tables of G * rows_per_rank rows, a formula of the row):
 *   1. shuffle_on on a nullable INT64 key: no row, value or validity bit is
 *      lost; every null-key row sits on rank 0xFFFFFFFF % G; a valid key
 *      lives on one rank;
 *   2. distributed_inner_join on a nullable key (null == null, the a*b cross
 *      product included; garbage under nulls equal to valid keys of the other
 *      side) against a host join of the global tables: row count and an
 *      order-insensitive checksum over every value and validity bit;
 *   3. the same with a non-nullable key, nullable payloads and
 *      over_decom_factor 2 (the batched pipeline);
 *   in 1-3 one rank passes one payload column WITHOUT a mask while the others
 *   pass masks: the output column still has a mask on every rank;
 *   4. distribute_table, collect_tables and the generic plan API refuse a
 *      nullable table with an exception, before any communication;
 *   5. mask-free tables: the Communicator sees exactly the send/recv calls
 *      and bytes it saw before masks existed. The program prints them as a
 *      "COUNTS" line; tests/test_gpu_nulls.py holds the values recorded from
 *      the commit before validity masks.
 *
 * Built with -DNULL_LOOPBACK_COUNTS_ONLY the program contains check 5 alone
 * and uses nothing newer than the mask-free interface (that is how the
 * recorded values were taken).
 *
 * Build/run: tests/test_gpu_nulls.py::test_null_loopback.
 */
#ifdef NULL_LOOPBACK_COUNTS_ONLY
#define HOST_TABLE_NO_MASKS
#endif
#include "host_table.hpp"
#include "loopback.hpp"

#include "all_to_all_comm.hpp"
#include "compression.hpp"
#include "distribute_table.hpp"
#include "distributed_join.hpp"
#include "shuffle_on.hpp"

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

/* ---------------- check 5: mask-free call and byte counts ---------------- */

/* rows [row0, row0+rows) of a mask-free (INT64 key, INT32, STRING) table, or
 * of an (INT64 key, INT64) pair when `pair` */
static std::unique_ptr<cudf::table> plain_table(int64_t row0, int64_t rows, bool left, bool pair,
                                                int64_t distinct)
{
  std::vector<int64_t> key((size_t)rows), p64((size_t)rows);
  std::vector<int32_t> p32((size_t)rows);
  std::vector<std::string> ps((size_t)rows);
  for (int64_t t = 0; t < rows; t++) {
    const uint64_t g = (uint64_t)(row0 + t) + (left ? 0ull : 1000003ull);
    key[(size_t)t] = (int64_t)(dj_mix64(g) % (uint64_t)distinct);
    p64[(size_t)t] = (int64_t)g * 3;
    p32[(size_t)t] = (int32_t)(g * 7);
    ps[(size_t)t] = str_of(g);
  }
  std::vector<std::unique_ptr<cudf::column>> cols;
  cols.push_back(device_fixed(cudf::type_id::INT64, key.data(), rows, 8));
  if (pair) {
    cols.push_back(device_fixed(cudf::type_id::INT64, p64.data(), rows, 8));
  } else {
    cols.push_back(device_fixed(cudf::type_id::INT32, p32.data(), rows, 4));
    cols.push_back(device_strings(ps));
  }
  return std::make_unique<cudf::table>(std::move(cols));
}

static void count_mask_free(int G, int64_t R)
{
  const int64_t distinct = std::max<int64_t>(4, G * R / 3);
  Mailbox mb;
  std::atomic<long long> out_rows{0};
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    for (int pair = 0; pair < 2; pair++) {
      auto left = plain_table(r * R, R, true, pair != 0, distinct);
      auto right = plain_table(r * R, R, false, pair != 0, distinct);
      auto lo = generate_compression_options_distributed(left->view(), false);
      auto ro = generate_compression_options_distributed(right->view(), false);
      auto sh = shuffle_on(left->view(), {0}, comm, lo, cudf::hash_id::HASH_MURMUR3, 12345678u);
      auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, 2,
                                        false, nullptr, G);
      out_rows += sh->num_rows() + res->num_rows();
    }
  });
  printf("COUNTS G=%d R=%lld sends=%lld recvs=%lld send_bytes=%lld recv_bytes=%lld rows=%lld\n",
         G, (long long)R, mb.sends.load(), mb.recvs.load(), mb.send_bytes.load(),
         mb.recv_bytes.load(), out_rows.load());
}

#ifndef NULL_LOOPBACK_COUNTS_ONLY

/* the tables of checks 1-3: both sides draw their keys from the same values,
 * and one rank passes column 1 of the right table without a mask */
static TablePair tables_of(int G, int64_t R, bool null_keys)
{
  TablePair p(G, R, null_keys);
  p.maskless = kMasklessRight;
  return p;
}

static void check_join(int G, int64_t R, bool null_keys, int od)
{
  const TablePair tp = tables_of(G, R, null_keys);
  long long want_rows = 0, got_rows = 0;
  uint64_t want_sum = 0, got_sum = 0;
  host_join(join_kind::INNER, global_table(tp, true), global_table(tp, false), &want_rows,
            &want_sum);
  Mailbox mb;
  std::mutex m;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto left = to_device(rank_table(tp, r, true));
    auto right = to_device(rank_table(tp, r, false));
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, od,
                                      false, nullptr, G);
    if (res->num_columns() != 6) FAIL("JOIN OUTPUT SCHEMA WRONG");
    for (int c = 0; c < 6; c++) {
      const bool want_mask = (c != 0 && c != 3) || null_keys;
      if (res->get_column(c).nullable() != want_mask)
        FAIL("rank %d: output column %d nullable=%d, expected %d", r, c,
             (int)res->get_column(c).nullable(), (int)want_mask);
    }
    long long rows = 0;
    uint64_t sum = 0;
    output_sum(join_kind::INNER, from_device(*res), 3, &rows, &sum);
    std::lock_guard<std::mutex> g(m);
    got_rows += rows;
    got_sum += sum;
  });
  printf("join G=%d R=%lld null_keys=%d od=%d: host rows=%lld sum=%llx; got rows=%lld sum=%llx\n",
         G, (long long)R, (int)null_keys, od, want_rows, (unsigned long long)want_sum, got_rows,
         (unsigned long long)got_sum);
  if (want_rows != got_rows || want_sum != got_sum) FAIL("NULL LOOPBACK JOIN MISMATCH");
}

static void check_shuffle(int G, int64_t R)
{
  const TablePair tp = tables_of(G, R, true);
  const HTable all = global_table(tp, false);
  uint64_t want_sum = 0, got_sum = 0;
  for (size_t i = 0; i < rows_of(all); i++) want_sum += dj_mix64(row_hash(all, 0, 3, i));
  Mailbox mb;
  std::mutex m;
  std::map<std::string, int> owner;
  long long got_rows = 0;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto t = to_device(rank_table(tp, r, false));
    auto opts = generate_compression_options_distributed(t->view(), false);
    auto sh = shuffle_on(t->view(), {0}, comm, opts, cudf::hash_id::HASH_MURMUR3, 12345678u);
    for (int c = 0; c < 3; c++)
      if (!sh->get_column(c).nullable()) FAIL("rank %d: shuffled column %d lost its mask", r, c);
    HTable h = from_device(*sh);
    std::lock_guard<std::mutex> g(m);
    for (size_t i = 0; i < rows_of(h); i++) {
      got_sum += dj_mix64(row_hash(h, 0, 3, i));
      got_rows++;
      const std::string k = key_code(h, i);
      if (k == "n" && r != (int)(0xFFFFFFFFu % (unsigned)G))
        FAIL("NULL KEY ROW ON RANK %d, expected %u", r, 0xFFFFFFFFu % (unsigned)G);
      auto it = owner.emplace(k, r).first;
      if (it->second != r) FAIL("KEY ON TWO RANKS (%d and %d)", it->second, r);
    }
  });
  printf("shuffle G=%d R=%lld: rows=%lld sum=%llx (want %zu, %llx)\n", G, (long long)R, got_rows,
         (unsigned long long)got_sum, rows_of(all), (unsigned long long)want_sum);
  if (got_rows != (long long)rows_of(all) || got_sum != want_sum)
    FAIL("NULL LOOPBACK SHUFFLE MISMATCH");
}

/* the entry points that do not carry masks say so */
static void check_refusals()
{
  Mailbox mb;
  LoopbackComm comm(0, 1, &mb);
  auto t = to_device(host_table(0, 8, false, true, 4, 3));
  int refused = 0;
  try {
    distribute_table(t->view(), &comm);
  } catch (std::runtime_error const&) {
    refused++;
  }
  try {
    collect_tables(t->view(), &comm);
  } catch (std::runtime_error const&) {
    refused++;
  }
  try {
    std::vector<AllToAllCommBuffer> bufs;
    append_to_all_to_all_comm_buffers(t->view(), t->mutable_view(), {0, 8}, {0, 8}, bufs,
                                      generate_none_compression_options(t->view()));
  } catch (std::runtime_error const&) {
    refused++;
  }
  if (refused != 3 || mb.sends.load() != 0) FAIL("NULLABLE TABLE NOT REFUSED (%d of 3)", refused);
  printf("refusals OK\n");
}

#endif /* NULL_LOOPBACK_COUNTS_ONLY */

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int64_t R = argc > 2 ? atoll(argv[2]) : 5;
  if (G < 2 || G > 16 || R < 1) FAIL("usage: null_loopback G(2..16) rows_per_rank");
  CHECK(hipSetDevice(0));
  count_mask_free(G, R);
#ifndef NULL_LOOPBACK_COUNTS_ONLY
  check_refusals();
  check_shuffle(G, R);
  check_join(G, R, /*null_keys=*/true, /*od=*/1);
  check_join(G, R, /*null_keys=*/false, /*od=*/2);
  printf("NULL LOOPBACK OK\n");
#endif
  return 0;
}
