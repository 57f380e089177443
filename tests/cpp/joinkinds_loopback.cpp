/*
 * joinkinds_loopback.cpp — left / left semi / left anti joins across G ranks
 * on ONE GPU. Ranks run as host threads over the counting loopback
 * Communicator of loopback.hpp; the host tables and the host join are those
 * of host_table.hpp.
 *
 * usage: joinkinds_loopback G rows_per_rank
 *
 * Checks (global tables of G * rows_per_rank rows, a formula of the row):
 *   1. each of LEFT, LEFT_SEMI, LEFT_ANTI against a host join of the global
 *      tables: row count and an order-insensitive checksum over every value
 *      and validity bit —
 *        a. on a nullable key: null-key rows all meet on one rank; run once
 *           with null keys on both sides and (LEFT, ANTI) once with none on
 *           the right, where every null left key appears exactly once;
 *        b. on a non-nullable key, where one rank passes a left payload
 *           column WITHOUT a mask: the output column still has a mask on
 *           every rank;
 *      a LEFT result masks every right-hand column on every rank;
 *   2. the same semi join with the right table as keys only and with three
 *      wide payload columns behind the key: the Communicator sees identical
 *      send and receive bytes — right-hand payloads stay home;
 *   3. (G = 8) one LEFT join with nvlink_domain_size 4, i.e. through the
 *      inter-domain stage.
 *
 * Build/run: tests/test_gpu_join_kinds_loopback.py.
 */
#include "host_table.hpp"
#include "loopback.hpp"

#include "compression.hpp"
#include "distributed_join.hpp"

#include <algorithm>
#include <mutex>

static const char* kind_name(join_kind k)
{
  return k == join_kind::LEFT ? "left" : k == join_kind::LEFT_SEMI ? "semi" : "anti";
}

struct RunResult {
  long long rows, send_bytes, recv_bytes;
  uint64_t sum;
};

/* one distributed join of `kind` over G ranks, checked against the host join */
static RunResult check_join(join_kind kind, int G, int64_t R, bool null_keys, int domain,
                            RightShape shape = kRightPlain, bool right_nulls = true)
{
  /* right keys draw from two thirds of the left keys' values, so about a
   * third of the left keys have no partner; with a non-nullable key one rank
   * passes column 1 of the left table without a mask */
  TablePair tp(G, R, null_keys);
  tp.right_distinct = std::max<int64_t>(2, tp.distinct * 2 / 3);
  tp.maskless = null_keys ? kMasklessNone : kMasklessLeft;
  tp.shape = shape;
  tp.right_nulls = right_nulls;
  long long want_rows = 0, got_rows = 0;
  uint64_t want_sum = 0, got_sum = 0;
  host_join(kind, global_table(tp, true), global_table(tp, false), &want_rows, &want_sum);
  Mailbox mb;
  std::mutex m;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto left = to_device(rank_table(tp, r, true));
    auto right = to_device(rank_table(tp, r, false));
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    std::unique_ptr<cudf::table> res;
    if (kind == join_kind::LEFT)
      res = distributed_left_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, 2, false,
                                  nullptr, domain);
    else
      res = distributed_join(kind, left->view(), right->view(), {0}, {0}, comm, lo, ro, 1, false,
                             nullptr, domain);
    const int nl = left->num_columns();
    const int want_cols = nl + (kind == join_kind::LEFT ? right->num_columns() : 0);
    if (res->num_columns() != want_cols) FAIL("JOIN OUTPUT SCHEMA WRONG");
    for (int c = 0; c < want_cols; c++) {
      /* left side: a mask where any rank passed one; right side of LEFT: always */
      const bool want_mask = c >= nl || c != 0 || null_keys;
      if (res->get_column(c).nullable() != want_mask)
        FAIL("rank %d: output column %d nullable=%d, expected %d", r, c,
             (int)res->get_column(c).nullable(), (int)want_mask);
    }
    long long rows = 0;
    uint64_t sum = 0;
    output_sum(kind, from_device(*res), (size_t)nl, &rows, &sum);
    std::lock_guard<std::mutex> g(m);
    got_rows += rows;
    got_sum += sum;
  });
  printf("%s G=%d R=%lld null_keys=%d right_nulls=%d domain=%d shape=%d: host rows=%lld sum=%llx; got rows=%lld "
         "sum=%llx; send_bytes=%lld recv_bytes=%lld\n",
         kind_name(kind), G, (long long)R, (int)null_keys, (int)right_nulls, domain, (int)shape,
         want_rows,
         (unsigned long long)want_sum, got_rows, (unsigned long long)got_sum,
         mb.send_bytes.load(), mb.recv_bytes.load());
  if (want_rows != got_rows || want_sum != got_sum) FAIL("JOIN KINDS LOOPBACK MISMATCH");
  if (want_rows == 0) FAIL("JOIN KINDS LOOPBACK: empty reference result checks nothing");
  return RunResult{got_rows, mb.send_bytes.load(), mb.recv_bytes.load(), got_sum};
}

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int64_t R = argc > 2 ? atoll(argv[2]) : 1000;
  if (G < 2 || G > 16 || R < 1) FAIL("usage: joinkinds_loopback G(2..16) rows_per_rank");
  CHECK(hipSetDevice(0));
  for (join_kind kind : {join_kind::LEFT, join_kind::LEFT_SEMI, join_kind::LEFT_ANTI}) {
    check_join(kind, G, R, /*null_keys=*/true, /*domain=*/G);
    check_join(kind, G, R, /*null_keys=*/false, /*domain=*/G);
  }
  /* null left keys without a partner: each appears once, padded (LEFT) or
   * kept (ANTI), although all of them meet on one rank */
  check_join(join_kind::LEFT, G, R, true, G, kRightPlain, /*right_nulls=*/false);
  check_join(join_kind::LEFT_ANTI, G, R, true, G, kRightPlain, /*right_nulls=*/false);
  /* payloads stay home: the wire sees the same bytes whatever rides behind
   * the right table's key */
  const RunResult keys = check_join(join_kind::LEFT_SEMI, G, R, true, G, kRightKeysOnly);
  const RunResult wide = check_join(join_kind::LEFT_SEMI, G, R, true, G, kRightWide);
  if (keys.send_bytes != wide.send_bytes || keys.recv_bytes != wide.recv_bytes)
    FAIL("SEMI JOIN SHIPPED RIGHT-HAND PAYLOAD BYTES (%lld/%lld vs %lld/%lld)", wide.send_bytes,
         wide.recv_bytes, keys.send_bytes, keys.recv_bytes);
  if (keys.rows != wide.rows || keys.sum != wide.sum) FAIL("SEMI JOIN DEPENDS ON RIGHT PAYLOADS");
  if (keys.send_bytes == 0) FAIL("SEMI JOIN SENT NOTHING");
  if (G == 8) check_join(join_kind::LEFT, G, R, true, /*domain=*/4);
  printf("JOIN KINDS LOOPBACK OK\n");
  return 0;
}
