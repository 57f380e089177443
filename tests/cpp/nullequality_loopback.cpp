/*
 * nullequality_loopback.cpp — null_equality::UNEQUAL joins of every kind across
 * G ranks on ONE GPU. Ranks run as host threads over the counting loopback
 * Communicator of loopback.hpp; the host tables and the host join are those
 * of host_table.hpp (key on column 0, nullable, the values under its nulls
 * are 1 and -1, both valid keys of the other side).
 *
 * usage: nullequality_loopback G rows_per_rank
 *
 * Checks (global tables of G * rows_per_rank rows):
 *   1. each of INNER, LEFT, LEFT_SEMI, LEFT_ANTI under UNEQUAL against the
 *      host model: the host join of the globally stripped tables (no row with
 *      a null key), plus the stripped left rows for LEFT (null-padded) and
 *      LEFT_ANTI — row count and an order-insensitive checksum over every
 *      value and validity bit;
 *   2. the same kind under EQUAL on tables the host stripped beforehand: the
 *      Mailbox counts the same number of sends and the same send bytes as in
 *      the UNEQUAL run — null-key rows never reach the communicator;
 *   3. a LEFT_SEMI run and a LEFT run whose null-key right rows carry longer
 *      strings in an extra STRING payload column, every valid-key row staying
 *      as it was: the same wire bytes and (LEFT_SEMI) the same result;
 *   4. (G = 8) the LEFT join once more with nvlink_domain_size 4, i.e. through
 *      the inter-domain stage, against the same model and the same wire rule.
 *
 * Build/run: tests/test_gpu_null_equality_loopback.py.
 */
#include "host_table.hpp"
#include "loopback.hpp"

#include "compression.hpp"
#include "distributed_join.hpp"

#include <algorithm>
#include <mutex>

static const char* kind_name(join_kind k)
{
  return k == join_kind::INNER  ? "inner"
         : k == join_kind::LEFT ? "left"
         : k == join_kind::LEFT_SEMI ? "semi"
                                     : "anti";
}

/* the rows of t whose key (column 0) is valid, or the others; masks stay */
static HTable key_rows(const HTable& t, bool valid_keys)
{
  HTable out = t;
  for (auto& c : out) {
    c.v.clear();
    c.s.clear();
    c.valid.clear();
  }
  for (size_t i = 0; i < rows_of(t); i++) {
    if ((bool)t[0].valid[i] != valid_keys) continue;
    for (size_t c = 0; c < t.size(); c++) {
      if (t[c].type == cudf::type_id::STRING)
        out[c].s.push_back(t[c].s[i]);
      else
        out[c].v.push_back(t[c].v[i]);
      out[c].valid.push_back(t[c].valid[i]);
    }
  }
  return out;
}

static void append(HTable& all, const HTable& t)
{
  if (all.empty()) {
    all = t;
    return;
  }
  for (size_t c = 0; c < t.size(); c++) {
    all[c].v.insert(all[c].v.end(), t[c].v.begin(), t[c].v.end());
    all[c].s.insert(all[c].s.end(), t[c].s.begin(), t[c].s.end());
    all[c].valid.insert(all[c].valid.end(), t[c].valid.begin(), t[c].valid.end());
  }
}

/* the host model of UNEQUAL: the null == null host join of the stripped
 * tables, plus the stripped left rows for LEFT (padded) and LEFT_ANTI */
static void host_join_unequal(join_kind kind, const HTable& l, const HTable& r, long long* rows,
                              uint64_t* sum)
{
  host_join(kind, key_rows(l, true), key_rows(r, true), rows, sum);
  if (kind != join_kind::LEFT && kind != join_kind::LEFT_ANTI) return;
  const HTable nulls = key_rows(l, false);
  const uint64_t pad = null_row_hash(r.size());
  for (size_t i = 0; i < rows_of(nulls); i++) {
    const uint64_t lh = row_hash(nulls, 0, nulls.size(), i);
    *sum += kind == join_kind::LEFT ? dj_mix64(lh ^ dj_mix64(pad)) : dj_mix64(lh);
    (*rows)++;
  }
}

/* what rides behind the right table's columns */
enum RightExtra {
  kNoExtra,
  kExtraStrings,     /* a STRING payload column, str_of(row) */
  kExtraLongOnNulls  /* the same, 40 bytes longer in the null-key rows */
};

static HTable make_rank_table(const TablePair& tp, int r, bool left, RightExtra extra)
{
  HTable t = rank_table(tp, r, left);
  if (left || extra == kNoExtra) return t;
  HCol c;
  c.type = cudf::type_id::STRING;
  c.mask = true;
  for (size_t i = 0; i < rows_of(t); i++) {
    std::string s = str_of((uint64_t)(r * tp.R) + i + 77);
    if (extra == kExtraLongOnNulls && !t[0].valid[i]) s += std::string(40, 'z');
    c.s.push_back(s);
    c.valid.push_back(i % 5 != 0);
  }
  t.push_back(c);
  return t;
}

struct RunResult {
  long long rows, sends, send_bytes;
  uint64_t sum;
};

/* one distributed join of `kind` over G ranks under `mode`; with pre_strip the
 * host removes every null-key row from each rank's tables first. Checked
 * against the host model either way (on stripped tables the two modes agree). */
static RunResult check_join(join_kind kind, int G, int64_t R, int domain,
                            cudf::null_equality mode, bool pre_strip,
                            RightExtra extra = kNoExtra, RightShape shape = kRightPlain)
{
  TablePair tp(G, R, /*null_keys=*/true);
  tp.right_distinct = std::max<int64_t>(2, tp.distinct * 2 / 3);
  tp.every = 5;  // one key in five is null
  tp.shape = shape;
  HTable gl, gr;
  std::vector<HTable> ls, rs;
  for (int r = 0; r < G; r++) {
    HTable l = make_rank_table(tp, r, true, extra), rt = make_rank_table(tp, r, false, extra);
    if (pre_strip) {
      l = key_rows(l, true);
      rt = key_rows(rt, true);
    }
    append(gl, l);
    append(gr, rt);
    ls.push_back(std::move(l));
    rs.push_back(std::move(rt));
  }
  long long want_rows = 0, got_rows = 0;
  uint64_t want_sum = 0, got_sum = 0;
  host_join_unequal(kind, gl, gr, &want_rows, &want_sum);
  if (!pre_strip && rows_of(key_rows(gl, false)) * 10 < rows_of(gl))
    FAIL("NULL EQUALITY LOOPBACK: too few null keys to check anything");
  Mailbox mb;
  std::mutex m;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto left = to_device(ls[(size_t)r]);
    auto right = to_device(rs[(size_t)r]);
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    std::unique_ptr<cudf::table> res;
    if (kind == join_kind::LEFT)
      res = distributed_left_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, 1, false,
                                  nullptr, domain, mode);
    else
      res = distributed_join(kind, left->view(), right->view(), {0}, {0}, comm, lo, ro, 1, false,
                             nullptr, domain, mode);
    const bool pairs = kind == join_kind::INNER || kind == join_kind::LEFT;
    const int nl = left->num_columns();
    const int want_cols = nl + (pairs ? right->num_columns() : 0);
    if (res->num_columns() != want_cols) FAIL("JOIN OUTPUT SCHEMA WRONG");
    /* every source column carries a mask here, so every output column does */
    for (int c = 0; c < want_cols; c++)
      if (!res->get_column(c).nullable()) FAIL("rank %d: output column %d has no mask", r, c);
    long long rows = 0;
    uint64_t sum = 0;
    output_sum(kind, from_device(*res), (size_t)nl, &rows, &sum);
    std::lock_guard<std::mutex> g(m);
    got_rows += rows;
    got_sum += sum;
  });
  printf("%s G=%d R=%lld unequal=%d pre_strip=%d domain=%d extra=%d shape=%d: host rows=%lld "
         "sum=%llx; got rows=%lld sum=%llx; sends=%lld send_bytes=%lld\n",
         kind_name(kind), G, (long long)R, (int)(mode == cudf::null_equality::UNEQUAL),
         (int)pre_strip, domain, (int)extra, (int)shape, want_rows, (unsigned long long)want_sum,
         got_rows, (unsigned long long)got_sum, mb.sends.load(), mb.send_bytes.load());
  if (want_rows != got_rows || want_sum != got_sum) FAIL("NULL EQUALITY LOOPBACK MISMATCH");
  if (want_rows == 0) FAIL("NULL EQUALITY LOOPBACK: empty reference result checks nothing");
  return RunResult{got_rows, mb.sends.load(), mb.send_bytes.load(), got_sum};
}

/* UNEQUAL on the full tables against EQUAL on host-stripped ones: the same wire */
static void check_kind(join_kind kind, int G, int64_t R, int domain)
{
  const RunResult sql = check_join(kind, G, R, domain, cudf::null_equality::UNEQUAL, false);
  const RunResult pre = check_join(kind, G, R, domain, cudf::null_equality::EQUAL, true);
  if (sql.sends != pre.sends || sql.send_bytes != pre.send_bytes)
    FAIL("%s: NULL-KEY ROWS REACHED THE COMMUNICATOR (sends %lld vs %lld, bytes %lld vs %lld)",
         kind_name(kind), sql.sends, pre.sends, sql.send_bytes, pre.send_bytes);
  if (sql.send_bytes == 0) FAIL("%s: SENT NOTHING", kind_name(kind));
}

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int64_t R = argc > 2 ? atoll(argv[2]) : 1000;
  if (G < 2 || G > 16 || R < 1) FAIL("usage: nullequality_loopback G(2..16) rows_per_rank");
  CHECK(hipSetDevice(0));
  const cudf::null_equality sql = cudf::null_equality::UNEQUAL;
  for (join_kind kind :
       {join_kind::INNER, join_kind::LEFT, join_kind::LEFT_SEMI, join_kind::LEFT_ANTI})
    check_kind(kind, G, R, /*domain=*/G);
  /* what the null-key right rows carry never matters to the wire */
  const RunResult semi = check_join(join_kind::LEFT_SEMI, G, R, G, sql, false, kExtraStrings);
  const RunResult semi_long =
    check_join(join_kind::LEFT_SEMI, G, R, G, sql, false, kExtraLongOnNulls);
  if (semi.send_bytes != semi_long.send_bytes || semi.sends != semi_long.sends)
    FAIL("SEMI JOIN WIRE DEPENDS ON NULL-KEY RIGHT ROWS (%lld vs %lld bytes)", semi.send_bytes,
         semi_long.send_bytes);
  if (semi.rows != semi_long.rows || semi.sum != semi_long.sum)
    FAIL("SEMI JOIN DEPENDS ON NULL-KEY RIGHT ROWS");
  const RunResult left = check_join(join_kind::LEFT, G, R, G, sql, false, kExtraStrings);
  const RunResult left_long = check_join(join_kind::LEFT, G, R, G, sql, false, kExtraLongOnNulls);
  if (left.send_bytes != left_long.send_bytes || left.sends != left_long.sends)
    FAIL("LEFT JOIN SHIPPED NULL-KEY RIGHT ROWS (%lld vs %lld bytes)", left.send_bytes,
         left_long.send_bytes);
  if (left.rows != left_long.rows || left.sum != left_long.sum)
    FAIL("LEFT JOIN DEPENDS ON NULL-KEY RIGHT ROWS");
  if (G == 8) check_kind(join_kind::LEFT, G, R, /*domain=*/4);
  printf("NULL EQUALITY LOOPBACK OK\n");
  return 0;
}
