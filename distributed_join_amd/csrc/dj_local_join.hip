/*
 * dj_local_join.hip — the local join of two tables: the bucketed-LDS engine
 * behind a capacity retry, output assembly for INNER and for the LEFT kinds,
 * and the null-key handling of null_equality::UNEQUAL (dj_host.hpp).
 */
#include "dj_host.hpp"

namespace dj_host {

/* the bucketed-LDS engine with its capacity retry: rerun at the exact size
 * when the matches outnumber the first-try capacity. Host-synchronous. */
static std::pair<JoinOut, int64_t> run_bucket_join(const int64_t* lk, const int64_t* lp,
                                                   int64_t ln, const int64_t* rk,
                                                   const int64_t* rp, int64_t rn)
{
  hipStream_t st = dj_rt_stream();
  DBuf scratch((size_t)dj_bucket_join_scratch_bytes(ln, rn));
  int64_t cap = JoinOut::default_cap(rn);
  for (;;) {
    JoinOut out(cap);
    out.clear(st);
    dj_bucket_local_join(lk, lp, ln, rk, rp, rn, out.o0.i64(), out.o1.i64(), out.o2.i64(),
                         out.o3.i64(), cap, out.counter(), out.error(), scratch.p);
    const JoinMeta m = read_back<JoinMeta>(out.meta.p, st);
    DJ_CHECK_ERROR(m.error == 0, "join: sentinel flag not cleared by the bucket path");
    if (m.count <= cap) return {std::move(out), m.count};
    cap = m.count;
  }
}

/* appends one 0-row column per column of t; masked where the source is, or
 * everywhere (the right-hand side of a left join) */
static void append_empty_columns(cudf::table_view t, bool all_masked,
                                 std::vector<std::unique_ptr<cudf::column>>& cols)
{
  for (cudf::size_type c = 0; c < t.num_columns(); c++) {
    if (is_string(t.column(c)))
      cols.push_back(std::make_unique<cudf::column>((cudf::size_type)0, (int64_t)0));
    else
      cols.push_back(std::make_unique<cudf::column>(t.column(c).type(), (cudf::size_type)0));
    if (all_masked || t.column(c).nullable()) {
      cols.back()->allocate_null_mask();
      cols.back()->set_null_count(0);
    }
  }
}

std::unique_ptr<cudf::table> empty_join_result(cudf::table_view left, cudf::table_view right)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  append_empty_columns(left, false, cols);
  append_empty_columns(right, false, cols);
  return std::make_unique<cudf::table>(std::move(cols));
}

/* the first n rows of the engine's four outputs as four INT64 columns */
static std::unique_ptr<cudf::table> adopt_i64x4(JoinOut& out, int64_t n)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (DBuf* d : {&out.o0, &out.o1, &out.o2, &out.o3}) {
    cols.push_back(std::make_unique<cudf::column>(cudf::data_type(cudf::type_id::INT64),
                                                  (cudf::size_type)n, d->p));
    d->p = nullptr;
  }
  return std::make_unique<cudf::table>(std::move(cols));
}

/* int64 pairs adopt the engine's outputs as they are. Otherwise o1/o3 hold
 * source row indices and every column is gathered — EXCEPT a single integer
 * key column (left_key / right_key >= 0), whose joined values already sit in
 * o0/o2 and are adopted or narrowed instead (see gather_table_columns) */
std::unique_ptr<cudf::table> assemble_join_output(cudf::table_view left, cudf::table_view right,
                                                  JoinOut& out, int64_t nout,
                                                  cudf::size_type left_key,
                                                  cudf::size_type right_key)
{
  if (joins_i64_pairs(left, right, left_key, right_key)) return adopt_i64x4(out, nout);
  hipStream_t st = dj_rt_stream();
  std::vector<std::unique_ptr<cudf::column>> cols;
  gather_table_columns(left, out.o1, nout, left_key, &out.o0, cols, st);
  gather_table_columns(right, out.o3, nout, right_key, &out.o2, cols, st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return std::make_unique<cudf::table>(std::move(cols));
}

/* LEFT / LEFT_SEMI / LEFT_ANTI from the pair list: out.o1[0..nout) are the
 * left row indices of the matching pairs (after the collision filter),
 * out.o3 the right ones; li_cap is the number of elements out.o1 has room
 * for. The matched left rows are marked in a bitmap of ln bits
 * (dj::mark_rows) and the kept row set is read back in ascending order
 * (dj::select_rows), so that the gather it feeds streams through the source.
 *   semi / anti: the left columns of the marked / unmarked rows
 *   left:        left columns by [o1 , unmatched] in one gather; right
 *                columns gathered for the nout pairs and null-padded for the
 *                nun unmatched rows in the same allocation — the inner part
 *                is written once
 * Host-synchronous. */
static std::unique_ptr<cudf::table> assemble_left_kind(join_kind kind, cudf::table_view left,
                                                       cudf::table_view right, JoinOut& out,
                                                       int64_t nout, int64_t li_cap)
{
  hipStream_t st = dj_rt_stream();
  const int64_t ln = left.num_rows();
  std::vector<std::unique_ptr<cudf::column>> cols;
  if (ln == 0) {
    append_empty_columns(left, false, cols);
    if (kind == join_kind::LEFT) append_empty_columns(right, true, cols);
    return std::make_unique<cudf::table>(std::move(cols));
  }
  const size_t bitmap_bytes = (size_t)((ln + 31) / 32) * 4;
  DBuf bits(bitmap_bytes), count(8);
  DBuf scratch(dj::select_rows_scratch_bytes(ln));
  DJ_HIP_CALL(hipMemsetAsync(bits.p, 0, bitmap_bytes, st));
  dj::mark_rows(out.o1.i64(), nout, (uint32_t*)bits.p, st);

  if (kind != join_kind::LEFT) {
    DBuf sel((size_t)ln * 8);
    dj::select_rows((const uint32_t*)bits.p, ln, kind == join_kind::LEFT_SEMI, sel.i64(),
                    count.i64(), st, scratch.p);
    const int64_t nsel = read_back<int64_t>(count.p, st);
    if (nsel == 0)
      append_empty_columns(left, false, cols);
    else
      gather_table_columns(left, sel, nsel, -1, nullptr, cols, st);
    DJ_HIP_CALL(hipStreamSynchronize(st));
    return std::make_unique<cudf::table>(std::move(cols));
  }

  /* the unmatched rows go straight behind the pairs' left indices */
  if (li_cap < nout + ln) {
    DBuf wide((size_t)(nout + ln) * 8);
    if (nout > 0)
      DJ_HIP_CALL(hipMemcpyAsync(wide.p, out.o1.p, (size_t)nout * 8, hipMemcpyDeviceToDevice, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));  // the old array returns to the pool
    out.o1 = std::move(wide);
  }
  dj::select_rows((const uint32_t*)bits.p, ln, false, out.o1.i64() + nout, count.i64(), st,
                  scratch.p);
  const int64_t nsel = read_back<int64_t>(count.p, st);
  DJ_CHECK_ERROR(nout + nsel <= INT32_MAX, "left join: output exceeds 2^31 rows");
  gather_table_columns(left, out.o1, nout + nsel, -1, nullptr, cols, st);
  gather_table_columns(right, out.o3, nout, -1, nullptr, cols, st, nsel);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return std::make_unique<cudf::table>(std::move(cols));
}

static dj::TupleKeyCol tuple_key_col(cudf::column_view col)
{
  dj::TupleKeyCol d{};
  d.data = col.head<void>();
  d.chars = (const uint8_t*)col.chars();
  d.kind = is_string(col) ? (int)dj::kKeyStr : key_kind(col.type());
  d.valid = col.null_mask();
  return d;
}

/* ---- null_equality::UNEQUAL: a row with a null anywhere in its key tuple
 * matches nothing, so it never enters the engine ---- */

/* which rows of a table hold no null in their key tuple */
struct KeyRowValidity {
  DBuf own;                       // the AND of the key masks, where it had to be built
  const uint32_t* bits{nullptr};  // 1 = no null in the tuple; nullptr: every row
  int64_t nnull{0};               // rows with a null in their tuple
};

/* Only the key columns that may hold a null take part. With exactly one, that
 * column's mask IS the row validity (select_rows and compact_keyed_rows
 * ignore its bits past the row count) and only its nulls are counted.
 * Host-synchronous when a mask takes part. */
static KeyRowValidity key_row_validity(cudf::table_view t,
                                       std::vector<cudf::size_type> const& on, hipStream_t st)
{
  KeyRowValidity v;
  const uint32_t* masks[dj::kMaxKeyMasks];
  int nm = 0;
  for (auto c : on) {
    cudf::column_view col = t.column(c);
    if (!col.nullable() || col.null_count() == 0) continue;
    DJ_CHECK_ERROR(nm < dj::kMaxKeyMasks, "up to 4 join key columns supported");
    masks[nm++] = col.null_mask();
  }
  const int64_t n = t.num_rows();
  if (nm == 0 || n == 0) return v;
  /* the number of null-key rows sizes the compacted arrays, so it is counted
   * from the bits here and not taken from a view's null_count */
  DBuf cnt(8);
  DJ_HIP_CALL(hipMemsetAsync(cnt.p, 0, 8, st));
  if (nm == 1) {
    dj::count_unset_bits(masks[0], n, (unsigned long long*)cnt.p, st);
  } else {
    v.own = DBuf((size_t)((n + 31) / 32) * 4);
    dj::key_row_validity(masks, nm, n, (uint32_t*)v.own.p, (unsigned long long*)cnt.p, st);
  }
  v.nnull = (int64_t)read_back<unsigned long long>(cnt.p, st);
  if (v.nnull > 0) v.bits = nm == 1 ? masks[0] : (const uint32_t*)v.own.p;
  return v;
}

/* the engine's view of one side under UNEQUAL: the keys of the valid-key
 * rows and, as the payload, their row numbers in the table */
struct CompactedKeys {
  DBuf keys, rows;
  int64_t n{0};
};

static CompactedKeys compact_valid_keys(KeyRowValidity const& v, const int64_t* keys,
                                        int64_t nrows, hipStream_t st)
{
  CompactedKeys c;
  c.n = nrows - v.nnull;
  if (c.n <= 0) return c;
  c.keys = DBuf((size_t)c.n * 8);
  c.rows = DBuf((size_t)c.n * 8);
  DBuf scratch(dj::select_rows_scratch_bytes(nrows)), count(8);
  dj::compact_keyed_rows(v.bits, nrows, keys, c.rows.i64(), c.keys.i64(), count.i64(), st,
                         scratch.p);
  const int64_t got = read_back<int64_t>(count.p, st);
  DJ_CHECK_ERROR(got == c.n, "join: a key column's null_count disagrees with its mask");
  return c;
}

/* INNER returns left-cols + right-cols with keys duplicated, row order
 * unspecified; the other kinds build the same pair list and hand it to
 * assemble_left_kind. A single integer key column is the engine's key as it
 * is (widened when narrow). Composite keys, and STRING keys even alone,
 * bucket-join on the fused key chain (fuse_keys: the row hash stands in for
 * a string) with row-index payloads, then drop fused-hash collisions against
 * the real columns — the single-key engine does the heavy lifting; only
 * placement/equality semantics widen. (Reference: cudf::inner_join on
 * arbitrary left_on/right_on, distributed_join.cpp:71-132.) */
std::unique_ptr<cudf::table> local_join(
  join_kind kind, cudf::table_view left, cudf::table_view right,
  std::vector<cudf::size_type> const& lon, std::vector<cudf::size_type> const& ron,
  cudf::null_equality compare_nulls)
{
  const bool inner = kind == join_kind::INNER;
  const bool sql = compare_nulls == cudf::null_equality::UNEQUAL;
  DJ_CHECK_ERROR(lon.size() == ron.size(), "left_on/right_on must have equal length");
  bool str_keys = false;
  for (size_t c = 0; c < lon.size(); c++) {
    const bool ls = is_string(left.column(lon[c])), rs = is_string(right.column(ron[c]));
    DJ_CHECK_ERROR(ls == rs, "a STRING key column must pair with a STRING key column");
    str_keys |= ls;
  }
  /* under null_equality::EQUAL nullable keys take the fused route too:
   * fuse_keys gives every null element one constant, so all-null tuples meet
   * in the bucket join, and the tuple filter applies EQUAL against the masks.
   * Under UNEQUAL the null-key rows stay out of the engine (below), so a
   * single integer key runs unfused whatever its mask; composite and STRING
   * keys still fuse, and every tuple their filter sees is fully valid. */
  const bool fused = lon.size() > 1 || str_keys ||
                     (!sql && (any_nullable_key(left, lon) || any_nullable_key(right, ron)));
  hipStream_t st = dj_rt_stream();
  const int64_t ln = left.num_rows(), rn = right.num_rows();
  /* no pair list to build: every left row (if any) is unmatched */
  auto no_pairs = [&]() {
    if (inner) return empty_join_result(left, right);  // distributed_join.cpp:76-83
    JoinOut none;
    return assemble_left_kind(kind, left, right, none, 0, 0);
  };
  if (ln == 0 || rn == 0) return no_pairs();
  /* UNEQUAL: the rows of each side that hold a null in their key tuple. A
   * side left with no valid-key row is an empty side. */
  KeyRowValidity lvalid, rvalid;
  if (sql) {
    lvalid = key_row_validity(left, lon, st);
    rvalid = key_row_validity(right, ron, st);
    if (lvalid.nnull == ln || rvalid.nnull == rn) return no_pairs();
  }

  /* the output's key columns: known only for a single integer key (a fused
   * key's columns are gathered like any other) */
  const cudf::size_type left_key = fused ? -1 : lon[0], right_key = fused ? -1 : ron[0];
  DBuf lkey_tmp, rkey_tmp;
  const int64_t* lk;
  const int64_t* rk;
  if (fused) {
    lkey_tmp = fuse_keys(left, lon, st);
    rkey_tmp = fuse_keys(right, ron, st);
    lk = lkey_tmp.i64();
    rk = rkey_tmp.i64();
  } else {
    lk = key_as_i64(left.column(left_key), lkey_tmp);
    rk = key_as_i64(right.column(right_key), rkey_tmp);
  }
  /* general path payload = row index; the partition kernels synthesize it
   * (pay == nullptr -> i), so no iota arrays to materialize or re-read
   * (2.4 GB/step at the TPC-H shape) */
  /* the other kinds need the left row of every pair, so they always join on
   * row-index payloads, 2 x INT64 tables included */
  const bool pairs = inner && joins_i64_pairs(left, right, left_key, right_key);
  const int64_t* lp = pairs ? left.column(1).head<int64_t>() : nullptr;
  const int64_t* rp = pairs ? right.column(1).head<int64_t>() : nullptr;
  /* UNEQUAL with null keys: the engine joins the keys of the valid-key rows
   * and carries their row numbers as the payload, so the pair list comes back
   * in row numbers of the original tables: no column is compacted, the null
   * rows of the left stay unmarked (LEFT pads them, LEFT_ANTI keeps them)
   * and those of the right are in no pair */
  int64_t eln = ln, ern = rn;
  CompactedKeys lc, rc;
  if (lvalid.nnull > 0) {
    lc = compact_valid_keys(lvalid, lk, ln, st);
    lk = lc.keys.i64();
    lp = lc.rows.i64();
    eln = lc.n;
  }
  if (rvalid.nnull > 0) {
    rc = compact_valid_keys(rvalid, rk, rn, st);
    rk = rc.keys.i64();
    rp = rc.rows.i64();
    ern = rc.n;
  }

  auto joined = run_bucket_join(lk, lp, eln, rk, rp, ern);
  JoinOut& out = joined.first;
  int64_t nout = joined.second;
  int64_t li_cap = out.cap;  // elements the left-index array has room for
  if (fused) {
    /* collision filter: keep the (li, ri) pairs whose REAL key tuples are
     * equal (the bucket join matched on the fused hash; unequal tuples
     * sharing a fused value are hash collisions to drop). Output order is
     * unspecified (atomic append), as the join's own output order already is. */
    dj::TupleKeys tk{};
    tk.nk = (int)lon.size();
    for (size_t c = 0; c < lon.size(); c++) {
      tk.l[c] = tuple_key_col(left.column(lon[c]));
      tk.r[c] = tuple_key_col(right.column(ron[c]));
    }
    /* a left join appends its unmatched rows (at most ln) behind the pairs */
    li_cap = std::max<int64_t>(nout, 1) + (kind == join_kind::LEFT ? ln : 0);
    DBuf li2((size_t)li_cap * 8);
    DBuf ri2((size_t)std::max<int64_t>(nout, 1) * 8);
    out.clear(st);
    dj::filter_tuple_matches_mixed(tk, out.o1.i64(), out.o3.i64(), nout, li2.i64(), ri2.i64(),
                                   (unsigned long long*)out.counter(), st);
    nout = read_back<int64_t>(out.counter(), st);
    if (nout == 0 && inner) return empty_join_result(left, right);
    out.o1 = std::move(li2);
    out.o3 = std::move(ri2);
  }
  if (!inner) return assemble_left_kind(kind, left, right, out, nout, li_cap);
  return assemble_join_output(left, right, out, nout, left_key, right_key);
}

/* One full gather of the table through the ascending row list of
 * select_rows; `valid` keeps the schema, mask presence included, and
 * `null_rows` is in the form the rank appends to its result: the table's
 * columns and, with pad_with, behind them that table's columns as all-null
 * cells, as a LEFT join pads an unmatched row. */
StrippedTable strip_null_keys(cudf::table_view t, std::vector<cudf::size_type> const& on,
                              bool keep_null_rows, const cudf::table_view* pad_with)
{
  hipStream_t st = dj_rt_stream();
  StrippedTable out;
  const int64_t n = t.num_rows();
  KeyRowValidity v = key_row_validity(t, on, st);
  if (v.nnull == 0) return out;
  DBuf scratch(dj::select_rows_scratch_bytes(n)), count(8);
  auto take = [&](bool want_set, int64_t expect, const cudf::table_view* pad) {
    std::vector<std::unique_ptr<cudf::column>> cols;
    if (expect == 0) {
      append_empty_columns(t, false, cols);
      if (pad) append_empty_columns(*pad, true, cols);
      return std::make_unique<cudf::table>(std::move(cols));
    }
    DBuf sel((size_t)expect * 8);
    dj::select_rows(v.bits, n, want_set, sel.i64(), count.i64(), st, scratch.p);
    gather_table_columns(t, sel, expect, -1, nullptr, cols, st);
    if (pad) {
      DBuf none;
      gather_table_columns(*pad, none, 0, -1, nullptr, cols, st, expect);
    }
    DJ_HIP_CALL(hipStreamSynchronize(st));
    return std::make_unique<cudf::table>(std::move(cols));
  };
  out.valid = take(true, n - v.nnull, nullptr);
  if (keep_null_rows) out.null_rows = take(false, v.nnull, pad_with);
  return out;
}

}  // namespace dj_host
