/*
 * dj_table_ops.hip — what the join and shuffle routes do to whole tables:
 * key and type predicates, the engine's int64 view of key columns (widened
 * or fused), the output gather, the stable hash partition, row placement
 * and concatenation (dj_host.hpp).
 */
#include "dj_host.hpp"

#include <stdexcept>

namespace dj_host {

bool is_string(cudf::column_view col) { return col.type().id() == cudf::type_id::STRING; }

/* FLOAT32/FLOAT64 keys refuse loudly (cuDF normalises -0.0/NaN before hashing
 * float keys; that is not implemented — INTEGRATION.md "Known restrictions") */
int key_kind(cudf::data_type t)
{
  DJ_CHECK_ERROR(!cudf::is_floating(t),
                 "FLOAT32/FLOAT64 columns cannot be join/shuffle keys (payload only)");
  DJ_CHECK_ERROR(cudf::is_integer_rep(t),
                 "join/shuffle key columns must be integer-rep or STRING columns");
  const bool u = cudf::is_unsigned_rep(t);
  switch (cudf::size_of(t)) {
    case 8: return dj::kKeyI64;
    case 4: return u ? dj::kKeyU32 : dj::kKeyI32;
    case 2: return u ? dj::kKeyU16 : dj::kKeyI16;
    default: return u ? dj::kKeyU8 : dj::kKeyI8;
  }
}

static bool is_new_type(cudf::data_type t) { return (int)t.id() >= (int)cudf::type_id::INT16; }

/* a key pair may mix the long-standing reps (INT32 with INT64, chrono with
 * its integer rep); a pair involving INT16, an unsigned type or BOOL8 must match exactly */
void check_key_pairs(cudf::table_view left, cudf::table_view right,
                     std::vector<cudf::size_type> const& lon,
                     std::vector<cudf::size_type> const& ron)
{
  for (size_t c = 0; c < lon.size() && c < ron.size(); c++) {
    const cudf::data_type lt = left.column(lon[c]).type(), rt = right.column(ron[c]).type();
    if (lt.id() != cudf::type_id::STRING) (void)key_kind(lt);
    if (rt.id() != cudf::type_id::STRING) (void)key_kind(rt);
    DJ_CHECK_ERROR(lt == rt || (!is_new_type(lt) && !is_new_type(rt)),
                   "join key pair: INT16/UINT8/UINT16/UINT32/UINT64/BOOL8 key columns must "
                   "have the same type on both sides");
  }
}

bool any_nullable(cudf::table_view t)
{
  for (cudf::size_type c = 0; c < t.num_columns(); c++)
    if (t.column(c).nullable()) return true;
  return false;
}

bool any_nullable_key(cudf::table_view t, std::vector<cudf::size_type> const& on)
{
  for (auto c : on)
    if (t.column(c).nullable()) return true;
  return false;
}

/* columns 0..31: callers refuse a wider table that has any mask, see the
 * AllToAllCommunicator constructor */
uint32_t nullable_bits(cudf::table_view t)
{
  uint32_t bits = 0;
  for (cudf::size_type c = 0; c < t.num_columns() && c < 32; c++)
    if (t.column(c).nullable()) bits |= 1u << c;
  return bits;
}

void check_no_masks(cudf::table_view t, const char* what)
{
  if (any_nullable(t))
    throw std::runtime_error(std::string(what) +
                             ": nullable columns (validity masks) are not supported here; "
                             "use shuffle_on / distributed_inner_join / AllToAllCommunicator");
}

bool any_string_key(cudf::table_view t, std::vector<cudf::size_type> const& on)
{
  for (auto c : on)
    if (is_string(t.column(c))) return true;
  return false;
}

/* A STRING column enters the chain as its dj_string_key64 row hash
 * (dj_strhash.h), computed into a temporary 64-bit column. The single-key
 * engine then partitions/joins on the fused value as if it were the key, and
 * the caller filters hash-collision false positives against the real columns
 * afterwards (local_join). DJ_TEST_WEAK_FUSE collapses the value to 4 bits so
 * tests can exercise that filter deterministically. */
DBuf fuse_keys(cudf::table_view t, std::vector<cudf::size_type> const& on, hipStream_t st)
{
  const int64_t n = t.num_rows();
  DJ_CHECK_ERROR(on.size() >= 1 && on.size() <= 4,
                 "multi-column join keys: 1..4 key columns supported");
  const int64_t* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  const uint32_t* masks[4] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t kinds = 0;
  std::vector<DBuf> str_keys;
  for (size_t c = 0; c < on.size(); c++) {
    cudf::column_view col = t.column(on[c]);
    masks[c] = col.null_mask();
    if (is_string(col)) {
      /* rows are hashed whatever their validity; the kernel below replaces
       * the hash of a null row by the null constant */
      str_keys.emplace_back((size_t)(n > 0 ? n : 1) * 8);
      dj::hash_strings(col.head<int32_t>(), (const uint8_t*)col.chars(), n,
                       (uint64_t*)str_keys.back().p, st);
      ptrs[c] = str_keys.back().i64();
      kinds |= (uint32_t)dj::kKeyI64 << (4 * c);
      continue;
    }
    ptrs[c] = col.head<int64_t>();
    kinds |= (uint32_t)key_kind(col.type()) << (4 * c);
  }
  static const int weak = getenv("DJ_TEST_WEAK_FUSE") ? 1 : 0;
  DBuf out((size_t)(n > 0 ? n : 1) * 8);
  if (n > 0) {
    dj::fuse_key_columns(ptrs, masks, kinds, (int)on.size(), n, weak, out.i64(), st);
    DJ_HIP_CALL(hipGetLastError());
    /* the row-hash temporaries go back to the pool on return */
    if (!str_keys.empty()) DJ_HIP_CALL(hipStreamSynchronize(st));
  }
  return out;
}

const int64_t* key_as_i64(cudf::column_view col, int64_t* dst, hipStream_t st)
{
  const int kind = key_kind(col.type());
  if (kind == dj::kKeyI64) return col.head<int64_t>();
  dj::widen_key(col.head<void>(), kind, (int64_t)col.size(), dst, st);
  return dst;
}

const int64_t* key_as_i64(cudf::column_view col, DBuf& tmp)
{
  if (key_kind(col.type()) != dj::kKeyI64) tmp = DBuf((size_t)col.size() * 8);
  return key_as_i64(col, tmp.i64(), dj_rt_stream());
}

cudf::table_view view_i64_pair(const void* c0, const void* c1, int64_t n)
{
  const cudf::data_type i64(cudf::type_id::INT64);
  return cudf::table_view({cudf::column_view(i64, (cudf::size_type)n, c0),
                           cudf::column_view(i64, (cudf::size_type)n, c1)});
}

/* the hot shape: exactly two INT64 columns, one of them the key, and no
 * validity mask (a table with any mask takes the general paths) */
static bool is_i64_pair(cudf::table_view t, cudf::size_type key_col)
{
  return t.num_columns() == 2 && (key_col == 0 || key_col == 1) &&
         t.column(0).type().id() == cudf::type_id::INT64 &&
         t.column(1).type().id() == cudf::type_id::INT64 && !t.column(0).nullable() &&
         !t.column(1).nullable();
}

/* the engine's four outputs then ARE the result columns (payloads travel
 * through the join) */
bool joins_i64_pairs(cudf::table_view left, cudf::table_view right, cudf::size_type left_key,
                     cudf::size_type right_key)
{
  return left_key == 0 && right_key == 0 && is_i64_pair(left, 0) && is_i64_pair(right, 0);
}

/* gather a STRING column by a row-index permutation: sizes gather -> scan ->
 * chars gather (the reference's thrust::gather + scan strings recipe,
 * strings_column.cu:39-131, as one reusable step). null_tail > 0 appends
 * that many empty rows behind the n gathered ones (the null right-hand cells
 * of a left join): their offsets all equal the chars total. */
static std::unique_ptr<cudf::column> gather_string_column(cudf::column_view src,
                                                          const int64_t* d_idx, int64_t n,
                                                          int64_t null_tail = 0)
{
  hipStream_t st = dj_rt_stream();
  DBuf sizes((size_t)(n > 0 ? n : 1) * 4);
  DBuf starts((size_t)(n > 0 ? n : 1) * 4);
  dj::gather_sizes_starts(src.head<int32_t>(), d_idx, n, (int32_t*)sizes.p,
                          (int32_t*)starts.p, st);
  DBuf off(((size_t)n + 1) * 4);
  DBuf scan_scratch(dj::offsets_from_sizes_scratch_bytes(n));
  DBuf total64(8);
  DJ_HIP_CALL(hipMemsetAsync(total64.p, 0, 8, st));
  dj::offsets_from_sizes((const int32_t*)sizes.p, n, (int32_t*)off.p, scan_scratch.p, st);
  dj::sum_sizes_i64((const int32_t*)sizes.p, n, total64.i64(), st);
  int32_t total = 0;
  int64_t tot64 = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&total, (int32_t*)off.p + n, 4, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipMemcpyAsync(&tot64, total64.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  /* int32 offsets are the cudf convention this boundary keeps (the
   * reference's cuDF 0.19 has the same 2^31 chars-per-column cap) —
   * overflow must refuse loudly, not scribble (a gathered join output
   * easily exceeds it: 600 M rows x ~7.6 B chars did) */
  DJ_CHECK_ERROR(tot64 <= INT32_MAX,
                 "string gather: output chars exceed 2^31 (int32 offsets limit; shrink "
                 "the per-batch output with over_decom or more ranks)");
  auto col = std::make_unique<cudf::column>((cudf::size_type)(n + null_tail), (int64_t)total);
  DJ_HIP_CALL(hipMemcpyAsync(col->head(), off.p, ((size_t)n + 1) * 4,
                             hipMemcpyDeviceToDevice, st));
  if (null_tail > 0) dj::fill_i32((int32_t*)col->head() + n + 1, null_tail, total, st);
  dj::gather_chars_from_starts((const uint8_t*)src.chars(), (const int32_t*)starts.p, n,
                               (const int32_t*)col->head(), (uint8_t*)col->chars(), st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return col;
}

/* All fixed-width columns go through ONE dj::gather_table call (the
 * width-generic kernel, dj_kernels.hip "table gather"); STRING columns keep
 * gather_string_column. The key column (key_col >= 0) is not gathered: its
 * joined values already sit in key_vals as int64 (each random-line gather of
 * 240 M rows costs ~5 ms; adopting the key buffer is free, narrowing to the
 * key's own width is a streaming copy).
 *
 * null_tail >= 0 builds the right-hand side of a left join: every column has
 * n + null_tail rows, the tail rows are null cells (zero bytes, empty
 * strings), and EVERY column carries a mask, whether its source had one or
 * not and also when null_tail is 0. The default, -1, is the plain gather. */
void gather_table_columns(cudf::table_view src, DBuf& idx, int64_t n, cudf::size_type key_col,
                          DBuf* key_vals, std::vector<std::unique_ptr<cudf::column>>& cols,
                          hipStream_t st, int64_t null_tail)
{
  const int64_t* d_idx = idx.i64();
  const bool pad = null_tail >= 0;
  const int64_t tail = pad ? null_tail : 0;
  DJ_CHECK_ERROR(!pad || key_vals == nullptr, "gather: a null-padded side adopts no key buffer");
  std::vector<dj::GatherCol> gc;
  const int64_t* key_src = nullptr;
  void* key_dst = nullptr;
  int key_width = 0;
  const size_t first = cols.size();
  for (cudf::size_type c = 0; c < src.num_columns(); c++) {
    cudf::column_view v = src.column(c);
    if (v.type().id() == cudf::type_id::STRING) {
      cols.push_back(gather_string_column(v, d_idx, n, tail));
      continue;
    }
    const int width = cudf::size_of(v.type());
    DJ_CHECK_ERROR(width > 0, "gather: unsupported column type");
    if (c == key_col && key_vals != nullptr) {
      if (width == 8) {
        cols.push_back(std::make_unique<cudf::column>(v.type(), (cudf::size_type)n, key_vals->p));
        key_vals->p = nullptr;
        continue;
      }
      auto col = std::make_unique<cudf::column>(v.type(), (cudf::size_type)n);
      key_src = key_vals->i64();
      key_dst = col->head();
      key_width = width;
      cols.push_back(std::move(col));
      continue;
    }
    auto col = std::make_unique<cudf::column>(v.type(), (cudf::size_type)(n + tail));
    gc.push_back(dj::GatherCol{v.head<void>(), col->head(), width});
    if (tail > 0)
      DJ_HIP_CALL(hipMemsetAsync((uint8_t*)col->head() + (size_t)n * width, 0,
                                 (size_t)tail * width, st));
    cols.push_back(std::move(col));
  }
  dj_timing::Scope t(DJ_PHASE_GATHER, st);
  if (key_dst != nullptr && n > 0) dj::narrow_key(key_src, n, key_width, key_dst, st);
  dj::gather_table(gc.data(), (int)gc.size(), d_idx, n, dj::kGatherAuto, st);

  /* validity: every nullable source column gets an output mask through
   * dj::gather_bitmasks over the same index array (launches of their own,
   * one per column, after the value gather — DESIGN.md §3d), key and STRING
   * columns included; a mask-free table stops here. A null-padded side
   * masks every column: a null source mask gathers as all valid, and the
   * tail bits stay 0 from the memset below (gather_bitmasks writes bits
   * [0, roundup(n, 64)) only, the ones at and past n as 0). */
  if (!pad && !any_nullable(src)) return;
  std::vector<cudf::column*> masked;
  std::vector<const uint32_t*> msrc;
  for (cudf::size_type c = 0; c < src.num_columns(); c++) {
    if (!pad && !src.column(c).nullable()) continue;
    masked.push_back(cols[first + (size_t)c].get());
    msrc.push_back(src.column(c).null_mask());
  }
  /* any number of nullable columns: descriptors of at most kMaxSchemaCols,
   * as gather_table takes its columns */
  const size_t nm = masked.size();
  DBuf d_counts(nm * 4);
  DJ_HIP_CALL(hipMemsetAsync(d_counts.p, 0, nm * 4, st));
  for (size_t k0 = 0; k0 < nm; k0 += dj::kMaxSchemaCols) {
    dj::BitmaskGatherDesc bd{};
    bd.ncols = (int)std::min<size_t>(nm - k0, dj::kMaxSchemaCols);
    for (int k = 0; k < bd.ncols; k++) {
      bd.src[k] = msrc[k0 + (size_t)k];
      bd.dst[k] = masked[k0 + (size_t)k]->allocate_null_mask();
      if (pad)
        DJ_HIP_CALL(hipMemsetAsync(
          bd.dst[k], 0,
          std::max<size_t>(cudf::bitmask_allocation_size_bytes((cudf::size_type)(n + tail)), 64),
          st));
    }
    dj::gather_bitmasks(bd, d_idx, n, (uint32_t*)d_counts.p + k0, st);
  }
  std::vector<uint32_t> h_counts(nm);
  DJ_HIP_CALL(hipMemcpyAsync(h_counts.data(), d_counts.p, nm * 4, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  for (size_t k = 0; k < nm; k++)
    masked[k]->set_null_count((cudf::size_type)(h_counts[k] + (uint32_t)tail));
}

/* permutation computed on (key, iota) with the stable wave-ballot kernel,
 * then one gather per column. 2-column all-INT64 tables skip the gathers
 * (keys+payload move directly through the partition scatter). */
PartitionedTable partition_table(cudf::table_view in, cudf::size_type key_col, int nparts,
                                 int hash_fn, uint32_t seed, const int64_t* ext_keys)
{
  hipStream_t st = dj_rt_stream();
  const int64_t n = in.num_rows();
  DBuf key_tmp;
  const int64_t* keys = ext_keys ? ext_keys : key_as_i64(in.column(key_col), key_tmp);
  DBuf scratch(dj::hash_partition_scratch_bytes(n, nparts));
  DBuf d_off((size_t)(nparts + 1) * 8);

  const bool fast2 = ext_keys == nullptr && is_i64_pair(in, key_col);

  std::vector<std::unique_ptr<cudf::column>> cols;
  if (fast2)
    for (cudf::size_type c = 0; c < 2; c++)
      cols.push_back(std::make_unique<cudf::column>(in.column(c).type(), (cudf::size_type)n));

  {
    dj_timing::Scope t1(DJ_PHASE_PART_COUNT, st);
    dj::partition_count(keys, n, nparts, hash_fn, seed, scratch.p, st);
  }
  {
    dj_timing::Scope t2(DJ_PHASE_PART_SCAN, st);
    dj::partition_scan(n, nparts, scratch.p, d_off.i64(), st);
  }
  if (fast2) {
    const cudf::size_type pay_col = key_col == 0 ? 1 : 0;
    dj_timing::Scope t3(DJ_PHASE_PART_SCATTER, st);
    dj::partition_scatter(keys, in.column(pay_col).head<int64_t>(), n, nparts, hash_fn, seed,
                          d_off.i64(), scratch.p,
                          (int64_t*)cols[key_col]->head(), (int64_t*)cols[pay_col]->head(), st);
  } else {
    DBuf iota((size_t)n * 8), perm((size_t)n * 8), keys_out((size_t)n * 8);
    dj::iota_i64(iota.i64(), n, st);
    {
      dj_timing::Scope t3(DJ_PHASE_PART_SCATTER, st);
      dj::partition_scatter(keys, iota.i64(), n, nparts, hash_fn, seed, d_off.i64(), scratch.p,
                            keys_out.i64(), perm.i64(), st);
    }
    gather_table_columns(in, perm, n, -1, nullptr, cols, st);
  }
  auto out = std::make_unique<cudf::table>(std::move(cols));
  std::vector<int64_t> off_host(nparts + 1);
  DJ_HIP_CALL(hipMemcpyAsync(off_host.data(), d_off.p, (size_t)(nparts + 1) * 8,
                             hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  PartitionedTable r;
  r.tbl = std::move(out);
  r.offsets.assign(off_host.begin(), off_host.end());
  return r;
}

/* the rows of `input` grouped into nparts contiguous ranges by the hash of
 * their key. Multi-column keys, and any STRING key, place on the fused key
 * chain (our spec, dj_hash.h — MurmurHash3 placement is parity-unpinned,
 * SURVEY.md §8c) */
PartitionedTable place_rows(cudf::table_view input, std::vector<cudf::size_type> const& on,
                            int nparts, int hash_fn, uint32_t seed)
{
  DBuf fused;
  const bool str_key = any_string_key(input, on);
  if (on.size() > 1 || str_key) {
    DJ_CHECK_ERROR(hash_fn != DJ_HASH_IDENTITY || !str_key,
                   "identity-hash shuffle is not defined for STRING key columns "
                   "(cuDF has no identity hash for strings either); use HASH_MURMUR3");
    DJ_CHECK_ERROR(hash_fn != DJ_HASH_IDENTITY,
                   "identity-hash shuffle requires a single key column");
    fused = fuse_keys(input, on, dj_rt_stream());
  } else if (input.column(on[0]).nullable()) {
    /* a single nullable integer key: valid rows place exactly as without the
     * mask, null rows on the null element hash (dj_hash.h). The per-row hash
     * is computed here and the partition runs on it with the identity hash
     * (hash % nparts either way), leaving the partition kernels untouched. */
    const int64_t n = input.num_rows();
    cudf::column_view col = input.column(on[0]);
    fused = DBuf((size_t)(n > 0 ? n : 1) * 8);
    if (n > 0)
      dj::nullable_key_hash(col.head<void>(), key_kind(col.type()), col.null_mask(), n, hash_fn,
                            seed, fused.i64(), dj_rt_stream());
    return partition_table(input, on[0], nparts, DJ_HASH_IDENTITY, 0, fused.i64());
  }
  return partition_table(input, on[0], nparts, hash_fn, seed, fused.p ? fused.i64() : nullptr);
}

std::unique_ptr<cudf::table> concat_tables(std::vector<std::unique_ptr<cudf::table>>& parts)
{
  if (parts.size() == 1) return std::move(parts[0]);
  hipStream_t st = dj_rt_stream();
  dj_timing::Scope t(DJ_PHASE_CONCAT, st);
  int64_t total = 0;
  for (auto& p : parts) total += p->num_rows();
  std::vector<std::unique_ptr<cudf::column>> cols;
  /* validity: the parts' masks back to back (a part without one counts as
   * all valid); the segment tables live until the sync below */
  std::vector<DBuf> seg_tables;
  auto concat_masks = [&](cudf::size_type c, cudf::column& col) {
    bool any = false;
    for (auto& p : parts) any |= p->get_column(c).nullable();
    if (!any) return;
    std::vector<BitSeg> segs;
    int64_t nulls = 0;
    for (auto& p : parts) {
      segs.push_back(BitSeg{p->get_column(c).null_mask(), 0, p->num_rows()});
      nulls += p->get_column(c).null_count();
    }
    seg_tables.push_back(copy_bit_segments(segs, col.allocate_null_mask(), st));
    col.set_null_count((cudf::size_type)nulls);
  };
  for (cudf::size_type c = 0; c < parts[0]->num_columns(); c++) {
    auto type = parts[0]->get_column(c).type();
    if (type.id() == cudf::type_id::STRING) {
      int64_t total_chars = 0;
      for (auto& p : parts) total_chars += p->get_column(c).chars_size();
      auto col = std::make_unique<cudf::column>((cudf::size_type)total, total_chars);
      int64_t row_off = 0, char_off = 0;
      for (auto& p : parts) {
        int64_t nrows = p->num_rows();
        int64_t nchars = p->get_column(c).chars_size();
        if (nrows > 0)
          dj::rebase_offsets((const int32_t*)p->get_column(c).head(), nrows + 1,
                             (int32_t)char_off, (int32_t*)col->head() + row_off, st);
        if (nchars > 0)
          DJ_HIP_CALL(hipMemcpyAsync((uint8_t*)col->chars() + char_off,
                                     p->get_column(c).chars(), (size_t)nchars,
                                     hipMemcpyDeviceToDevice, st));
        row_off += nrows;
        char_off += nchars;
      }
      concat_masks(c, *col);
      cols.push_back(std::move(col));
      continue;
    }
    auto col = std::make_unique<cudf::column>(type, (cudf::size_type)total);
    int64_t off = 0;
    for (auto& p : parts) {
      int64_t nrows = p->num_rows();
      if (nrows > 0)
        DJ_HIP_CALL(hipMemcpyAsync((int8_t*)col->head() + off * cudf::size_of(type),
                                   p->get_column(c).head(),
                                   (size_t)nrows * cudf::size_of(type),
                                   hipMemcpyDeviceToDevice, st));
      off += nrows;
    }
    concat_masks(c, *col);
    cols.push_back(std::move(col));
  }
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return std::make_unique<cudf::table>(std::move(cols));
}

}  // namespace dj_host
