/*
 * dj_cpp_cabi.hip — the C ABI over the C++ orchestration (for the Python
 * measurement harness; additive — SURVEY.md §8b): communicators, the join
 * and shuffle entry points over raw arrays and column descriptors, table
 * accessors, and the test/bench hooks (include/distributed_join.h).
 * dj_rccl_selftest sits with the communicators in dj_comm.hip.
 */
#include "dj_host.hpp"

#include <stdexcept>

using namespace dj_host;

namespace {

/* dj_ncol_desc[nc] (include/distributed_join.h) -> table view of n rows,
 * masks attached */
cudf::table_view view_from_descs(const dj_ncol_desc* cols, int nc, int64_t n)
{
  using cudf::data_type;
  using cudf::type_id;
  std::vector<cudf::column_view> v;
  for (int c = 0; c < nc; c++) {
    const auto* mask = (const cudf::bitmask_type*)cols[c].null_mask;
    const cudf::size_type nulls = mask ? (cudf::size_type)cols[c].null_count : 0;
    if ((type_id)cols[c].type_id == type_id::STRING)
      v.emplace_back(data_type(type_id::STRING), (cudf::size_type)n, cols[c].data,
                     cols[c].chars, cols[c].chars_bytes, mask, nulls);
    else
      v.emplace_back(data_type((type_id)cols[c].type_id), (cudf::size_type)n, cols[c].data,
                     mask, nulls);
  }
  return cudf::table_view(v);
}

/* a dj_col_desc is a dj_ncol_desc without a mask */
cudf::table_view view_from_descs(const dj_col_desc* cols, int nc, int64_t n)
{
  std::vector<dj_ncol_desc> masked((size_t)nc);
  for (int c = 0; c < nc; c++)
    masked[(size_t)c] = dj_ncol_desc{cols[c].type_id, cols[c].data, cols[c].chars,
                                     cols[c].chars_bytes, nullptr, 0};
  return view_from_descs(masked.data(), nc, n);
}

/* DJ_HASH_* of the C header -> cudf::hash_id */
cudf::hash_id to_hash_id(int hash_function)
{
  return hash_function == DJ_HASH_IDENTITY ? cudf::hash_id::HASH_IDENTITY
                                           : cudf::hash_id::HASH_MURMUR3;
}

/* the bodies of the entry points that come in a _cols and an _ncols form */

void* inner_join_views(void* comm, cudf::table_view left, cudf::table_view right,
                       const int32_t* lon, const int32_t* ron, int nkeys, int over_decom,
                       int report_timing)
{
  std::vector<cudf::size_type> lo(lon, lon + nkeys), ro(ron, ron + nkeys);
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  auto result = distributed_inner_join(left, right, lo, ro, (Communicator*)comm, lopts,
                                       ropts, over_decom, report_timing != 0, nullptr, 1);
  return result.release();
}

/* compression: 0 = none, 1 = the fixed bitpack policy
 * (generate_compression_options_distributed), 2 = sampling auto-select
 * (generate_auto_select_compression_options), 3 = an explicit bitpack
 * cascaded option on EVERY column, whatever its type (reaches the option
 * validation: a loud error on FLOAT32/FLOAT64/BOOL8 columns). */
void* shuffle_on_view(void* comm, cudf::table_view input, const int32_t* on, int nkeys,
                      int hash_function, uint32_t seed, int compression)
{
  std::vector<cudf::size_type> keys(on, on + nkeys);
  std::vector<ColumnCompressionOptions> opts;
  if (compression == 2) {
    opts = generate_auto_select_compression_options(input);
  } else if (compression == 3) {
    nvcompCascadedFormatOpts bp{};
    bp.use_bp = 1;
    opts.assign((size_t)input.num_columns(),
                ColumnCompressionOptions(CompressionMethod::cascaded, bp));
  } else {
    opts = generate_compression_options_distributed(input, compression != 0);
  }
  try {
    auto result = shuffle_on(input, keys, (Communicator*)comm, opts, to_hash_id(hash_function),
                             seed, false, nullptr);
    return result.release();
  } catch (std::exception const& e) {
    /* no exception crosses the C ABI: loud exit, as DJ_CHECK_ERROR */
    fprintf(stderr, "ERROR: %s\n", e.what());
    exit(1);
  }
}

void* partition_view(cudf::table_view input, const int32_t* on, int nkeys, int nparts,
                     int hash_function, uint32_t seed, int64_t* h_offsets)
{
  DJ_CHECK_ERROR(nkeys >= 1 && nkeys <= 4, "partition: 1..4 key columns");
  DJ_CHECK_ERROR(nparts >= 1 && nparts <= dj::kMaxPartitions, "partition: 1..1024 parts");
  std::vector<cudf::size_type> keys(on, on + nkeys);
  PartitionedTable part =
    place_rows(input, keys, nparts,
               hash_function == DJ_HASH_IDENTITY ? DJ_HASH_IDENTITY : DJ_HASH_MURMUR3, seed);
  for (int i = 0; i <= nparts; i++) h_offsets[i] = part.offsets[(size_t)i];
  return part.tbl.release();
}

/* the timing loop of the kernel hooks: `launch` runs max(reps, 1) times on
 * `st`, each between a hipEvent pair; h_ms (host double[reps], may be NULL)
 * receives the milliseconds. Host-synchronous. */
template <class Launch>
void time_reps(int reps, double* h_ms, hipStream_t st, Launch launch)
{
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipEventRecord(e0, st));
    launch();
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
}

}  // namespace

extern "C" {

void* dj_cpp_comm_create(int rank, int size, const void* id_bytes)
{
  if (size <= 1) {
    auto* c = new LocalCommunicator();
    g_default_comm = c;
    return c;
  }
  return new RCCLCommunicator(rank, size, id_bytes);
}

void dj_cpp_comm_destroy(void* comm)
{
  auto* c = (Communicator*)comm;
  c->finalize();
  if (g_default_comm == c) g_default_comm = nullptr;
  delete c;
}

/* full distributed_inner_join over int64 key/payload columns; returns an
 * opaque cudf::table*. Cascaded bitpack on the wire when compression != 0;
 * nvlink_domain_size as in the C++ API. The reference's README
 * benchmark runs with its default nvlink_domain_size=1 (IB-domain shuffle of
 * both tables + local join, distributed_join.cpp:152-199 + README.md:73-86);
 * on one 8x MI355X node the whole node is ONE xGMI domain, so
 * nvlink_domain_size = world engages the batched all-to-all pipeline (fused
 * wire path + comm/compute overlap) — the MI355X-correct configuration. */
void* dj_cpp_distributed_inner_join_i64_full(void* comm, const int64_t* d_lk,
                                             const int64_t* d_lp, int64_t ln,
                                             const int64_t* d_rk, const int64_t* d_rp,
                                             int64_t rn, int over_decom, int report_timing,
                                             int compression, int nvlink_domain_size)
{
  cudf::table_view left = view_i64_pair(d_lk, d_lp, ln), right = view_i64_pair(d_rk, d_rp, rn);
  auto opts = generate_compression_options_distributed(left, compression != 0);
  auto result = distributed_inner_join(left, right, {0}, {0}, (Communicator*)comm, opts, opts,
                                       over_decom, report_timing != 0, nullptr,
                                       nvlink_domain_size);
  return result.release();
}

/* the same without compression, nvlink_domain_size = 1 */
void* dj_cpp_distributed_inner_join_i64(void* comm, const int64_t* d_lk, const int64_t* d_lp,
                                        int64_t ln, const int64_t* d_rk, const int64_t* d_rp,
                                        int64_t rn, int over_decom, int report_timing)
{
  return dj_cpp_distributed_inner_join_i64_full(comm, d_lk, d_lp, ln, d_rk, d_rp, rn,
                                                over_decom, report_timing, 0, 1);
}

/* the same with nvlink_domain_size = 1 */
void* dj_cpp_distributed_inner_join_i64_opts(void* comm, const int64_t* d_lk,
                                             const int64_t* d_lp, int64_t ln,
                                             const int64_t* d_rk, const int64_t* d_rp,
                                             int64_t rn, int over_decom, int report_timing,
                                             int compression)
{
  return dj_cpp_distributed_inner_join_i64_full(comm, d_lk, d_lp, ln, d_rk, d_rp, rn,
                                                over_decom, report_timing, compression, 1);
}

void* dj_cpp_shuffle_on_i64_comp(void* comm, const int64_t* d_keys, const int64_t* d_pay,
                                 int64_t n, int hash_function, uint32_t seed, int compression)
{
  cudf::table_view input = view_i64_pair(d_keys, d_pay, n);
  auto opts = generate_compression_options_distributed(input, compression != 0);
  auto result = shuffle_on(input, {0}, (Communicator*)comm, opts, to_hash_id(hash_function),
                           seed, false, nullptr);
  return result.release();
}

void* dj_cpp_shuffle_on_i64(void* comm, const int64_t* d_keys, const int64_t* d_pay, int64_t n,
                            int hash_function, uint32_t seed)
{
  return dj_cpp_shuffle_on_i64_comp(comm, d_keys, d_pay, n, hash_function, seed, 0);
}

/* deterministic test/bench string payload from keys (string_payload.cu
 * pattern): returns offsets (int32[n+1]) and chars device buffers via out
 * params; caller frees with dj_dfree */
void dj_gen_test_strings(const int64_t* d_keys, int64_t n, void** out_offsets,
                         void** out_chars, int64_t* out_chars_bytes)
{
  hipStream_t st = dj_rt_stream();
  DBuf sizes((size_t)(n > 0 ? n : 1) * 4);
  dj::make_test_string_sizes(d_keys, n, (int32_t*)sizes.p, st);
  int32_t* offsets = (int32_t*)dj_dmalloc((n + 1) * 4);
  DBuf scr(dj::offsets_from_sizes_scratch_bytes(n));
  dj::offsets_from_sizes((const int32_t*)sizes.p, n, offsets, scr.p, st);
  const int32_t total = read_back<int32_t>(offsets + n, st);
  uint8_t* chars = (uint8_t*)dj_dmalloc(total > 0 ? total : 1);
  dj::fill_test_strings(d_keys, n, offsets, chars, st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  *out_offsets = offsets;
  *out_chars = chars;
  *out_chars_bytes = total;
}

/* distributed join with int64 keys and STRING payloads (BASELINE config 4) */
void* dj_cpp_distributed_inner_join_i64str(void* comm, const int64_t* d_lk,
                                           const void* l_offsets, const void* l_chars,
                                           int64_t l_chars_bytes, int64_t ln,
                                           const int64_t* d_rk, const void* r_offsets,
                                           const void* r_chars, int64_t r_chars_bytes,
                                           int64_t rn, int over_decom, int report_timing)
{
  const int i64 = (int)cudf::type_id::INT64, str = (int)cudf::type_id::STRING;
  const dj_col_desc lcols[2] = {{i64, d_lk, nullptr, 0}, {str, l_offsets, l_chars, l_chars_bytes}};
  const dj_col_desc rcols[2] = {{i64, d_rk, nullptr, 0}, {str, r_offsets, r_chars, r_chars_bytes}};
  const int32_t key = 0;
  return inner_join_views(comm, view_from_descs(lcols, 2, ln), view_from_descs(rcols, 2, rn),
                          &key, &key, 1, over_decom, report_timing);
}

/* generic column-descriptor join (e.g. the TPC-H lineitem x orders shape:
 * int64 key + string payload on one side, int64 key + int64 payload on the
 * other). dj_col_desc: include/distributed_join.h; type_id: 2=INT32,
 * 3=INT64, 4=STRING (cudf::type_id values). Key indices may name STRING
 * columns. lon/ron are int32 arrays of nkeys column indices
 * (distributed_inner_join with composite left_on/right_on). */
void* dj_cpp_distributed_inner_join_cols_multi(void* comm, const dj_col_desc* lcols, int nl,
                                               int64_t ln, const dj_col_desc* rcols, int nr,
                                               int64_t rn, const int32_t* lon,
                                               const int32_t* ron, int nkeys, int over_decom,
                                               int report_timing)
{
  return inner_join_views(comm, view_from_descs(lcols, nl, ln), view_from_descs(rcols, nr, rn),
                          lon, ron, nkeys, over_decom, report_timing);
}

/* single-key variant */
void* dj_cpp_distributed_inner_join_cols(void* comm, const dj_col_desc* lcols, int nl,
                                         int64_t ln, const dj_col_desc* rcols, int nr,
                                         int64_t rn, int key_l, int key_r, int over_decom,
                                         int report_timing)
{
  const int32_t lon = key_l, ron = key_r;
  return dj_cpp_distributed_inner_join_cols_multi(comm, lcols, nl, ln, rcols, nr, rn, &lon,
                                                  &ron, 1, over_decom, report_timing);
}

/* shuffle_on over column descriptors; `on` names nkeys key columns, STRING
 * ones included (placement on the fused key chain, dj_hash.h). compression:
 * see shuffle_on_view. */
void* dj_cpp_shuffle_on_cols(void* comm, const dj_col_desc* cols, int nc, int64_t n,
                             const int32_t* on, int nkeys, int hash_function, uint32_t seed,
                             int compression)
{
  return shuffle_on_view(comm, view_from_descs(cols, nc, n), on, nkeys, hash_function, seed,
                         compression);
}

/* test hook: the placement step of shuffle_on alone (place_rows, the very
 * function shuffle_on calls before its all-to-all). Partitions the table
 * into nparts contiguous ranges and writes the nparts+1 row offsets to
 * h_offsets. Lets one GPU check placement against the dj_hash.h spec for
 * nparts > 1. */
void* dj_cpp_partition_cols(const dj_col_desc* cols, int nc, int64_t n, const int32_t* on,
                            int nkeys, int nparts, int hash_function, uint32_t seed,
                            int64_t* h_offsets)
{
  return partition_view(view_from_descs(cols, nc, n), on, nkeys, nparts, hash_function, seed,
                        h_offsets);
}

/* the nullable-descriptor forms of the three entry points above */
void* dj_cpp_distributed_inner_join_ncols_multi(void* comm, const dj_ncol_desc* lcols, int nl,
                                                int64_t ln, const dj_ncol_desc* rcols, int nr,
                                                int64_t rn, const int32_t* lon,
                                                const int32_t* ron, int nkeys, int over_decom,
                                                int report_timing)
{
  return inner_join_views(comm, view_from_descs(lcols, nl, ln), view_from_descs(rcols, nr, rn),
                          lon, ron, nkeys, over_decom, report_timing);
}

void* dj_cpp_shuffle_on_ncols(void* comm, const dj_ncol_desc* cols, int nc, int64_t n,
                              const int32_t* on, int nkeys, int hash_function, uint32_t seed,
                              int compression)
{
  return shuffle_on_view(comm, view_from_descs(cols, nc, n), on, nkeys, hash_function, seed,
                         compression);
}

void* dj_cpp_partition_ncols(const dj_ncol_desc* cols, int nc, int64_t n, const int32_t* on,
                             int nkeys, int nparts, int hash_function, uint32_t seed,
                             int64_t* h_offsets)
{
  return partition_view(view_from_descs(cols, nc, n), on, nkeys, nparts, hash_function, seed,
                        h_offsets);
}

/* test hook: concat_tables, the step that joins the batches of the batched
 * pipeline into one result (a STRING column's offsets are rebased part by
 * part, masks concatenate bit-exactly). A single-rank join never has more
 * than one part, so only this hook reaches the step without a second rank.
 * Takes ownership of the n >= 1 input tables. */
void* dj_cpp_concat_tables(void* const* tables, int n)
{
  DJ_CHECK_ERROR(n >= 1, "concat: at least one table");
  std::vector<std::unique_ptr<cudf::table>> parts;
  for (int i = 0; i < n; i++) parts.emplace_back((cudf::table*)tables[i]);
  return concat_tables(parts).release();
}

const void* dj_table_column_null_mask(void* tbl, int i)
{
  return ((const cudf::table*)tbl)->get_column(i).null_mask();
}
int64_t dj_table_column_null_count(void* tbl, int i)
{
  return ((const cudf::table*)tbl)->get_column(i).null_count();
}

/* test/bench hook for the mask gather (include/distributed_join.h) */
void dj_gather_bitmasks(const void* const* h_src_masks, void* const* h_dst_masks, int ncols,
                        const int64_t* d_idx, int64_t n, int64_t* h_null_counts, int reps,
                        double* h_ms, int cols_per_launch)
{
  hipStream_t st = dj_rt_stream();
  DJ_CHECK_ERROR(ncols >= 0 && ncols <= dj::kMaxSchemaCols, "gather_bitmasks: <= 32 columns");
  dj::BitmaskGatherDesc bd{};
  bd.ncols = ncols;
  for (int c = 0; c < ncols; c++) {
    bd.src[c] = (const uint32_t*)h_src_masks[c];
    bd.dst[c] = (uint32_t*)h_dst_masks[c];
  }
  DBuf d_counts(dj::kMaxSchemaCols * 4);
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipMemsetAsync(d_counts.p, 0, dj::kMaxSchemaCols * 4, st));
    DJ_HIP_CALL(hipEventRecord(e0, st));
    dj::gather_bitmasks(bd, d_idx, n, (uint32_t*)d_counts.p, st,
                        cols_per_launch > 0 ? cols_per_launch : dj::kMaskColsPerLaunch);
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
  uint32_t h_counts[dj::kMaxSchemaCols];
  DJ_HIP_CALL(hipMemcpy(h_counts, d_counts.p, sizeof(h_counts), hipMemcpyDeviceToHost));
  for (int c = 0; c < ncols; c++) h_null_counts[c] = h_counts[c];
}

/* test hook for the mask segment copy + null count (include/distributed_join.h) */
int64_t dj_copy_bitmask_segments(const void* const* h_src_masks, const int64_t* h_src_bits,
                                 const int64_t* h_nbits, int S, void* d_dst)
{
  hipStream_t st = dj_rt_stream();
  std::vector<BitSeg> segs;
  int64_t total = 0;
  for (int i = 0; i < S; i++) {
    segs.push_back(BitSeg{(const uint32_t*)h_src_masks[i], h_src_bits[i], h_nbits[i]});
    total += h_nbits[i];
  }
  DBuf table = copy_bit_segments(segs, (uint32_t*)d_dst, st);
  DBuf cnt(8);
  DJ_HIP_CALL(hipMemsetAsync(cnt.p, 0, 8, st));
  dj::count_unset_bits((const uint32_t*)d_dst, total, (unsigned long long*)cnt.p, st);
  return (int64_t)read_back<unsigned long long>(cnt.p, st);
}

void* dj_cpp_distributed_join_ncols_multi(void* comm, int kind, const dj_ncol_desc* lcols,
                                          int nl, int64_t ln, const dj_ncol_desc* rcols, int nr,
                                          int64_t rn, const int32_t* lon, const int32_t* ron,
                                          int nkeys, int over_decom, int report_timing)
{
  return dj_cpp_distributed_join_ncols_multi_ne(comm, kind, DJ_NULL_EQUAL, lcols, nl, ln, rcols,
                                                nr, rn, lon, ron, nkeys, over_decom,
                                                report_timing);
}

void* dj_cpp_distributed_join_ncols_multi_ne(void* comm, int kind, int null_equality,
                                             const dj_ncol_desc* lcols, int nl, int64_t ln,
                                             const dj_ncol_desc* rcols, int nr, int64_t rn,
                                             const int32_t* lon, const int32_t* ron, int nkeys,
                                             int over_decom, int report_timing)
{
  DJ_CHECK_ERROR(kind >= DJ_JOIN_INNER && kind <= DJ_JOIN_LEFT_ANTI, "join kind must be 0..3");
  DJ_CHECK_ERROR(null_equality == DJ_NULL_EQUAL || null_equality == DJ_NULL_UNEQUAL,
                 "null_equality must be DJ_NULL_EQUAL (0) or DJ_NULL_UNEQUAL (1)");
  auto left = view_from_descs(lcols, nl, ln);
  auto right = view_from_descs(rcols, nr, rn);
  std::vector<cudf::size_type> lo(lon, lon + nkeys), ro(ron, ron + nkeys);
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  auto result = distributed_join((join_kind)kind, left, right, lo, ro, (Communicator*)comm,
                                 lopts, ropts, over_decom, report_timing != 0, nullptr, 1,
                                 null_equality == DJ_NULL_UNEQUAL
                                   ? cudf::null_equality::UNEQUAL
                                   : cudf::null_equality::EQUAL);
  return result.release();
}

/* test/bench hooks for the row-set kernels (include/distributed_join.h) */
void dj_mark_rows(const int64_t* d_idx, int64_t n, void* d_bits, int mode, int reps,
                  double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  time_reps(reps, h_ms, st, [&] {
    dj::mark_rows(d_idx, n, (uint32_t*)d_bits, st, mode < 0 ? dj::kMarkDefault : mode);
  });
}

int64_t dj_select_rows(const void* d_bits, int64_t nrows, int want_set, int64_t* d_out_idx,
                       int reps, double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  DBuf scratch(dj::select_rows_scratch_bytes(nrows)), count(8);
  time_reps(reps, h_ms, st, [&] {
    dj::select_rows((const uint32_t*)d_bits, nrows, want_set != 0, d_out_idx, count.i64(), st,
                    scratch.p);
  });
  int64_t h = 0;
  DJ_HIP_CALL(hipMemcpy(&h, count.p, 8, hipMemcpyDeviceToHost));
  return h;
}

int64_t dj_compact_keyed_rows(const void* d_bits, int64_t nrows, const int64_t* d_keys,
                              int64_t* d_out_idx, int64_t* d_out_keys, int reps, double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  DBuf scratch(dj::select_rows_scratch_bytes(nrows)), count(8);
  time_reps(reps, h_ms, st, [&] {
    dj::compact_keyed_rows((const uint32_t*)d_bits, nrows, d_keys, d_out_idx, d_out_keys,
                           count.i64(), st, scratch.p);
  });
  int64_t h = 0;
  DJ_HIP_CALL(hipMemcpy(&h, count.p, 8, hipMemcpyDeviceToHost));
  return h;
}

int64_t dj_key_row_validity(const void* const* h_masks, int nmasks, int64_t nrows, void* d_out)
{
  hipStream_t st = dj_rt_stream();
  DJ_CHECK_ERROR(nmasks >= 1 && nmasks <= dj::kMaxKeyMasks, "key_row_validity: 1..4 masks");
  const uint32_t* masks[dj::kMaxKeyMasks];
  for (int c = 0; c < nmasks; c++) masks[c] = (const uint32_t*)h_masks[c];
  DBuf cnt(8);
  DJ_HIP_CALL(hipMemsetAsync(cnt.p, 0, 8, st));
  dj::key_row_validity(masks, nmasks, nrows, (uint32_t*)d_out, (unsigned long long*)cnt.p, st);
  return (int64_t)read_back<unsigned long long>(cnt.p, st);
}

int64_t dj_select_rows_tile_rows(void) { return dj::select_rows_tile_rows(); }

/* test/bench hook for the table gather (include/distributed_join.h) */
void dj_gather_columns(const dj_gather_desc* descs, int ncols, const int64_t* d_idx, int64_t n,
                       int mode, int reps, double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  std::vector<dj::GatherCol> gc;
  for (int c = 0; c < ncols; c++)
    gc.push_back(dj::GatherCol{descs[c].src, descs[c].dst, descs[c].width});
  time_reps(reps, h_ms, st, [&] { dj::gather_table(gc.data(), ncols, d_idx, n, mode, st); });
}

/* test hook: d_out[i] = dj_murmur3_bytes(row i, seed) through the STRING-key
 * row-hash kernel (its staged and direct paths, selected per block as in
 * production). Host-synchronous. */
void dj_hash_strings(const void* d_offsets, const void* d_chars, int64_t chars_bytes, int64_t n,
                     uint32_t seed, uint32_t* d_out)
{
  hipStream_t st = dj_rt_stream();
  /* an empty chars buffer is never dereferenced; drop the pointer so a stale
   * one cannot be */
  if (chars_bytes <= 0) d_chars = nullptr;
  dj::hash_strings_seeded((const int32_t*)d_offsets, (const uint8_t*)d_chars, n, seed, d_out,
                          st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
}

/* d_out[i] = dj_string_key64(row i): what a STRING key column contributes to
 * the fused key chain. Launches the kernel `reps` times, each between a
 * hipEvent pair; h_ms (host double[reps], may be NULL) receives the
 * per-launch milliseconds (benchmark/string_key_bench.py). Host-synchronous. */
void dj_string_keys64(const void* d_offsets, const void* d_chars, int64_t chars_bytes,
                      int64_t n, uint64_t* d_out, int reps, double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  if (chars_bytes <= 0) d_chars = nullptr;
  time_reps(reps, h_ms, st, [&] {
    dj::hash_strings((const int32_t*)d_offsets, (const uint8_t*)d_chars, n, d_out, st);
  });
}

/* behavior hook for the parity tests: distribute a 2-column int64 table
 * from rank 0 and collect it back (distribute_table.hpp round trip);
 * returns the collected table on rank 0, nullptr elsewhere */
void* dj_cpp_distribute_collect_roundtrip_i64(void* comm, const int64_t* d_keys,
                                              const int64_t* d_pay, int64_t n)
{
  cudf::table_view global = view_i64_pair(d_keys, d_pay, n);
  auto local = distribute_table(global, (Communicator*)comm);
  auto merged = collect_tables(local->view(), (Communicator*)comm);
  return merged.release();
}

int dj_table_column_type(void* tbl, int i)
{
  return (int)((cudf::table*)tbl)->get_column(i).type().id();
}
const void* dj_table_column_chars(void* tbl, int i)
{
  return ((cudf::table*)tbl)->get_column(i).chars();
}
int64_t dj_table_column_chars_size(void* tbl, int i)
{
  return ((cudf::table*)tbl)->get_column(i).chars_size();
}

int64_t dj_table_num_rows(void* tbl) { return ((cudf::table*)tbl)->num_rows(); }
int dj_table_num_columns(void* tbl) { return ((cudf::table*)tbl)->num_columns(); }
const void* dj_table_column_data(void* tbl, int i)
{
  return ((cudf::table*)tbl)->get_column(i).head();
}
void dj_table_free(void* tbl) { delete (cudf::table*)tbl; }

}  // extern "C"
