/*
 * dj_kernels.hpp — host-side launchers for the gfx950 HIP kernels of the
 * distributed repartitioned hash join hot path.
 *
 * These replace the third-party cuDF 0.19 kernels the reference calls on its
 * hot path (SURVEY.md §2 third-party kernel table):
 *   - hash_partition  <- cudf::hash_partition (distributed_join.cpp:213-225,
 *                        shuffle_on.cpp:59-60)
 *   - build/probe     <- cudf::inner_join (distributed_join.cpp:79)
 *   - generate_*      <- generate_dataset.cuh:40-260 (restated deterministic)
 *
 * All launchers are stream-ordered on the given hipStream_t and operate on
 * raw device pointers (columnar int64 arrays). No torch types.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dj {

/* int64 value marking an empty hash-table slot; build rows carrying it are
 * skipped in-table and joined out-of-band (neg1_cross_join below). Set via
 * 0xFF memset. */
constexpr int64_t kEmptyKey = -1;

/* nparts = world_size x over_decom; the stable wave-ballot partition covers
 * any nparts <= 1024 (lane q owns partitions q, q+64, ... — cost linear in
 * nparts). The reference's own tests drive up to 80 (8 ranks x od 10,
 * compare_against_single_gpu.cu:237-268). */
constexpr int kMaxPartitions = 1024;

/* ----- synthetic inputs (deterministic, spec in dj_rng.h) ----- */
void generate_build(int64_t* d_keys, int64_t* d_pay, int64_t n_global, int64_t rand_max,
                    uint64_t seed, bool uniq, int64_t row0, int64_t nrows, hipStream_t s);
void generate_probe(int64_t* d_keys, int64_t* d_pay, int64_t build_n_global, int64_t rand_max,
                    double selectivity, uint64_t seed, int64_t row0, int64_t nrows, hipStream_t s);

/* ----- stable hash partition (histogram + scan + wave-ballot scatter) ----- */
size_t hash_partition_scratch_bytes(int64_t n, int nparts);
/* sub-steps, so the C ABI can time each kernel separately */
void partition_count(const int64_t* d_keys, int64_t n, int nparts, int hash_fn,
                     uint32_t hash_seed, void* d_scratch, hipStream_t s);
void partition_scan(int64_t n, int nparts, void* d_scratch, int64_t* d_offsets, hipStream_t s);
void partition_scatter(const int64_t* d_keys, const int64_t* d_pay, int64_t n, int nparts,
                       int hash_fn, uint32_t hash_seed, const int64_t* d_offsets,
                       void* d_scratch, int64_t* d_out_keys, int64_t* d_out_pay,
                       hipStream_t s);
/* d_offsets: device array of nparts+1 int64 partition offsets (offsets[0]=0).
 * Stable: rows keep input order inside each partition. nparts <= 1024. */
void hash_partition(const int64_t* d_keys, const int64_t* d_pay, int64_t n, int nparts,
                    int hash_fn, uint32_t hash_seed, int64_t* d_out_keys, int64_t* d_out_pay,
                    int64_t* d_offsets, void* d_scratch, hipStream_t s);

/* ----- local inner join: open-addressing build + probe-append ----- */
/* Number of table slots for ln build rows (power of two, <=50% fill).
 * The table buffer holds nslots interleaved 16 B {key,val} pairs
 * (2*nslots int64). */
int64_t join_table_slots(int64_t ln);
/* Initialize table pairs to kEmptyKey (async memset over 16*nslots bytes). */
void join_table_init(int64_t* d_table, int64_t nslots, hipStream_t s);
/* Insert build rows. d_error (device int32) set to 1 if any key==kEmptyKey. */
void join_build(const int64_t* d_lk, const int64_t* d_lp, int64_t ln, int64_t* d_table,
                int64_t nslots, int* d_error, hipStream_t s);
/* Probe rows; append matches (lkey, lpay, rkey, rpay) to the 4 output
 * columns at positions drawn from d_counter (device int64, caller-zeroed),
 * one wave-aggregated atomic per emit round. Rows beyond `cap` are counted
 * but not written (caller re-runs bigger). */
void join_probe(const int64_t* d_rk, const int64_t* d_rp, int64_t rn, const int64_t* d_table,
                int64_t nslots, int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                int64_t* d_out3, int64_t cap, int64_t* d_counter, hipStream_t s);

/* ----- bucketed LDS join (the product local-join path; see dj_kernels.hip
 * "bucketed LDS join" comment block) ----- */
constexpr int kBucketBlocks = 512;
constexpr int kSubBuckets = 256;
constexpr int kJoinBucketRowCap = 1536;  // 75% of the 2048-slot LDS table
int bucket_count_for(int64_t ln, int64_t rn);
/* decomposition B = PA x F: PA pass-A groups (<=1024, one per thread in the
 * scans), F pass-B sub-buckets (256 up to B=262144 — the historical shape —
 * then 512/1024, bit fields disjoint per subF_of) */
inline int bucket_groups_for(int B)
{
  int PA = B / 256;
  if (PA < 1) PA = 1;
  if (PA > 1024) PA = 1024;
  return PA;
}
/* pass-A slack segment capacity (rows per group): mean + ~6% + 1024 covers
 * hash-uniform inputs w.h.p.; skewed inputs overflow -> bit 2 of
 * any_overflow -> the caller redoes the join exactly */
inline int64_t slack_capA(int64_t n, int PA)
{
  const int64_t m = n / PA;
  return m + m / 16 + 1024;
}
/* per-bucket slack capacity for the count-free pass B (mean + 16 sqrt(mean),
 * rounded to 8). 7 sigma covers Poisson (unique-ish keys) but duplicate keys
 * inflate bucket variance by ~(1 + multiplicity): TPC-H lineitem (m ~ 4)
 * overflowed 7 sigma EVERY step, wasting the slack attempt before the exact
 * compact retry. 16 sqrt(lam) covers multiplicity up to ~8 for ~25% more
 * slack memory; beyond that bit 2 of any_overflow still routes to the
 * compact retry (same contract as slack_capA). */
inline int64_t slack_capB(int64_t n, int B)
{
  const int64_t lam = n / B < 1 ? 1 : n / B;
  int64_t s = 1;
  while (s * s < lam) s++;  // ceil(sqrt(lam))
  int64_t cap = lam + 16 * s + 16;
  return (cap + 7) & ~(int64_t)7;
}
/* Two-level non-stable partition into B buckets (B = PA*F per
 * bucket_groups_for; up to 1024x1024 = 1M buckets for ~800M-row tables) of
 * interleaved 16 B {key,payload} pairs. d_tmp_pairs: pass-A staging —
 * longlong2[PA * slack_capA(n, PA)] when d_any_overflow is non-null (the
 * slack path: no count pass; group skew beyond the slack sets BIT 2 of
 * *d_any_overflow and the partition output is INCOMPLETE — caller must redo
 * the whole join), else longlong2[n] (exact two-pass path). d_counts:
 * u32[kBucketBlocks*PA]; d_totals: u32[PA]; d_segoff: int64[PA+1];
 * d_offsets: int64[B+1]. */
void bucket_partition2(const int64_t* d_keys, const int64_t* d_pay, int64_t n, int B,
                       longlong2* d_tmp_pairs, uint32_t* d_counts, uint32_t* d_totals,
                       int64_t* d_segoff, int64_t* d_offsets, longlong2* d_out_pairs,
                       int* d_any_overflow, hipStream_t s);
/* Count-free two-level slack partition of BOTH tables (round 2, the product
 * local-join path): pass A as bucket_partition2's slack path, then pass B
 * scatters each group's rows into per-bucket SLACK segments at analytic
 * starts b*capB (capB = slack_capB(n, B)) with LDS cursors — no seghist sweep
 * (the r1 pass B fetched full 16 B lines just to histogram 8 B keys: 3.28 GB
 * PMC fetch vs 2.4 GB algorithmic). Bucket b of table t holds d_len<t>[b]
 * rows at d_out<t>[b*capB<t>]. Both tables go through one pass-A and one
 * pass-B launch (tail-wave fill), so each needs a private tmp/cursor set:
 * d_tmp<t>: longlong2[PA*slack_capA(n<t>,PA)]; d_cur<t>: u32[PA]. Overflow of
 * any slack segment sets bit 2 of *d_any_overflow (partition output
 * incomplete -> caller redoes exactly). Requires PA >= 2, n < 2^32,
 * PA*slack_capA(n,PA)+n and B*capB < 2^32 (checked; errors loudly
 * otherwise).
 * Contracts the direct tests rely on (tests/cpp/slack_pair_check.cpp):
 * - capB<t> is ANY caller-chosen per-bucket capacity >= 1 — the layout, the
 *   limits and the length clamp all derive from the argument; slack_capB(n, B)
 *   is merely what the product passes. d_out<t> is longlong2[B*capB<t>].
 * - n0 + n1 >= 1: the pass-A grid split divides by n0 + n1 (either table
 *   alone may be empty; its lens are then all 0).
 * - bits already set in *d_any_overflow are kept (the kernels only OR in 2);
 *   d_cur<t> needs no reset by the caller and reads back min(group count,
 *   slack_capA) per group. */
void bucket_partition2_slack_pair(const int64_t* d_k0, const int64_t* d_p0, int64_t n0,
                                  longlong2* d_tmp0, uint32_t* d_cur0, int64_t capB0,
                                  longlong2* d_out0, uint32_t* d_len0, const int64_t* d_k1,
                                  const int64_t* d_p1, int64_t n1, longlong2* d_tmp1,
                                  uint32_t* d_cur1, int64_t capB1, longlong2* d_out1,
                                  uint32_t* d_len1, int B, int* d_any_overflow,
                                  hipStream_t s);
/* Fused per-bucket LDS build+probe over bucketed pair tables. table_slots:
 * 2048 (2 blocks/CU, bucket cap 1536 build rows = kJoinBucketRowCap) or
 * 4096 (1 block/CU, cap 3072 — for the fused wire path when the PA*F
 * fan-out cap leaves big buckets). Buckets whose build side exceeds the cap
 * set overflow_flags[b]/any_overflow and are skipped (host runs the
 * global-table path on them / redoes the batch). Contract: B must be a
 * multiple of 4 (the in-kernel flush-group size; every bucket_count_for and
 * fused-wire PA*F is) — errors loudly otherwise. */
void lds_join(const longlong2* d_lrows, const int64_t* d_loff, const longlong2* d_rrows,
              const int64_t* d_roff, int B, int table_slots, int64_t* d_out0, int64_t* d_out1,
              int64_t* d_out2, int64_t* d_out3, int64_t cap, int64_t* d_counter,
              uint32_t* d_overflow_flags, int* d_any_overflow, int* d_error, hipStream_t s);
/* Same fused join over the slack bucket layout of
 * bucket_partition2_slack_pair:
 * bucket b = d_lrows[b*capL .. +d_llen[b]) x d_rrows[b*capR .. +d_rlen[b]).
 * Contract: B must be a multiple of 4 (the in-kernel flush-group size) —
 * pad d_llen/d_rlen with zero-length buckets; errors loudly otherwise. */
void lds_join_slack(const longlong2* d_lrows, const uint32_t* d_llen, int64_t capL,
                    const longlong2* d_rrows, const uint32_t* d_rlen, int64_t capR, int B,
                    int table_slots, int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                    int64_t* d_out3, int64_t cap, int64_t* d_counter,
                    uint32_t* d_overflow_flags, int* d_any_overflow, int* d_error,
                    hipStream_t s);
/* lds_join_kernel's shape (tests size their buckets from it): rows of the
 * LDS output stage; the staged-row count at which a bucket before its group's
 * last one flushes early; buckets per flush group; the grid cap in groups (a
 * block takes group blockIdx.x + k * grid_groups in its trip k). */
struct LdsJoinShape {
  int stage_rows, watermark, flush_group, grid_groups;
};
LdsJoinShape lds_join_shape();
/* the partition launchers' shape (tests size their inputs from it): rows of
 * the staged tile of the counted scatters and pass B over lists
 * (fused_partition, subpart_lists, bucket_partition2), of the slack pass A and
 * of the slack pass B; chunking blocks per table of a pass A (the slack pair
 * launches 2 * bucket_blocks and splits them by table size); block size. */
struct BucketPartitionShape {
  int scatter_tile, slack_tile, btile, bucket_blocks, bucket_threads;
};
BucketPartitionShape bucket_partition_shape();
/* the stable hash partition's geometry (tests size their inputs from it): a
 * wave takes ceil(n / nwaves) consecutive rows, nwaves = ceil(n /
 * target_rows_per_wave) capped at wave_cap and rounded up to whole blocks of
 * waves_per_block waves; the per-partition scan over the waves covers
 * scan_block of them per pass. */
struct HashPartitionShape {
  int target_rows_per_wave, wave_cap, waves_per_block, scan_block;
};
HashPartitionShape hash_partition_shape();
/* the global-table join's and neg1_cross_join's grid: block size and the cap
 * in blocks; one trip of a kernel covers block * grid_cap rows */
struct TableJoinShape {
  int block, grid_cap;
};
TableJoinShape table_join_shape();
/* Global-table build/probe over interleaved pair inputs (skew fallback). */
void join_build_pairs(const longlong2* d_rows, int64_t ln, int64_t* d_table, int64_t nslots,
                      int* d_error, hipStream_t s);
void join_probe_pairs(const longlong2* d_rows, int64_t rn, const int64_t* d_table,
                      int64_t nslots, int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                      int64_t* d_out3, int64_t cap, int64_t* d_counter, hipStream_t s);

/* ----- strings-column kernels (dj_strings.hip; see its header comment for
 * the reference helpers each replaces) ----- */
void sizes_from_offsets(const int32_t* d_offsets, int64_t n, int32_t* d_sizes, hipStream_t s);
/* true 64-bit total of int32 sizes -> d_total (one i64; caller zeroes) —
 * overflow guard for the int32 offsets convention */
void sum_sizes_i64(const int32_t* d_sizes, int64_t n, int64_t* d_total, hipStream_t s);
size_t offsets_from_sizes_scratch_bytes(int64_t n);
void offsets_from_sizes(const int32_t* d_sizes, int64_t n, int32_t* d_offsets, void* d_scratch,
                        hipStream_t s);
void gather_sizes_starts(const int32_t* d_src_off, const int64_t* d_idx, int64_t n,
                         int32_t* d_sizes, int32_t* d_starts, hipStream_t s);
void gather_chars_from_starts(const uint8_t* d_src_chars, const int32_t* d_starts, int64_t n,
                              const int32_t* d_dst_off, uint8_t* d_dst_chars, hipStream_t s);
void gather_sizes(const int32_t* d_src_off, const int64_t* d_idx, int64_t n, int32_t* d_sizes,
                  hipStream_t s);
/* STRING key columns (dj_strhash.h spec): d_out[i] = dj_string_key64 of row
 * i. Reads offsets[0..n] and exactly the chars bytes the rows cover. */
void hash_strings(const int32_t* d_offsets, const uint8_t* d_chars, int64_t n, uint64_t* d_out,
                  hipStream_t s);
/* same kernel, d_out[i] = dj_murmur3_bytes(row i, seed) (test hook) */
void hash_strings_seeded(const int32_t* d_offsets, const uint8_t* d_chars, int64_t n,
                         uint32_t seed, uint32_t* d_out, hipStream_t s);
/* collision filter over key tuples of integer-rep and STRING columns: keep
 * the (li, ri) pairs whose key tuples are equal column by column (strings: length, then
 * bytes); appends to d_out_li/d_out_ri at positions drawn from *d_count
 * (caller-zeroed), order unspecified. Per column and side: kind, data
 * (values, or int32 offsets for kKeyStr) and chars (kKeyStr only). */
enum {
  kKeyI32 = 0,
  kKeyI64 = 1, /* also UINT64, reinterpreted */
  kKeyStr = 2,
  kKeyI8 = 3,
  kKeyI16 = 4,
  kKeyU8 = 5, /* also BOOL8 */
  kKeyU16 = 6,
  kKeyU32 = 7
};
/* element i of an integer-rep key column as the engine's int64 key: signed
 * reps sign-extend, unsigned reps zero-extend */
__host__ __device__ __forceinline__ int64_t load_key_i64(const void* p, int kind, int64_t i)
{
  switch (kind) {
    case kKeyI64: return ((const int64_t*)p)[i];
    case kKeyI32: return (int64_t)((const int32_t*)p)[i];
    case kKeyU32: return (int64_t)((const uint32_t*)p)[i];
    case kKeyI16: return (int64_t)((const int16_t*)p)[i];
    case kKeyU16: return (int64_t)((const uint16_t*)p)[i];
    case kKeyI8: return (int64_t)((const int8_t*)p)[i];
    default: return (int64_t)((const uint8_t*)p)[i];
  }
}
/* the element hash a null key element contributes (cuDF's row-hasher
 * convention; spec in dj_hash.h) */
constexpr uint32_t kNullKeyHash = 0xFFFFFFFFu;
struct TupleKeyCol {
  const void* data;
  const uint8_t* chars;
  int kind;
  const uint32_t* valid; /* validity mask, or nullptr: every element valid */
};
__host__ __device__ __forceinline__ bool key_is_valid(const uint32_t* valid, int64_t i)
{
  return valid == nullptr || ((valid[i >> 5] >> (i & 31)) & 1u);
}
struct TupleKeys {
  TupleKeyCol l[4], r[4];
  int nk;
};
void filter_tuple_matches_mixed(const TupleKeys& keys, const int64_t* d_li, const int64_t* d_ri,
                                int64_t n, int64_t* d_out_li, int64_t* d_out_ri,
                                unsigned long long* d_count, hipStream_t s);
void make_test_string_sizes(const int64_t* d_keys, int64_t n, int32_t* d_sizes, hipStream_t s);
void fill_test_strings(const int64_t* d_keys, int64_t n, const int32_t* d_offsets,
                       uint8_t* d_chars, hipStream_t s);

/* ----- fused rank+group partition + segment-list pass B (fast2 wire path;
 * see dj_kernels.hip "fused rank+group partition" block) ----- */
void fused_partition(const int64_t* d_keys, const int64_t* d_pay, int64_t n, int nparts_rank,
                     uint32_t seed, int PA, uint32_t* d_counts, uint32_t* d_totals,
                     int64_t* d_offsets, int64_t* d_out_keys, int64_t* d_out_pay,
                     hipStream_t s);
void subpart_lists(const int64_t* d_keys, const int64_t* d_pay, const int64_t* d_seg_bounds,
                   int nseg, int PA, int F, const int64_t* d_group_base,
                   longlong2* d_out_pairs, int64_t* d_bucket_offsets, hipStream_t s);

/* ----- cascaded codec (dj_compress.hip; wire format in its header) -----
 * 32-byte slice header. scheme bit0 = delta, bit1 = RLE (values subslice
 * and run-lengths subslice follow, each bitpacked; nruns/len_bits valid
 * iff RLE). bits == 0xFFFF means stored raw (scheme ignored). */
struct CompSliceHeader {
  uint32_t bits;      // value bit width (0xFFFF = raw)
  uint32_t scheme;    // bit0 delta, bit1 RLE
  uint64_t count;     // original element count
  uint64_t nruns;     // RLE only
  uint32_t len_bits;  // RLE only: run-length bit width
  uint32_t reserved;
};
size_t compress_bound(int64_t count, int elem_size);
size_t compress_scratch_bytes(int64_t count);
/* num_rles > 0 requires d_scratch (compress_scratch_bytes(count)); the
 * packed-vs-raw decision happens on-device, fully stream-ordered. The
 * final 32 B header at d_out carries everything needed for
 * compressed_size_from_header after one sync. */
void compress_slice_async(const void* d_in, int64_t count, int elem_size, int num_rles,
                          int num_deltas, int use_bp, uint8_t* d_out, void* d_scratch,
                          hipStream_t s);
size_t compressed_size_from_header(const CompSliceHeader& h, int elem_size);
void decompress_slice_async(const uint8_t* d_comp, const CompSliceHeader& h, int elem_size,
                            void* d_out, void* d_scratch, hipStream_t s);

/* ----- table gather (dj_kernels.hip "table gather" block) -----
 * dst[i] = src[idx[i]], i in [0, n), for every fixed-width column of a table
 * through ONE index array. width is the element size in bytes (1/2/4/8);
 * src may be any element-aligned address, dst must be 16-byte aligned (a
 * fresh column from the arena is). Reads idx[0..n) and the indexed source
 * elements, writes dst bytes [0, n*width) and nothing else. */
constexpr int kMaxSchemaCols = 32;
struct GatherCol {
  const void* src;
  void* dst;
  int width;
};
struct GatherDesc {
  GatherCol col[kMaxSchemaCols];
  int ncols;
};
enum {
  kGatherFused = 0,     /* one launch for all columns, 4 rows/thread, packed stores */
  kGatherPerColumn = 1, /* one launch per column, 1 row/thread */
  kGatherAuto = 2       /* per-width routing by measurement */
};
void gather_table(const GatherCol* cols, int ncols, const int64_t* d_idx, int64_t n, int mode,
                  hipStream_t s);

/* ----- validity masks (dj_bitmask.hip; cuDF layout: row i = bit i % 32 of
 * uint32 word i / 32, 1 = valid, nullptr = all valid) ----- */
struct BitmaskGatherDesc {
  const uint32_t* src[kMaxSchemaCols]; /* nullptr: every gathered bit is 1 */
  uint32_t* dst[kMaxSchemaCols];       /* 8-byte aligned, roundup(n, 64) / 8 bytes */
  int ncols;
};
/* columns one gather_bitmasks launch takes: the kernel handles up to
 * kMaxSchemaCols, but a launch that interleaves many source masks loses their
 * cache residency, so the engine launches once per column */
constexpr int kMaskColsPerLaunch = 1;
/* dst_c bit i = src_c bit idx[i], i in [0, n); dst bits [n, roundup(n, 64))
 * are written 0. d_null_counts[c] (caller-zeroed, kMaxSchemaCols entries) is
 * advanced by the number of 0 bits written to column c among the n rows. */
void gather_bitmasks(const BitmaskGatherDesc& desc, const int64_t* d_idx, int64_t n,
                     uint32_t* d_null_counts, hipStream_t s,
                     int cols_per_launch = kMaskColsPerLaunch);
/* Concatenate S bit ranges into d_dst. d_segments is one device block of
 * 8-byte entries: S source mask pointers (nullptr = all valid), S source bit
 * offsets, then S+1 destination bit offsets — non-decreasing, [0] = 0,
 * [S] = total_bits, so segment s fills destination bits
 * [dst_bit[s], dst_bit[s+1]) (zero length allowed). Writes the
 * ceil(total_bits / 32) destination words whole, bits past total_bits as 0;
 * of segment s it reads only source words src_bit/32 ..
 * (src_bit + nbits - 1)/32. */
void copy_bitmask_segments(const void* d_segments, int S, int64_t total_bits, uint32_t* d_dst,
                           hipStream_t s);
/* *d_count (caller-zeroed) += number of 0 bits among the first n of d_mask */
void count_unset_bits(const uint32_t* d_mask, int64_t n, unsigned long long* d_count,
                      hipStream_t s);
/* Row validity of a key tuple: word w of d_out = the AND of word w of the
 * nmasks (1..kMaxKeyMasks) host-listed device masks, a null pointer counting
 * as all ones; bits at and past nrows are written as 0 whatever the sources
 * hold there. d_out holds ceil(nrows / 32) words, each stored once.
 * *d_null_count (caller-zeroed) += the 0 bits among the first nrows. Runs on
 * the mask-word grid (kSpanMaskWords). */
constexpr int kMaxKeyMasks = 4;
void key_row_validity(const uint32_t* const* masks, int nmasks, int64_t nrows, uint32_t* d_out,
                      unsigned long long* d_null_count, hipStream_t s);

/* ----- row sets (dj_rowset.hip; same bit layout, here 1 = "row is in the
 * set"): from a join's pair list to the rows a left / semi / anti join keeps */
/* mark_rows variants, for the benchmark's ablation; the engine runs
 * kMarkDefault: the wave merge alone. The load check never paid for itself
 * on MI355X — the atomic OR on the L2-resident bitmap costs what the load
 * costs. */
constexpr int kMarkMerge = 1; /* lanes naming one word combine their bits first */
constexpr int kMarkCheck = 2; /* load the word, skip the atomic when nothing is new */
constexpr int kMarkDefault = kMarkMerge;
/* Sets bit d_idx[i] of d_bits for every i < n. The caller zeroes d_bits
 * (ceil(nrows / 32) words) and guarantees 0 <= d_idx[i] < nrows. Any index may
 * occur any number of times. Reads d_idx[0..n); writes (atomic OR) only words
 * that hold a marked bit. */
void mark_rows(const int64_t* d_idx, int64_t n, uint32_t* d_bits, hipStream_t s,
               int mode = kMarkDefault);
/* Writes to d_out_idx, ascending, the i < nrows whose bit of d_bits equals
 * want_set, and their number to *d_count. Bits at and past nrows in the last
 * word are ignored. d_out_idx holds as many elements as are selected (nrows
 * always suffices); d_scratch holds select_rows_scratch_bytes(nrows). Reads
 * ceil(nrows / 32) words of d_bits. */
size_t select_rows_scratch_bytes(int64_t nrows);
void select_rows(const uint32_t* d_bits, int64_t nrows, bool want_set, int64_t* d_out_idx,
                 int64_t* d_count, hipStream_t s, void* d_scratch);
/* select_rows(want_set = true) that carries a key along: d_out_idx as there,
 * and d_out_keys[k] = d_keys[d_out_idx[k]]. d_keys holds nrows elements, both
 * outputs as many as are selected; scratch and grid (kSpanSelectRows) are
 * select_rows'. */
void compact_keyed_rows(const uint32_t* d_bits, int64_t nrows, const int64_t* d_keys,
                        int64_t* d_out_idx, int64_t* d_out_keys, int64_t* d_count,
                        hipStream_t s, void* d_scratch);
/* rows one block of select_rows ranks at a time (tests probe around it) */
int64_t select_rows_tile_rows();

/* ----- test hook: what one launch of a capped-grid helper kernel covers -----
 * Every helper kernel outside the bucket-join core runs on a grid capped at a
 * few thousand blocks and takes the rest of its input in further trips of a
 * grid-stride loop; the scans behind them turn per-tile partials into offsets
 * in one block, in passes. `trip` is the number of items (rows, words, groups
 * x 32 values — the unit the family's callers size by) one full grid covers
 * in one trip, `scan_pass` the number of items whose partials one pass of the
 * single-block scan covers (0: the family has no such scan). Each file answers
 * for its own families from the constants its launchers use, and returns
 * {0, 0} for a family of another file. Tests size their inputs from these. */
struct GridSpan {
  int64_t trip;
  int64_t scan_pass;
};
enum {
  kSpanMaskGather = 0,   /* gather_bitmasks: rows */
  kSpanMaskWords = 1,    /* copy_bitmask_segments, count_unset_bits, key_row_validity:
                            mask words */
  kSpanMarkRows = 2,     /* mark_rows: indices */
  kSpanSelectRows = 3,   /* select_rows, compact_keyed_rows: rows; scan_pass: tile_scan
                            with chunk 1 */
  kSpanGatherFused = 4,  /* gather_table, fused kernel: rows */
  kSpanGatherColumn = 5, /* gather_table, per-column kernel: rows */
  kSpanStringRows = 6,   /* sizes_from_offsets, gather_sizes_starts,
                            gather_chars_from_starts, filter_tuple_matches_mixed */
  kSpanStringSum = 7,    /* sum_sizes_i64: rows */
  kSpanStringScan = 8,   /* offsets_from_sizes: rows */
  kSpanStringHash = 9,   /* hash_strings: rows */
  kSpanCodecElems = 10,  /* codec element loops: elements; scan_pass: values of
                            scan64_exclusive */
  kSpanCodecPack = 11,   /* codec pack loops: values (32 per group) */
  kSpanKeyHelpers = 12,  /* widen_key, narrow_key, fuse_key_columns, nullable_key_hash,
                            rebase_offsets (dj_key_helpers.hip): rows */
  kSpanFamilies = 13
};
GridSpan bitmask_grid_span(int family);
GridSpan rowset_grid_span(int family);
GridSpan gather_grid_span(int family);
GridSpan strings_grid_span(int family);
GridSpan compress_grid_span(int family);
GridSpan key_helper_grid_span(int family); /* dj_key_helpers.hip */

/* ----- key helper kernels (dj_key_helpers.hip): a thread per row, grid
 * kSpanKeyHelpers. Enqueue only; n >= 0 rows ----- */
/* d_dst[i] = i / = value */
void iota_i64(int64_t* d_dst, int64_t n, hipStream_t s);
void fill_i32(int32_t* d_dst, int64_t n, int32_t value, hipStream_t s);
/* integer-rep key column of kind kKey* <-> the engine's int64 key:
 * d_dst[i] = load_key_i64(d_src, kind, i); back by truncation to `width`
 * (1, 2 or 4) bytes */
void widen_key(const void* d_src, int kind, int64_t n, int64_t* d_dst, hipStream_t s);
void narrow_key(const int64_t* d_src, int64_t n, int width, void* d_dst, hipStream_t s);
/* d_out[i] = the dj_mix64 chain over row i of ncols (<= 4) key columns; kinds
 * holds 4 bits of kKey* per column, d_masks[c] (nullptr = all valid) makes a
 * null element enter as kNullKeyHash; weak != 0 keeps 4 bits of the hash */
void fuse_key_columns(const int64_t* const d_cols[4], const uint32_t* const d_masks[4],
                      uint32_t kinds, int ncols, int64_t n, int weak, int64_t* d_out,
                      hipStream_t s);
/* d_out[i] = dj_row_hash of a valid element of a nullable key column,
 * kNullKeyHash of a null one */
void nullable_key_hash(const void* d_src, int kind, const uint32_t* d_valid, int64_t n,
                       int hash_fn, uint32_t seed, int64_t* d_out, hipStream_t s);
/* d_dst[i] = d_src[i] + base (STRING offsets of a concatenated part) */
void rebase_offsets(const int32_t* d_src, int64_t n, int32_t base, int32_t* d_dst, hipStream_t s);

/* ----- small utilities ----- */
void fill_i64(int64_t* d_dst, int64_t value, int64_t n, hipStream_t s);
/* out-of-band join of rows whose key equals the reserved empty sentinel
 * (-1): every table path skips them (setting the saw-sentinel flag); this
 * collects both sides' -1 payloads and appends their cross product to the
 * output, advancing *d_counter. Host-synchronous; rare path. */
void neg1_cross_join(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                     const int64_t* d_rk, const int64_t* d_rp, int64_t rn, int64_t* d_out0,
                     int64_t* d_out1, int64_t* d_out2, int64_t* d_out3, int64_t cap,
                     int64_t* d_counter, hipStream_t s);

}  // namespace dj
