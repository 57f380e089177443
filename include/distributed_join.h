/*
 * distributed_join.h — C ABI of the MI355X-native distributed repartitioned
 * hash join (libdistjoin.so).
 *
 * This is the drop-in boundary for the hot path of rapidsai/distributed-join
 * (reference at /root/reference). Each entry point names the reference
 * interface it replaces (file:line). The C++ surface mirroring the
 * reference's exact signatures (distributed_inner_join / shuffle_on /
 * Communicator) lives in include/distributed_join.hpp; this C ABI is the
 * additive layer the Python/ctypes measurement harness binds (SURVEY.md
 * §8b: "a thin C ABI ... exported for the Python/ctypes measurement
 * harness — additive, not replacing the C++ surface").
 *
 * Conventions: plain pointers + sizes, no torch/cudf types. Pointers named
 * d_* are DEVICE pointers (HIP), h_* are host pointers. All compute calls
 * are stream-ordered on the library's internal HIP stream; dj_sync()
 * synchronizes it. Errors print and exit(1), mirroring the reference's
 * error.hpp:22-99 contract.
 */
#ifndef DISTRIBUTED_JOIN_H
#define DISTRIBUTED_JOIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- device & memory management (replaces RMM pool usage,
 * reference src/setup.cpp:51-106; pool semantics via hipMallocAsync pool) */
int dj_device_count(void);
void dj_set_device(int device);
void* dj_dmalloc(int64_t bytes);
void dj_dfree(void* ptr);
void dj_memcpy_h2d(void* d_dst, const void* h_src, int64_t bytes);
void dj_memcpy_d2h(void* h_dst, const void* d_src, int64_t bytes);
void dj_memcpy_d2d(void* d_dst, const void* d_src, int64_t bytes);
void dj_sync(void);

/* ---------------- deterministic synthetic inputs (replaces
 * generate_dataset.cuh:40-260 / generate_table.cuh:39-57; spec: dj_rng.h).
 * Writes rows [row0, row0+nrows) of the GLOBAL table into device arrays. */
void dj_generate_build(int64_t* d_keys, int64_t* d_pay, int64_t n_global, int64_t rand_max,
                       uint64_t seed, int uniq, int64_t row0, int64_t nrows);
void dj_generate_probe(int64_t* d_keys, int64_t* d_pay, int64_t build_n_global,
                       int64_t rand_max, double selectivity, uint64_t seed, int64_t row0,
                       int64_t nrows);

/* ---------------- stable hash partition (replaces cudf::hash_partition as
 * called at distributed_join.cpp:213-225 and shuffle_on.cpp:59-60).
 * hash_fn: 0 = MURMUR3, 1 = IDENTITY (dj_hash.h spec). nparts in [1,64].
 * h_offsets: HOST int64[nparts+1] partition offsets (synchronizes). */
int64_t dj_partition_scratch_bytes(int64_t n, int nparts);
void dj_hash_partition(const int64_t* d_keys, const int64_t* d_pay, int64_t n, int nparts,
                       int hash_fn, uint32_t hash_seed, int64_t* d_out_keys,
                       int64_t* d_out_pay, int64_t* h_offsets, void* d_scratch);

/* ---------------- local inner join (replaces cudf::inner_join as called at
 * distributed_join.cpp:71-83). Open-addressing table of nslots =
 * dj_join_table_slots(ln) interleaved 16 B {key,val} pairs; caller
 * allocates d_table (2*nslots int64), d_error (1 int32, zeroed), d_counter
 * (1 int64, zeroed). Output columns are (lkey, lpay, rkey, rpay) — left
 * columns then right columns with the join key duplicated, row order
 * unspecified (reference pin: compare_against_single_gpu.cu:163-174).
 * Build keys equal to -1 (the empty-slot sentinel) are a loud error. */
int64_t dj_join_table_slots(int64_t ln);
void dj_join_table_init(int64_t* d_table, int64_t nslots);
void dj_join_build(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                   int64_t* d_table, int64_t nslots, int* d_error);
void dj_join_probe(const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                   const int64_t* d_table, int64_t nslots,
                   int64_t* d_out0, int64_t* d_out1, int64_t* d_out2, int64_t* d_out3,
                   int64_t cap, int64_t* d_counter);
int64_t dj_read_counter_i64(const int64_t* d_counter);
int dj_read_error_i32(const int* d_error);

/* ---------------- bucketed LDS local join (the PRODUCT local-join path;
 * same drop-in semantics as above, different engine: both tables are
 * bucket-partitioned so each bucket's hash table lives in LDS — no
 * HBM-resident table, all hot random access on-chip). Buckets whose build
 * side exceeds the LDS capacity (data skew / heavy duplicates) fall back to
 * the global-table path transparently. d_counter/d_error as above. */
int64_t dj_bucket_join_scratch_bytes(int64_t ln, int64_t rn);
void dj_bucket_local_join(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                          const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                          int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                          int64_t* d_out3, int64_t cap, int64_t* d_counter, int* d_error,
                          void* d_scratch);

/* Convenience one-call local join over the bucketed path (allocates its own
 * scratch; for tests and smoke, not the bench timed region). Returns the
 * match count; writes at most cap rows. */
int64_t dj_local_inner_join(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                            const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                            int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                            int64_t* d_out3, int64_t cap);
/* Same over the global-table build/probe path (the fallback engine),
 * exposed so tests can cross-check both engines. */
int64_t dj_local_inner_join_global(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                                   const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                                   int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                                   int64_t* d_out3, int64_t cap);

/* ---------------- phase timing (hipEvent pairs around every kernel launch;
 * replaces the reference's report_timing wall-clock prints,
 * distributed_join.cpp:120-130,235-240) */
enum dj_phase {
  DJ_PHASE_GENERATE = 0,
  DJ_PHASE_PART_COUNT = 1,
  DJ_PHASE_PART_SCAN = 2,
  DJ_PHASE_PART_SCATTER = 3,
  DJ_PHASE_TABLE_INIT = 4,
  DJ_PHASE_BUILD = 5,
  DJ_PHASE_PROBE = 6,
  DJ_PHASE_COMM = 7,
  DJ_PHASE_CONCAT = 8,
  DJ_PHASE_BUCKET_COUNT = 9,
  DJ_PHASE_BUCKET_SCAN = 10,
  DJ_PHASE_BUCKET_SCATTER = 11,
  DJ_PHASE_JOIN_FUSED = 12,
  DJ_PHASE_GATHER = 13, /* output assembly: the table gather + key narrowing */
  DJ_PHASE_COUNT_ = 14
};
void dj_timing_enable(int on);
void dj_timing_reset(void);
/* total milliseconds and number of launches recorded for a phase
 * (synchronizes the stream) */
double dj_timing_total_ms(int phase);
int64_t dj_timing_launches(int phase);

/* ---------------- RCCL communicator over xGMI (replaces the reference's
 * UCX/NCCL Communicator, communicator.hpp:31-90 + communicator.cpp:783-869;
 * bootstrap id is exchanged by the launcher, replacing MPI_Bcast of
 * ncclUniqueId at communicator.cpp:799-817). */
int dj_rccl_unique_id_bytes(void);
void dj_rccl_get_unique_id(void* h_id_bytes);
void dj_comm_init(int rank, int size, const void* h_id_bytes);
void dj_comm_finalize(void);
int dj_comm_rank(void);
int dj_comm_size(void);
/* grouped peer-slice exchange: for each peer p, send send_counts[p] int64
 * elements from d_send + send_offsets[p], receive recv_counts[p] into
 * d_recv + recv_offsets[p] (counts/offsets are HOST arrays, elements).
 * Implements send/recv_data_by_offset + all_to_all_comm
 * (all_to_all_comm.cpp:126-189,307-478) as one ncclGroupStart/End of
 * ncclSend/ncclRecv on the comm stream — no staging copies (RCCL takes
 * device pointers directly; the reference's 256 B staging at
 * communicator.cpp:820-869 is unnecessary over xGMI). */
void dj_all_to_all_i64(const int64_t* d_send, const int64_t* h_send_offsets,
                       int64_t* d_recv, const int64_t* h_recv_offsets);
/* exchange per-peer row counts (host arrays of size comm_size):
 * replaces communicate_sizes (all_to_all_comm.cpp:54-100) */
void dj_exchange_sizes(const int64_t* h_send_counts, int64_t* h_recv_counts);
/* world-1 RCCL init + grouped self send/recv of n bytes through the
 * RCCLCommunicator path (the same calls the N>1 exchange makes per peer);
 * returns 0 on success, 1 on payload mismatch */
int dj_rccl_selftest(int64_t n);

/* cascaded codec roundtrip (test hook): compress count elements of
 * elem_size (1/2/4/8) from d_in with {num_rles, num_deltas, use_bp} cascaded
 * passes, decompress into d_out, return the wire size in bytes */
int64_t dj_compress_roundtrip(const void* d_in, int64_t count, int elem_size, int num_rles,
                              int num_deltas, int use_bp, void* d_out);

/* ---------------- column descriptors + STRING key columns.
 * A column handed over the C ABI: type_id is a cudf::type_id value
 * (include/dj_cudf_types.hpp): 1=INT8, 2=INT32, 3=INT64, 4=STRING,
 * 5..9=TIMESTAMP_{DAYS,SECONDS,MILLISECONDS,MICROSECONDS,NANOSECONDS},
 * 10..14=DURATION_{same units}, 15=INT16, 16=UINT8, 17=UINT16, 18=UINT32,
 * 19=UINT64, 20=FLOAT32, 21=FLOAT64, 22=BOOL8. Every fixed-width type is a
 * valid payload column; all but FLOAT32/FLOAT64 are valid key columns (a key
 * pair involving one of 15..22 must have identical type ids on both sides).
 * data is the fixed-width device array (element-aligned), or the
 * int32 offsets[n+1] of a STRING column whose bytes are chars[0..chars_bytes).
 * The descriptor joins/shuffles take key indices that may name STRING
 * columns, alone or among up to 4 key columns (reference: arbitrary
 * left_on/right_on/on_columns forwarded to cudf::hash_partition and
 * cudf::inner_join, distributed_join.cpp:71-132, shuffle_on.cpp:59-60).
 * Placement spec: csrc/dj_hash.h "STRING and composite keys". */
typedef struct {
  int type_id;
  const void* data;
  const void* chars;
  int64_t chars_bytes;
} dj_col_desc;

/* shuffle_on over nc column descriptors of n rows; `on` holds nkeys key
 * column indices. Returns an opaque table (this rank's rows after the
 * shuffle). HASH_IDENTITY with a STRING key column is a loud error. */
void* dj_cpp_shuffle_on_cols(void* comm, const dj_col_desc* cols, int nc, int64_t n,
                             const int32_t* on, int nkeys, int hash_function, uint32_t seed,
                             int compression);
/* test hook: d_out[i] = MurmurHash3_x86_32(bytes of row i, seed) for a
 * STRING column of n rows, through the same kernel (LDS-staged and direct
 * paths) that hashes STRING key columns. Reads no byte outside
 * [d_chars, d_chars + chars_bytes). Synchronizes. */
void dj_hash_strings(const void* d_offsets, const void* d_chars, int64_t chars_bytes, int64_t n,
                     uint32_t seed, uint32_t* d_out);
/* d_out[i] = the 64-bit key a STRING row contributes to the fused key chain
 * (csrc/dj_strhash.h). Runs `reps` launches and writes each launch's
 * hipEvent milliseconds to h_ms (host double[reps]; may be NULL).
 * Synchronizes. */
void dj_string_keys64(const void* d_offsets, const void* d_chars, int64_t chars_bytes,
                      int64_t n, uint64_t* d_out, int reps, double* h_ms);


/* test hook: the placement step of shuffle_on alone — partitions the table
 * into nparts contiguous ranges exactly as shuffle_on does before its
 * all-to-all and writes the nparts+1 row offsets to h_offsets (host). Returns
 * the partitioned table. */
void* dj_cpp_partition_cols(const dj_col_desc* cols, int nc, int64_t n, const int32_t* on,
                            int nkeys, int nparts, int hash_function, uint32_t seed,
                            int64_t* h_offsets);

/* test/bench hook for the table gather kernel: for each of ncols descriptors
 * dst[i] = src[idx[i]] for i in [0, n), elements of `width` bytes (1/2/4/8).
 * mode 0 = the fused width-generic kernel (all columns in one launch, four
 * rows per thread, packed stores; dst must be 16-byte aligned), mode 1 = one
 * one-row-per-thread launch per column, mode 2 = the per-width routing the
 * engine uses. Runs `reps` times, each between a hipEvent pair; h_ms (host
 * double[reps], may be NULL) receives the milliseconds. Synchronizes. */
typedef struct {
  const void* src;
  void* dst;
  int width;
} dj_gather_desc;
void dj_gather_columns(const dj_gather_desc* descs, int ncols, const int64_t* d_idx, int64_t n,
                       int mode, int reps, double* h_ms);

/* ---------------- nullable columns (validity masks, cuDF layout: row i is
 * bit i % 32, LSB first, of uint32 word i / 32; 1 = valid; bits past n and
 * the values under a null row are unspecified). dj_ncol_desc is dj_col_desc
 * plus the mask: null_mask is a device pointer or NULL ("no nulls"),
 * null_count the number of null rows (0 when null_mask is NULL). Null keys
 * join with null_equality::EQUAL (null matches null and no valid key), the
 * default of the cudf::inner_join call the reference makes
 * (distributed_join.cpp:79), unless an entry point takes a null_equality
 * argument (dj_cpp_distributed_join_ncols_multi_ne below); a null key element places on the element hash
 * 0xFFFFFFFF (csrc/dj_hash.h). An output column has a mask exactly when its
 * source column had one. The *_cols entry points above stay mask-free. */
typedef struct {
  int type_id;
  const void* data;
  const void* chars;
  int64_t chars_bytes;
  const void* null_mask;
  int64_t null_count;
} dj_ncol_desc;

/* dj_cpp_distributed_inner_join_cols_multi over nullable descriptors */
void* dj_cpp_distributed_inner_join_ncols_multi(void* comm, const dj_ncol_desc* lcols, int nl,
                                                int64_t ln, const dj_ncol_desc* rcols, int nr,
                                                int64_t rn, const int32_t* lon,
                                                const int32_t* ron, int nkeys, int over_decom,
                                                int report_timing);
/* dj_cpp_shuffle_on_cols over nullable descriptors. The two share one body,
 * so `compression` means here what it means there: 0 none, 1 the fixed
 * bitpack policy, 2 sampling auto-select, 3 an explicit cascaded option on
 * every column (2 and 3 used to act as 1 on this entry point). */
void* dj_cpp_shuffle_on_ncols(void* comm, const dj_ncol_desc* cols, int nc, int64_t n,
                              const int32_t* on, int nkeys, int hash_function, uint32_t seed,
                              int compression);
/* dj_cpp_partition_cols over nullable descriptors */
void* dj_cpp_partition_ncols(const dj_ncol_desc* cols, int nc, int64_t n, const int32_t* on,
                             int nkeys, int nparts, int hash_function, uint32_t seed,
                             int64_t* h_offsets);
/* test hook: the concatenation step of the batched join pipeline alone — the
 * rows of the n >= 1 opaque tables (same schema) back to back; STRING offsets
 * are rebased part by part, masks concatenated (a part without one counts as
 * all valid). Takes ownership of the input tables: free only the result. */
void* dj_cpp_concat_tables(void* const* tables, int n);
/* mask (device pointer, NULL when the column has none) and exact null count
 * of column i of an opaque table */
const void* dj_table_column_null_mask(void* tbl, int i);
int64_t dj_table_column_null_count(void* tbl, int i);

/* test/bench hook for the mask gather kernel: for each of ncols (<= 32)
 * columns, bit i of d_dst_masks[c] = bit d_idx[i] of d_src_masks[c] (all 1
 * when that source is NULL), i in [0, n); destination bits [n, roundup(n, 64))
 * are written 0. h_src_masks / h_dst_masks are HOST arrays of device
 * pointers; each destination is 8-byte aligned and holds roundup(n, 64) / 8
 * bytes. h_null_counts (host int64[ncols]) receives the 0 bits written per
 * column. Runs `reps` times between hipEvent pairs; h_ms (host double[reps],
 * may be NULL) receives the milliseconds. cols_per_launch: how many columns
 * one kernel launch takes (1..32), 0 = what the engine uses. Synchronizes. */
void dj_gather_bitmasks(const void* const* h_src_masks, void* const* h_dst_masks, int ncols,
                        const int64_t* d_idx, int64_t n, int64_t* h_null_counts, int reps,
                        double* h_ms, int cols_per_launch);
/* test hook for the mask segment copy kernel: S bit ranges (host arrays:
 * device source mask or NULL = all valid, first source bit, length in bits)
 * land back to back in d_dst, whose ceil(total / 32) words are written whole
 * with the bits past the total as 0. Returns the number of 0 bits among the
 * total (through the null-count kernel). Synchronizes. */
int64_t dj_copy_bitmask_segments(const void* const* h_src_masks, const int64_t* h_src_bits,
                                 const int64_t* h_nbits, int S, void* d_dst);

/* ---------------- left / left semi / left anti joins.
 * dj_cpp_distributed_inner_join_ncols_multi with a join kind after comm:
 * 0 = INNER (forwards to the inner join), 1 = LEFT, 2 = LEFT_SEMI,
 * 3 = LEFT_ANTI (join_kind of include/distributed_join.hpp, which documents
 * the semantics). LEFT returns left columns then right columns, every
 * right-hand column with a mask; LEFT_SEMI / LEFT_ANTI return the left
 * columns only. */
#define DJ_JOIN_INNER 0
#define DJ_JOIN_LEFT 1
#define DJ_JOIN_LEFT_SEMI 2
#define DJ_JOIN_LEFT_ANTI 3
void* dj_cpp_distributed_join_ncols_multi(void* comm, int kind, const dj_ncol_desc* lcols,
                                          int nl, int64_t ln, const dj_ncol_desc* rcols, int nr,
                                          int64_t rn, const int32_t* lon, const int32_t* ron,
                                          int nkeys, int over_decom, int report_timing);

/* dj_cpp_distributed_join_ncols_multi with the null equality of the key
 * comparison after kind: DJ_NULL_EQUAL, the rule of every other entry point,
 * or DJ_NULL_UNEQUAL, SQL's, under which a row with a null in any column of
 * its key tuple matches nothing (include/distributed_join.hpp documents what
 * each kind then returns). Any other value raises. */
#define DJ_NULL_EQUAL 0
#define DJ_NULL_UNEQUAL 1
void* dj_cpp_distributed_join_ncols_multi_ne(void* comm, int kind, int null_equality,
                                             const dj_ncol_desc* lcols, int nl, int64_t ln,
                                             const dj_ncol_desc* rcols, int nr, int64_t rn,
                                             const int32_t* lon, const int32_t* ron, int nkeys,
                                             int over_decom, int report_timing);

/* test/bench hook for the row-marking kernel: sets bit d_idx[i] (row i = bit
 * i % 32 of uint32 word i / 32) of d_bits for every i < n. The caller zeroes
 * d_bits and keeps every index inside it; an index may repeat any number of
 * times. Only words that hold a marked bit are written. mode: -1 = what the
 * engine runs, else bit 0 = merge lanes naming one word before the atomic,
 * bit 1 = load the word and skip the atomic when no bit is new (0..3, for
 * the benchmark's ablation). Runs `reps` times between hipEvent pairs (the
 * bitmap is NOT re-zeroed in between: repetitions after the first find every
 * bit set); h_ms (host double[reps], may be NULL) receives the milliseconds.
 * Synchronizes. */
void dj_mark_rows(const int64_t* d_idx, int64_t n, void* d_bits, int mode, int reps,
                  double* h_ms);
/* test/bench hook for the row-selection kernels: writes to d_out_idx, in
 * ascending order, the i < nrows whose bit of d_bits equals want_set (bits at
 * and past nrows are ignored) and returns their number. d_out_idx holds at
 * least that many int64 (nrows always suffices). Runs `reps` times between
 * hipEvent pairs; h_ms as above. Synchronizes. */
int64_t dj_select_rows(const void* d_bits, int64_t nrows, int want_set, int64_t* d_out_idx,
                       int reps, double* h_ms);
/* test/bench hook for the keyed compaction: dj_select_rows with want_set = 1
 * that also writes d_out_keys[k] = d_keys[d_out_idx[k]]. d_keys holds nrows
 * int64, both outputs at least as many as are selected. Returns their
 * number; reps and h_ms as above. Synchronizes. */
int64_t dj_compact_keyed_rows(const void* d_bits, int64_t nrows, const int64_t* d_keys,
                              int64_t* d_out_idx, int64_t* d_out_keys, int reps, double* h_ms);
/* test/bench hook for the row validity of a key tuple: word w of d_out
 * (ceil(nrows / 32) uint32 words, each written once) = the AND of word w of
 * the nmasks (1..4) masks in the HOST array h_masks, a NULL entry counting
 * as all ones; bits at and past nrows are written as 0 whatever the sources
 * hold there. Returns the number of 0 bits among the first nrows.
 * Synchronizes. */
int64_t dj_key_row_validity(const void* const* h_masks, int nmasks, int64_t nrows, void* d_out);
/* rows one block of dj_select_rows ranks at a time */
int64_t dj_select_rows_tile_rows(void);

/* ---------------- test hook: spans of the capped-grid helper kernels.
 * Every helper kernel outside the bucket-join core is launched on a grid
 * capped at a few thousand blocks and covers the rest of its input in further
 * trips of a grid-stride loop; the scans behind them turn per-tile partials
 * into offsets in one block, in passes. For a kernel family, *trip_items is
 * the number of items (the unit named below) one full grid covers in one
 * trip and *scan_pass_items the number of items one pass of the single-block
 * scan covers (0: the family has no such scan). Both are computed from the
 * constants the launchers use, so tests that size their inputs from them
 * follow a changed cap. Returns 0, or -1 for an unknown family. */
#define DJ_SPAN_MASK_GATHER 0    /* gather_bitmasks: rows */
#define DJ_SPAN_MASK_WORDS 1     /* copy_bitmask_segments, count_unset_bits,
                                    key_row_validity: 32-bit words */
#define DJ_SPAN_MARK_ROWS 2      /* mark_rows: indices */
#define DJ_SPAN_SELECT_ROWS 3    /* select_rows, compact_keyed_rows: rows; scan: tile_scan
                                    with a chunk of 1 */
#define DJ_SPAN_GATHER_FUSED 4   /* table gather, fused kernel: rows */
#define DJ_SPAN_GATHER_COLUMN 5  /* table gather, per-column kernel: rows */
#define DJ_SPAN_STRING_ROWS 6    /* sizes_from_offsets, gather_sizes_starts,
                                    gather_chars_from_starts, tuple filter: rows */
#define DJ_SPAN_STRING_SUM 7     /* sum_sizes_i64: rows */
#define DJ_SPAN_STRING_SCAN 8    /* offsets_from_sizes: rows */
#define DJ_SPAN_STRING_HASH 9    /* hash_strings: rows */
#define DJ_SPAN_CODEC_ELEMS 10   /* cascaded codec element loops: elements; scan:
                                    values of its chunked int64 scan */
#define DJ_SPAN_CODEC_PACK 11    /* cascaded codec pack loops: values (32 a group) */
#define DJ_SPAN_KEY_HELPERS 12   /* widen_key, narrow_key, fuse_keys,
                                    nullable_key_hash, rebase_offsets: rows */
#define DJ_SPAN_FAMILIES 13
int dj_grid_span(int family, int64_t* trip_items, int64_t* scan_pass_items);

#ifdef __cplusplus
}
#endif

#endif /* DISTRIBUTED_JOIN_H */
