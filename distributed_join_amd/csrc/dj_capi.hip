/*
 * dj_capi.hip — C-ABI implementation (see include/distributed_join.h for the
 * contract and the reference interfaces each entry point replaces).
 */
#include "dj_error.hpp"
#include "dj_kernels.hpp"
#include "dj_timing.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/distributed_join.h"

namespace {

hipStream_t g_stream = nullptr;       // compute stream
hipStream_t g_comm_stream = nullptr;  // communication stream (xGMI overlap)

hipStream_t stream()
{
  if (!g_stream) DJ_HIP_CALL(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
  return g_stream;
}

hipStream_t comm_stream()
{
  if (!g_comm_stream) DJ_HIP_CALL(hipStreamCreateWithFlags(&g_comm_stream, hipStreamNonBlocking));
  return g_comm_stream;
}

/* ------------- phase timing registry (hipEvent pairs per launch) ------------- */

bool g_timing_on = false;

struct TimedSpan {
  int phase;
  hipEvent_t start, stop;
};
std::vector<TimedSpan> g_spans;
std::vector<hipEvent_t> g_event_pool;  // hipEventCreate costs ~10-20 us;
                                       // per-phase-per-step creation showed
                                       // up in the step time — reuse

hipEvent_t timing_event()
{
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  DJ_HIP_CALL(hipEventCreate(&e));
  return e;
}

using PhaseScope = dj_timing::Scope;

/* ------------- RCCL communicator state ------------- */

ncclComm_t g_comm = nullptr;
int g_rank = 0;
int g_size = 1;

}  // namespace

namespace dj_timing {

bool enabled() { return g_timing_on; }

void record_begin(int phase, hipStream_t s)
{
  TimedSpan t;
  t.phase = phase;
  t.start = timing_event();
  t.stop = timing_event();
  DJ_HIP_CALL(hipEventRecord(t.start, s));
  g_spans.push_back(t);
}

void record_end(hipStream_t s) { DJ_HIP_CALL(hipEventRecord(g_spans.back().stop, s)); }

}  // namespace dj_timing

/* streams shared with the C++ orchestration layer (dj_host.hpp) */
hipStream_t dj_rt_stream() { return stream(); }
hipStream_t dj_rt_comm_stream() { return comm_stream(); }

extern "C" {

/* ---------------- device & memory ---------------- */

int dj_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void dj_set_device(int device) { DJ_HIP_CALL(hipSetDevice(device)); }

void* dj_dmalloc(int64_t bytes)
{
  void* p = nullptr;
  DJ_HIP_CALL(hipMalloc(&p, (size_t)bytes));
  return p;
}

void dj_dfree(void* ptr)
{
  if (ptr) DJ_HIP_CALL(hipFree(ptr));
}

void dj_memcpy_h2d(void* d_dst, const void* h_src, int64_t bytes)
{
  DJ_HIP_CALL(hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, stream()));
  DJ_HIP_CALL(hipStreamSynchronize(stream()));
}

void dj_memcpy_d2h(void* h_dst, const void* d_src, int64_t bytes)
{
  DJ_HIP_CALL(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, stream()));
  DJ_HIP_CALL(hipStreamSynchronize(stream()));
}

void dj_memcpy_d2d(void* d_dst, const void* d_src, int64_t bytes)
{
  DJ_HIP_CALL(hipMemcpyAsync(d_dst, d_src, (size_t)bytes, hipMemcpyDeviceToDevice, stream()));
}

void dj_sync(void)
{
  DJ_HIP_CALL(hipStreamSynchronize(stream()));
  if (g_comm_stream) DJ_HIP_CALL(hipStreamSynchronize(g_comm_stream));
}

/* ---------------- generator ---------------- */

void dj_generate_build(int64_t* d_keys, int64_t* d_pay, int64_t n_global, int64_t rand_max,
                       uint64_t seed, int uniq, int64_t row0, int64_t nrows)
{
  PhaseScope t(DJ_PHASE_GENERATE, stream());
  dj::generate_build(d_keys, d_pay, n_global, rand_max, seed, uniq != 0, row0, nrows, stream());
}

void dj_generate_probe(int64_t* d_keys, int64_t* d_pay, int64_t build_n_global,
                       int64_t rand_max, double selectivity, uint64_t seed, int64_t row0,
                       int64_t nrows)
{
  PhaseScope t(DJ_PHASE_GENERATE, stream());
  dj::generate_probe(d_keys, d_pay, build_n_global, rand_max, selectivity, seed, row0, nrows,
                     stream());
}

/* ---------------- partition ---------------- */

int64_t dj_partition_scratch_bytes(int64_t n, int nparts)
{
  return (int64_t)dj::hash_partition_scratch_bytes(n, nparts);
}

void dj_hash_partition(const int64_t* d_keys, const int64_t* d_pay, int64_t n, int nparts,
                       int hash_fn, uint32_t hash_seed, int64_t* d_out_keys,
                       int64_t* d_out_pay, int64_t* h_offsets, void* d_scratch)
{
  static int64_t* d_offsets = nullptr;
  static int d_offsets_cap = 0;
  if (nparts + 1 > d_offsets_cap) {
    if (d_offsets) DJ_HIP_CALL(hipFree(d_offsets));
    DJ_HIP_CALL(hipMalloc(&d_offsets, (size_t)(nparts + 1) * sizeof(int64_t)));
    d_offsets_cap = nparts + 1;
  }
  {
    PhaseScope t(DJ_PHASE_PART_COUNT, stream());
    dj::partition_count(d_keys, n, nparts, hash_fn, hash_seed, d_scratch, stream());
  }
  {
    PhaseScope t(DJ_PHASE_PART_SCAN, stream());
    dj::partition_scan(n, nparts, d_scratch, d_offsets, stream());
  }
  {
    PhaseScope t(DJ_PHASE_PART_SCATTER, stream());
    dj::partition_scatter(d_keys, d_pay, n, nparts, hash_fn, hash_seed, d_offsets, d_scratch,
                          d_out_keys, d_out_pay, stream());
  }
  if (h_offsets) {
    DJ_HIP_CALL(hipMemcpyAsync(h_offsets, d_offsets, (size_t)(nparts + 1) * sizeof(int64_t),
                               hipMemcpyDeviceToHost, stream()));
    DJ_HIP_CALL(hipStreamSynchronize(stream()));
  }
}

/* ---------------- local join ---------------- */

int64_t dj_join_table_slots(int64_t ln) { return dj::join_table_slots(ln); }

void dj_join_table_init(int64_t* d_table, int64_t nslots)
{
  PhaseScope t(DJ_PHASE_TABLE_INIT, stream());
  dj::join_table_init(d_table, nslots, stream());
}

void dj_join_build(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                   int64_t* d_table, int64_t nslots, int* d_error)
{
  PhaseScope t(DJ_PHASE_BUILD, stream());
  dj::join_build(d_lk, d_lp, ln, d_table, nslots, d_error, stream());
}

void dj_join_probe(const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                   const int64_t* d_table, int64_t nslots,
                   int64_t* d_out0, int64_t* d_out1, int64_t* d_out2, int64_t* d_out3,
                   int64_t cap, int64_t* d_counter)
{
  PhaseScope t(DJ_PHASE_PROBE, stream());
  dj::join_probe(d_rk, d_rp, rn, d_table, nslots, d_out0, d_out1, d_out2,
                 d_out3, cap, d_counter, stream());
}

int64_t dj_read_counter_i64(const int64_t* d_counter)
{
  int64_t v = 0;
  dj_memcpy_d2h(&v, d_counter, sizeof(int64_t));
  return v;
}

int dj_read_error_i32(const int* d_error)
{
  int v = 0;
  dj_memcpy_d2h(&v, d_error, sizeof(int));
  return v;
}

int64_t dj_local_inner_join(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                            const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                            int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                            int64_t* d_out3, int64_t cap)
{
  if (ln == 0 || rn == 0) return 0;  // empty side => empty (distributed_join.cpp:76-83)
  void* d_scratch = dj_dmalloc(dj_bucket_join_scratch_bytes(ln, rn));
  int* d_error = (int*)dj_dmalloc(sizeof(int));
  int64_t* d_counter = (int64_t*)dj_dmalloc(sizeof(int64_t));
  DJ_HIP_CALL(hipMemsetAsync(d_error, 0, sizeof(int), stream()));
  DJ_HIP_CALL(hipMemsetAsync(d_counter, 0, sizeof(int64_t), stream()));
  dj_bucket_local_join(d_lk, d_lp, ln, d_rk, d_rp, rn, d_out0, d_out1, d_out2, d_out3, cap,
                       d_counter, d_error, d_scratch);
  int64_t n = dj_read_counter_i64(d_counter);
  DJ_CHECK_ERROR(dj_read_error_i32(d_error) == 0,
                 "dj build: key equal to the empty sentinel (-1) is unsupported");
  dj_dfree(d_scratch);
  dj_dfree(d_error);
  dj_dfree(d_counter);
  return n;
}

/* ---------------- bucketed LDS local join ---------------- */

namespace {

/* round-2 local join uses the count-free slack bucket layout (pass B writes
 * bucket b at b*capB with length lens[b] — bucket_partition2_slack_pair) whenever
 * its u32 row indices fit; otherwise the exact compact path. */
bool bucket_slack_mode(int64_t ln, int64_t rn, int B)
{
  const int PA = dj::bucket_groups_for(B);
  if (PA < 2) return false;
  const int64_t maxn = ln > rn ? ln : rn;
  if (maxn >= (int64_t)UINT32_MAX) return false;
  if ((int64_t)PA * dj::slack_capA(maxn, PA) + maxn >= (int64_t)UINT32_MAX) return false;
  if ((int64_t)B * dj::slack_capB(ln, B) >= (int64_t)UINT32_MAX) return false;
  if ((int64_t)B * dj::slack_capB(rn, B) >= (int64_t)UINT32_MAX) return false;
  return true;
}

struct BucketScratch {
  longlong2 *lpairs, *rpairs;  // bucketed {key,payload} pairs (final; slack
                               // layout B*capB when bucket_slack_mode)
  longlong2* tmp_pairs;        // pass-A staging (size max(ln,rn))
  longlong2* tmp_pairs2;       // second table's pass-A staging (slack mode)
  int64_t *loff, *roff;        // int64[B+1] (compact mode)
  uint32_t *llen, *rlen;       // u32[B] (slack mode)
  int64_t* segoff;             // int64[PA+1]
  uint32_t* counts;            // u32[kBucketBlocks*PA]
  uint32_t* totals;            // u32[PA] (also the slack pass-A cursors)
  uint32_t* flags;             // u32[B]
  int* any_overflow;           // int[1]
};

/* THE list of the bucket join's scratch allocations, each rounded up to 256
 * bytes: carves them from `base` and returns how many bytes they span. A
 * null base only measures (the pointers come out null). */
static size_t bucket_scratch_layout(void* base, int64_t ln, int64_t rn, int B, BucketScratch& s)
{
  const int PA = dj::bucket_groups_for(B);
  const int64_t maxn = ln > rn ? ln : rn;
  const bool slack = bucket_slack_mode(ln, rn, B);
  const size_t lrows = slack ? (size_t)B * dj::slack_capB(ln, B) : (size_t)ln;
  const size_t rrows = slack ? (size_t)B * dj::slack_capB(rn, B) : (size_t)rn;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* r = base ? (char*)base + off : nullptr;
    off += (bytes + 255) & ~(size_t)255;
    return r;
  };
  s.lpairs = (longlong2*)take(lrows * 16);
  s.rpairs = (longlong2*)take(rrows * 16);
  s.tmp_pairs = (longlong2*)take((size_t)(PA * dj::slack_capA(maxn, PA)) * 16);  // >= maxn
  s.tmp_pairs2 = slack ? (longlong2*)take((size_t)(PA * dj::slack_capA(maxn, PA)) * 16)
                       : nullptr;  // pair-launch partition needs both live
  s.loff = (int64_t*)take((size_t)(B + 1) * 8);
  s.roff = (int64_t*)take((size_t)(B + 1) * 8);
  const size_t Bpad = ((size_t)B + 3) & ~(size_t)3;  // lds_join_slack KBUK pad
  s.llen = (uint32_t*)take(Bpad * 4);
  s.rlen = (uint32_t*)take(Bpad * 4);
  s.segoff = (int64_t*)take((size_t)(PA + 1) * 8);
  s.counts = (uint32_t*)take((size_t)dj::kBucketBlocks * PA * 4);
  s.totals = (uint32_t*)take((size_t)PA * 4);
  s.flags = (uint32_t*)take((size_t)B * 4);
  s.any_overflow = (int*)take(16);
  return off;
}

BucketScratch carve_bucket_scratch(void* base, int64_t ln, int64_t rn, int B)
{
  BucketScratch s;
  bucket_scratch_layout(base, ln, rn, B, s);
  return s;
}

}  // namespace

int64_t dj_bucket_join_scratch_bytes(int64_t ln, int64_t rn)
{
  BucketScratch unused;
  return (int64_t)bucket_scratch_layout(nullptr, ln, rn, dj::bucket_count_for(ln, rn), unused);
}

/* enqueue-only core: all kernels stream-ordered, no host syncs. The skew
 * any-overflow flag is written to d_any_overflow (device int) for the caller
 * to check after its own sync; oversized buckets are SKIPPED by the fused
 * kernel and must be re-joined by the caller (dj_bucket_local_join does this
 * via the global-table path; the pipelined C++ orchestration redoes the
 * whole batch). */
static void bucket_local_join_enqueue_impl(const int64_t* d_lk, const int64_t* d_lp,
                                           int64_t ln, const int64_t* d_rk,
                                           const int64_t* d_rp, int64_t rn, int64_t* d_out0,
                                           int64_t* d_out1, int64_t* d_out2, int64_t* d_out3,
                                           int64_t cap, int64_t* d_counter, int* d_error,
                                           int* d_any_overflow, void* d_scratch,
                                           bool force_compact)
{
  if (ln == 0 || rn == 0) {
    DJ_HIP_CALL(hipMemsetAsync(d_any_overflow, 0, sizeof(int), stream()));
    return;  // empty side => empty (distributed_join.cpp:76-83)
  }
  const int B = dj::bucket_count_for(ln, rn);
  BucketScratch s = carve_bucket_scratch(d_scratch, ln, rn, B);
  hipStream_t st = stream();
  DJ_HIP_CALL(hipMemsetAsync(d_any_overflow, 0, sizeof(int), st));
  DJ_HIP_CALL(hipMemsetAsync(s.flags, 0, (size_t)B * 4, st));
  const int64_t maxn = ln > rn ? ln : rn;
  /* beyond ~400M rows/table the buckets exceed the 2048-slot cap — switch
   * to the 4096-slot table (cap 3072, covers the 800M single-GPU shape)
   * instead of overflowing every bucket into the per-bucket fallback */
  const int slots = (maxn / B > 1300) ? 4096 : 2048;
  if (!force_compact && bucket_slack_mode(ln, rn, B)) {
    const int64_t capBl = dj::slack_capB(ln, B), capBr = dj::slack_capB(rn, B);
    /* pad B to a multiple of 4 with zero-length buckets (the lds_join_slack
     * KBUK contract; carve_bucket_scratch sized llen/rlen for it) */
    const int Bpad = (B + 3) & ~3;
    if (Bpad != B) {
      DJ_HIP_CALL(hipMemsetAsync(s.llen + B, 0, (size_t)(Bpad - B) * 4, st));
      DJ_HIP_CALL(hipMemsetAsync(s.rlen + B, 0, (size_t)(Bpad - B) * 4, st));
    }
    {
      PhaseScope t(DJ_PHASE_BUCKET_SCATTER, st);
      /* both tables in one pass-A and one pass-B launch: the second table's
       * blocks fill the first's tail wave (s.counts is free in slack mode
       * and serves as the second cursor array) */
      dj::bucket_partition2_slack_pair(d_lk, d_lp, ln, s.tmp_pairs, s.totals, capBl,
                                       s.lpairs, s.llen, d_rk, d_rp, rn, s.tmp_pairs2,
                                       s.counts, capBr, s.rpairs, s.rlen, B, d_any_overflow,
                                       st);
    }
    PhaseScope t(DJ_PHASE_JOIN_FUSED, st);
    dj::lds_join_slack(s.lpairs, s.llen, capBl, s.rpairs, s.rlen, capBr, Bpad, slots, d_out0,
                       d_out1, d_out2, d_out3, cap, d_counter, s.flags, d_any_overflow,
                       d_error, st);
    return;
  }
  {
    PhaseScope t(DJ_PHASE_BUCKET_SCATTER, st);
    dj::bucket_partition2(d_lk, d_lp, ln, B, s.tmp_pairs, s.counts, s.totals, s.segoff,
                          s.loff, s.lpairs, d_any_overflow, st);
    dj::bucket_partition2(d_rk, d_rp, rn, B, s.tmp_pairs, s.counts, s.totals, s.segoff,
                          s.roff, s.rpairs, d_any_overflow, st);
  }
  {
    PhaseScope t(DJ_PHASE_JOIN_FUSED, st);
    dj::lds_join(s.lpairs, s.loff, s.rpairs, s.roff, B, slots, d_out0, d_out1, d_out2,
                 d_out3, cap, d_counter, s.flags, d_any_overflow, d_error, st);
  }
}

void dj_bucket_local_join_enqueue(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                                  const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                                  int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                                  int64_t* d_out3, int64_t cap, int64_t* d_counter,
                                  int* d_error, int* d_any_overflow, void* d_scratch)
{
  bucket_local_join_enqueue_impl(d_lk, d_lp, ln, d_rk, d_rp, rn, d_out0, d_out1, d_out2,
                                 d_out3, cap, d_counter, d_error, d_any_overflow, d_scratch,
                                 false);
}

void dj_bucket_local_join(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                          const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                          int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                          int64_t* d_out3, int64_t cap, int64_t* d_counter, int* d_error,
                          void* d_scratch)
{
  if (ln == 0 || rn == 0) return;  // empty side => empty (distributed_join.cpp:76-83)
  const int B = dj::bucket_count_for(ln, rn);
  BucketScratch s = carve_bucket_scratch(d_scratch, ln, rn, B);
  hipStream_t st = stream();
  dj_bucket_local_join_enqueue(d_lk, d_lp, ln, d_rk, d_rp, rn, d_out0, d_out1, d_out2,
                               d_out3, cap, d_counter, d_error, s.any_overflow, d_scratch);
  /* skew fallback: buckets whose build side exceeded the LDS row cap.
   * The sentinel flag rides the same sync (one host round trip per step). */
  int any = 0, saw_neg1 = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&any, s.any_overflow, sizeof(int), hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipMemcpyAsync(&saw_neg1, d_error, sizeof(int), hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  bool used_slack = bucket_slack_mode(ln, rn, B);
  bool retried = false;
  if (any & 2) {
    /* slack overflow (pass-A capA or per-bucket capB blown — duplicate-heavy
     * keys inflate bucket variance beyond the Poisson slack model): the
     * bucketed data is incomplete. First retry with the EXACT counted
     * two-pass partition (compact layout, ~2x the partition cost); only if
     * that also overflows its pass-A slack fall back to the global-table
     * join (the last-resort path — it cost 75 ms/step on the TPC-H shape
     * before this retry existed, gpurun_out/r2_tpch_prof2). */
    DJ_HIP_CALL(hipMemsetAsync(d_counter, 0, sizeof(int64_t), st));
    DJ_HIP_CALL(hipMemsetAsync(d_error, 0, sizeof(int), st));
    bucket_local_join_enqueue_impl(d_lk, d_lp, ln, d_rk, d_rp, rn, d_out0, d_out1, d_out2,
                                   d_out3, cap, d_counter, d_error, s.any_overflow,
                                   d_scratch, true);
    used_slack = false;
    retried = true;
    any = 0;
    DJ_HIP_CALL(hipMemcpyAsync(&any, s.any_overflow, sizeof(int), hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
  }
  /* sentinel (-1) keys: every join path skips them, setting the flag in
   * d_error; join them out-of-band at the end (cross product of the two
   * sides' -1 rows) and clear the flag — legal int64 data, not an error
   * (the reference's cudf::inner_join joins -1 normally). */
  auto neg1_fixup = [&](bool reread) {
    int saw = saw_neg1;
    if (reread) { /* a retry path re-ran the join and may have re-flagged */
      DJ_HIP_CALL(hipMemcpyAsync(&saw, d_error, sizeof(int), hipMemcpyDeviceToHost, st));
      DJ_HIP_CALL(hipStreamSynchronize(st));
    }
    if (saw) {
      DJ_HIP_CALL(hipMemsetAsync(d_error, 0, sizeof(int), st));
      dj::neg1_cross_join(d_lk, d_lp, ln, d_rk, d_rp, rn, d_out0, d_out1, d_out2, d_out3,
                          cap, d_counter, st);
    }
  };
  if (any & 2) {
    /* compact pass-A slack also blown: global-table redo on the inputs */
    DJ_HIP_CALL(hipMemsetAsync(d_counter, 0, sizeof(int64_t), st));
    DJ_HIP_CALL(hipMemsetAsync(d_error, 0, sizeof(int), st));
    int64_t nslots = dj::join_table_slots(ln);
    int64_t* d_table = (int64_t*)dj_dmalloc(nslots * 2 * sizeof(int64_t));
    dj_join_table_init(d_table, nslots);
    dj_join_build(d_lk, d_lp, ln, d_table, nslots, d_error);
    dj_join_probe(d_rk, d_rp, rn, d_table, nslots, d_out0, d_out1, d_out2, d_out3, cap,
                  d_counter);
    DJ_HIP_CALL(hipStreamSynchronize(st));
    dj_dfree(d_table);
    neg1_fixup(true);
    return;
  }
  if (any) {
    const bool slack = used_slack;
    const int64_t capBl = slack ? dj::slack_capB(ln, B) : 0;
    const int64_t capBr = slack ? dj::slack_capB(rn, B) : 0;
    std::vector<uint32_t> flags((size_t)B);
    std::vector<int64_t> loff((size_t)B + 1), roff((size_t)B + 1);
    std::vector<uint32_t> llen, rlen;
    DJ_HIP_CALL(hipMemcpy(flags.data(), s.flags, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (slack) {
      llen.resize((size_t)B);
      rlen.resize((size_t)B);
      DJ_HIP_CALL(hipMemcpy(llen.data(), s.llen, (size_t)B * 4, hipMemcpyDeviceToHost));
      DJ_HIP_CALL(hipMemcpy(rlen.data(), s.rlen, (size_t)B * 4, hipMemcpyDeviceToHost));
    } else {
      DJ_HIP_CALL(hipMemcpy(loff.data(), s.loff, ((size_t)B + 1) * 8, hipMemcpyDeviceToHost));
      DJ_HIP_CALL(hipMemcpy(roff.data(), s.roff, ((size_t)B + 1) * 8, hipMemcpyDeviceToHost));
    }
    for (int b = 0; b < B; b++) {
      if (!flags[b]) continue;
      int64_t l0 = slack ? (int64_t)b * capBl : loff[b];
      int64_t r0 = slack ? (int64_t)b * capBr : roff[b];
      int64_t lnb = slack ? (int64_t)llen[b] : loff[b + 1] - loff[b];
      int64_t rnb = slack ? (int64_t)rlen[b] : roff[b + 1] - roff[b];
      if (lnb == 0 || rnb == 0) continue;
      int64_t nslots = dj::join_table_slots(lnb);
      int64_t* d_table = (int64_t*)dj_dmalloc(nslots * 2 * sizeof(int64_t));
      dj_join_table_init(d_table, nslots);
      dj::join_build_pairs(s.lpairs + l0, lnb, d_table, nslots, d_error, st);
      dj::join_probe_pairs(s.rpairs + r0, rnb, d_table, nslots, d_out0, d_out1, d_out2,
                           d_out3, cap, d_counter, st);
      DJ_HIP_CALL(hipStreamSynchronize(st));
      dj_dfree(d_table);
    }
  }
  /* the per-bucket fallback above is the only place a skew-flagged bucket's
   * -1 rows are seen (join_build_pairs flags them): the snapshot taken
   * before it is stale whenever it ran */
  neg1_fixup(retried || any != 0);
}

int64_t dj_local_inner_join_global(const int64_t* d_lk, const int64_t* d_lp, int64_t ln,
                                   const int64_t* d_rk, const int64_t* d_rp, int64_t rn,
                                   int64_t* d_out0, int64_t* d_out1, int64_t* d_out2,
                                   int64_t* d_out3, int64_t cap)
{
  if (ln == 0 || rn == 0) return 0;
  int64_t nslots = dj::join_table_slots(ln);
  int64_t* d_table = (int64_t*)dj_dmalloc(nslots * 2 * sizeof(int64_t));
  int* d_error = (int*)dj_dmalloc(sizeof(int));
  int64_t* d_counter = (int64_t*)dj_dmalloc(sizeof(int64_t));
  DJ_HIP_CALL(hipMemsetAsync(d_error, 0, sizeof(int), stream()));
  DJ_HIP_CALL(hipMemsetAsync(d_counter, 0, sizeof(int64_t), stream()));
  dj_join_table_init(d_table, nslots);
  dj_join_build(d_lk, d_lp, ln, d_table, nslots, d_error);
  dj_join_probe(d_rk, d_rp, rn, d_table, nslots, d_out0, d_out1, d_out2, d_out3, cap,
                d_counter);
  int64_t n = dj_read_counter_i64(d_counter);
  DJ_CHECK_ERROR(dj_read_error_i32(d_error) == 0,
                 "dj_join_build: key equal to the empty sentinel (-1) is unsupported");
  dj_dfree(d_table);
  dj_dfree(d_error);
  dj_dfree(d_counter);
  return n;
}

/* ---------------- timing ---------------- */

void dj_timing_enable(int on) { g_timing_on = on != 0; }

void dj_timing_reset(void)
{
  for (auto& t : g_spans) {
    g_event_pool.push_back(t.start);
    g_event_pool.push_back(t.stop);
  }
  g_spans.clear();
}

double dj_timing_total_ms(int phase)
{
  dj_sync();
  double total = 0;
  for (auto& t : g_spans) {
    if (t.phase != phase) continue;
    float ms = 0;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, t.start, t.stop));
    total += ms;
  }
  return total;
}

int64_t dj_timing_launches(int phase)
{
  int64_t n = 0;
  for (auto& t : g_spans)
    if (t.phase == phase) n++;
  return n;
}

/* ---------------- RCCL communicator ---------------- */

int dj_rccl_unique_id_bytes(void) { return (int)sizeof(ncclUniqueId); }

void dj_rccl_get_unique_id(void* h_id_bytes)
{
  ncclUniqueId id;
  DJ_RCCL_CALL(ncclGetUniqueId(&id));
  memcpy(h_id_bytes, &id, sizeof(id));
}

void dj_comm_init(int rank, int size, const void* h_id_bytes)
{
  ncclUniqueId id;
  memcpy(&id, h_id_bytes, sizeof(id));
  DJ_RCCL_CALL(ncclCommInitRank(&g_comm, size, id, rank));
  g_rank = rank;
  g_size = size;
}

void dj_comm_finalize(void)
{
  if (g_comm) {
    DJ_RCCL_CALL(ncclCommDestroy(g_comm));
    g_comm = nullptr;
  }
}

int dj_comm_rank(void) { return g_rank; }
int dj_comm_size(void) { return g_size; }

void dj_all_to_all_i64(const int64_t* d_send, const int64_t* h_send_offsets, int64_t* d_recv,
                       const int64_t* h_recv_offsets)
{
  DJ_CHECK_ERROR(g_comm != nullptr, "dj_all_to_all_i64: communicator not initialized");
  hipStream_t cs = comm_stream();
  PhaseScope t(DJ_PHASE_COMM, cs);
  /* reference pattern: grouped per-peer send/recv of contiguous slices
   * (all_to_all_comm.cpp:126-189); self-partition via explicit D2D copy
   * (all_to_all_comm.cpp:610-653,710-726). Over xGMI each peer slice moves
   * on its own point-to-point link, so pairwise grouped send/recv is the
   * bandwidth-optimal all-to-all (no staging, no registration). */
  DJ_RCCL_CALL(ncclGroupStart());
  for (int p = 0; p < g_size; p++) {
    if (p == g_rank) continue;
    int64_t scount = h_send_offsets[p + 1] - h_send_offsets[p];
    int64_t rcount = h_recv_offsets[p + 1] - h_recv_offsets[p];
    if (scount > 0)
      DJ_RCCL_CALL(ncclSend(d_send + h_send_offsets[p], (size_t)scount, ncclInt64, p, g_comm, cs));
    if (rcount > 0)
      DJ_RCCL_CALL(ncclRecv(d_recv + h_recv_offsets[p], (size_t)rcount, ncclInt64, p, g_comm, cs));
  }
  DJ_RCCL_CALL(ncclGroupEnd());
  int64_t self_count = h_send_offsets[g_rank + 1] - h_send_offsets[g_rank];
  if (self_count > 0) {
    DJ_HIP_CALL(hipMemcpyAsync(d_recv + h_recv_offsets[g_rank],
                               d_send + h_send_offsets[g_rank],
                               (size_t)self_count * sizeof(int64_t), hipMemcpyDeviceToDevice,
                               cs));
  }
  DJ_HIP_CALL(hipStreamSynchronize(cs));  // launch_communication blocks the host
                                          // (all_to_all_comm.hpp:331 contract)
}

void dj_exchange_sizes(const int64_t* h_send_counts, int64_t* h_recv_counts)
{
  DJ_CHECK_ERROR(g_comm != nullptr, "dj_exchange_sizes: communicator not initialized");
  /* replaces communicate_sizes (all_to_all_comm.cpp:54-100): allgather the
   * G x G count matrix, read our column. Tiny (G*G*8 B). */
  hipStream_t cs = comm_stream();
  int64_t* d_mine = (int64_t*)dj_dmalloc((int64_t)g_size * sizeof(int64_t));
  int64_t* d_all = (int64_t*)dj_dmalloc((int64_t)g_size * g_size * sizeof(int64_t));
  DJ_HIP_CALL(hipMemcpyAsync(d_mine, h_send_counts, (size_t)g_size * sizeof(int64_t),
                             hipMemcpyHostToDevice, cs));
  DJ_RCCL_CALL(ncclAllGather(d_mine, d_all, (size_t)g_size, ncclInt64, g_comm, cs));
  std::vector<int64_t> all((size_t)g_size * g_size);
  DJ_HIP_CALL(hipMemcpyAsync(all.data(), d_all, all.size() * sizeof(int64_t),
                             hipMemcpyDeviceToHost, cs));
  DJ_HIP_CALL(hipStreamSynchronize(cs));
  for (int p = 0; p < g_size; p++) h_recv_counts[p] = all[(size_t)p * g_size + g_rank];
  dj_dfree(d_mine);
  dj_dfree(d_all);
}

/* cascaded codec roundtrip (test hook): compress d_in (count elements of
 * elem_size 4/8) with the given cascaded passes, decompress into d_out, and
 * return the wire size in bytes (header included). Pins the codec's
 * compressed == uncompressed semantics per scheme (the reference pins
 * nvcomp only through end-to-end equality, compare_against_analytical
 * runs with compression; our wire format is parity-unpinned). */
int64_t dj_compress_roundtrip(const void* d_in, int64_t count, int elem_size, int num_rles,
                              int num_deltas, int use_bp, void* d_out)
{
  hipStream_t st = stream();
  void* comp = dj_dmalloc((int64_t)dj::compress_bound(count, elem_size));
  void* scratch = dj_dmalloc((int64_t)dj::compress_scratch_bytes(count));
  dj::compress_slice_async(d_in, count, elem_size, num_rles, num_deltas, use_bp,
                           (uint8_t*)comp, scratch, st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  dj::CompSliceHeader h;
  DJ_HIP_CALL(hipMemcpy(&h, comp, sizeof(h), hipMemcpyDeviceToHost));
  int64_t wire = (int64_t)dj::compressed_size_from_header(h, elem_size);
  dj::decompress_slice_async((const uint8_t*)comp, h, elem_size, d_out, scratch, st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  dj_dfree(comp);
  dj_dfree(scratch);
  return wire;
}

/* test hook: spans of the capped-grid helper kernels (include/distributed_join.h).
 * Every file answers for its own families from its launchers' constants. */
int dj_grid_span(int family, int64_t* trip_items, int64_t* scan_pass_items)
{
  static_assert(DJ_SPAN_MASK_GATHER == dj::kSpanMaskGather &&
                  DJ_SPAN_MASK_WORDS == dj::kSpanMaskWords &&
                  DJ_SPAN_MARK_ROWS == dj::kSpanMarkRows &&
                  DJ_SPAN_SELECT_ROWS == dj::kSpanSelectRows &&
                  DJ_SPAN_GATHER_FUSED == dj::kSpanGatherFused &&
                  DJ_SPAN_GATHER_COLUMN == dj::kSpanGatherColumn &&
                  DJ_SPAN_STRING_ROWS == dj::kSpanStringRows &&
                  DJ_SPAN_STRING_SUM == dj::kSpanStringSum &&
                  DJ_SPAN_STRING_SCAN == dj::kSpanStringScan &&
                  DJ_SPAN_STRING_HASH == dj::kSpanStringHash &&
                  DJ_SPAN_CODEC_ELEMS == dj::kSpanCodecElems &&
                  DJ_SPAN_CODEC_PACK == dj::kSpanCodecPack &&
                  DJ_SPAN_KEY_HELPERS == dj::kSpanKeyHelpers &&
                  DJ_SPAN_FAMILIES == dj::kSpanFamilies,
                "DJ_SPAN_* of the C ABI and kSpan* of dj_kernels.hpp are one list");
  const dj::GridSpan all[] = {dj::bitmask_grid_span(family),  dj::rowset_grid_span(family),
                              dj::gather_grid_span(family),   dj::strings_grid_span(family),
                              dj::compress_grid_span(family), dj::key_helper_grid_span(family)};
  dj::GridSpan span{0, 0};
  for (const dj::GridSpan& s : all)
    if (s.trip > 0) span = s;
  if (span.trip <= 0) return -1;
  *trip_items = span.trip;
  *scan_pass_items = span.scan_pass;
  return 0;
}

}  // extern "C"
