/*
 * dj_strings.hip — gfx950 kernels for the strings-column path of the
 * distributed join (BASELINE config 4). MI355X-native equivalents of the
 * reference's thrust-based helpers (SURVEY.md §2 row "String column
 * support"):
 *   - sizes_from_offsets  <- calculate_string_sizes_from_offsets
 *                            (strings_column.cu:81-109, adjacent difference)
 *   - offsets_from_sizes  <- calculate_string_offsets_from_sizes
 *                            (strings_column.cu:111-131, inclusive scan with
 *                            offset[0] = 0 — sizes, not offsets, go on the
 *                            wire; receiver rebuilds offsets)
 *   - gather_sizes/gather_strings <- thrust::gather of per-partition char
 *                            offsets (strings_column.cu:39-79) generalized to
 *                            a row permutation (used by partition & join
 *                            output assembly)
 *   - make_test_string_sizes/fill_test_strings <- the deterministic string
 *                            payload of test/string_payload.cu:50-94
 *                            (len = k%7+1, char = 'a'+k%26)
 * String offsets are int32 (cudf convention; chars per column < 2^31 — the
 * reference shares this bound).
 */
#include "dj_error.hpp"
#include "dj_kernels.hpp"
#include "dj_strhash.h"

#include <hip/hip_runtime.h>

#include <cstdlib>

namespace dj {

namespace {
constexpr int SBLOCK = 256;
constexpr int SVPT = 8;  // elements per thread in the scan partials pass
constexpr int CHUNK = SBLOCK * SVPT;
/* blocks per launch at most; grid-stride loops cover the rest */
constexpr int SGRID_CAP = 2048;      // row loops and the scan's tile loops
constexpr int SUM_GRID_CAP = 1024;   // sum_sizes_i64
constexpr int HS_GRID_CAP = 4096;    // hash_strings
constexpr int SCAN_PASS = 1024;      // partials one pass of the single-block scan takes

int sgrid(int64_t n)
{
  int64_t b = (n + SBLOCK - 1) / SBLOCK;
  if (b > SGRID_CAP) b = SGRID_CAP;
  if (b < 1) b = 1;
  return (int)b;
}
}  // namespace

__global__ void sizes_from_offsets_kernel(const int32_t* __restrict__ offsets, int64_t n,
                                          int32_t* __restrict__ sizes)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) sizes[i] = offsets[i + 1] - offsets[i];
}

__global__ void sum_sizes_i64_kernel(const int32_t* __restrict__ sizes, int64_t n,
                                     int64_t* __restrict__ total)
{
  __shared__ int64_t red[256];
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t acc = 0;
  for (; i < n; i += stride) acc += sizes[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < (unsigned)off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd((unsigned long long*)total, (unsigned long long)red[0]);
}

void sum_sizes_i64(const int32_t* d_sizes, int64_t n, int64_t* d_total, hipStream_t s)
{
  int64_t b = (n + 255) / 256;
  if (b > SUM_GRID_CAP) b = SUM_GRID_CAP;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(sum_sizes_i64_kernel, dim3((uint32_t)b), dim3(256), 0, s, d_sizes, n,
                     d_total);
  DJ_HIP_CALL(hipGetLastError());
}

void sizes_from_offsets(const int32_t* d_offsets, int64_t n, int32_t* d_sizes, hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(sizes_from_offsets_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s, d_offsets,
                     n, d_sizes);
  DJ_HIP_CALL(hipGetLastError());
}

/* ---- exclusive scan of int32 sizes -> int32 offsets[n+1], offsets[0]=0 ----
 * Tile-coalesced: a block owns a 4096-element tile; loads/stores are
 * lane-contiguous, the per-thread serial work happens in LDS. (The first
 * version gave each THREAD a serial chunk — lane-adjacent addresses 8 KB
 * apart, 64 lines per load instruction: the scan alone cost 5 ms of the
 * TPC-H step, gpurun_out/r2_tpch_prof3.) Whole-column totals stay < 2^31
 * (the int32 offsets cap, enforced upstream), so in-tile prefixes fit i32. */

constexpr int SCAN_T = 4096;             // elements per block tile (16 KiB LDS)
constexpr int SSEG = SCAN_T / SBLOCK;    // serial segment per thread (16)

__global__ void scan_tile_partials_kernel(const int32_t* __restrict__ sizes, int64_t n,
                                          int64_t ntiles, int64_t* __restrict__ partials)
{
  __shared__ int64_t red[SBLOCK];
  for (int64_t c = blockIdx.x; c < ntiles; c += gridDim.x) {
    const int64_t base = c * SCAN_T;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < SSEG; k++) {
      int64_t i = base + (int64_t)k * SBLOCK + threadIdx.x;
      if (i < n) acc += sizes[i];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = SBLOCK / 2; off > 0; off >>= 1) {
      if (threadIdx.x < (unsigned)off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) partials[c] = red[0];
    __syncthreads();
  }
}

__global__ void scan_tile_finalize_kernel(const int32_t* __restrict__ sizes, int64_t n,
                                          int64_t ntiles,
                                          const int64_t* __restrict__ partials,
                                          int32_t* __restrict__ offsets)
{
  __shared__ int32_t tile[SCAN_T];
  __shared__ int64_t segsum[SBLOCK + 1];
  for (int64_t c = blockIdx.x; c < ntiles; c += gridDim.x) {
    const int64_t base = c * SCAN_T;
#pragma unroll
    for (int k = 0; k < SSEG; k++) {
      int64_t i = base + (int64_t)k * SBLOCK + threadIdx.x;
      tile[(int64_t)k * SBLOCK + threadIdx.x] = (i < n) ? sizes[i] : 0;
    }
    __syncthreads();
    /* in-place exclusive scan of this thread's contiguous LDS segment */
    int32_t acc = 0;
#pragma unroll
    for (int v = 0; v < SSEG; v++) {
      int32_t x = tile[threadIdx.x * SSEG + v];
      tile[threadIdx.x * SSEG + v] = acc;
      acc += x;
    }
    segsum[threadIdx.x] = acc;
    __syncthreads();
    /* exclusive scan of the 256 segment sums (Hillis-Steele in LDS) */
    for (int off = 1; off < SBLOCK; off <<= 1) {
      int64_t add = (threadIdx.x >= (unsigned)off) ? segsum[threadIdx.x - off] : 0;
      __syncthreads();
      segsum[threadIdx.x] += add;
      __syncthreads();
    }
    if (threadIdx.x == 0) segsum[SBLOCK] = segsum[SBLOCK - 1];  // tile total
    __syncthreads();
    const int64_t tbase = partials[c];
#pragma unroll
    for (int k = 0; k < SSEG; k++) {
      int64_t i = base + (int64_t)k * SBLOCK + threadIdx.x;
      if (i < n) {
        int j = (int)((int64_t)k * SBLOCK + threadIdx.x);
        int64_t seg_excl = (j >= SSEG) ? segsum[j / SSEG - 1] : 0;
        offsets[i] = (int32_t)(tbase + seg_excl + tile[j]);
      }
    }
    if (threadIdx.x == 0 && base + SCAN_T >= n)
      offsets[n] = (int32_t)(tbase + segsum[SBLOCK]);
    __syncthreads();
  }
}

/* single block: exclusive scan of partials in place */
__global__ void scan_partials_exclusive_kernel(int64_t* partials, int64_t nchunks)
{
  __shared__ int64_t sh[SCAN_PASS];
  __shared__ int64_t running_sh;
  if (threadIdx.x == 0) running_sh = 0;
  __syncthreads();
  for (int64_t base = 0; base < nchunks; base += SCAN_PASS) {
    int64_t c = base + threadIdx.x;
    int64_t v = (c < nchunks) ? partials[c] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_PASS; off <<= 1) {
      int64_t add = (threadIdx.x >= (unsigned)off) ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    int64_t rbase = running_sh;
    __syncthreads();
    if (c < nchunks) partials[c] = rbase + sh[threadIdx.x] - v;
    if (threadIdx.x == SCAN_PASS - 1) running_sh = rbase + sh[threadIdx.x];
    __syncthreads();
  }
}

size_t offsets_from_sizes_scratch_bytes(int64_t n)
{
  int64_t nchunks = (n + CHUNK - 1) / CHUNK;
  return (size_t)(nchunks > 0 ? nchunks : 1) * sizeof(int64_t);
}

void offsets_from_sizes(const int32_t* d_sizes, int64_t n, int32_t* d_offsets, void* d_scratch,
                        hipStream_t s)
{
  if (n <= 0) {
    DJ_HIP_CALL(hipMemsetAsync(d_offsets, 0, sizeof(int32_t), s));
    return;
  }
  int64_t* partials = (int64_t*)d_scratch;  // scratch sized by CHUNK < SCAN_T
  int64_t ntiles = (n + SCAN_T - 1) / SCAN_T;
  int tgrid = (int)(ntiles < SGRID_CAP ? ntiles : SGRID_CAP);
  hipLaunchKernelGGL(scan_tile_partials_kernel, dim3(tgrid), dim3(SBLOCK), 0, s, d_sizes, n,
                     ntiles, partials);
  DJ_HIP_CALL(hipGetLastError());
  hipLaunchKernelGGL(scan_partials_exclusive_kernel, dim3(1), dim3(SCAN_PASS), 0, s, partials,
                     ntiles);
  DJ_HIP_CALL(hipGetLastError());
  hipLaunchKernelGGL(scan_tile_finalize_kernel, dim3(tgrid), dim3(SBLOCK), 0, s, d_sizes, n,
                     ntiles, partials, d_offsets);
  DJ_HIP_CALL(hipGetLastError());
}

/* ---- permutation gathers ---- */

__global__ void gather_sizes_kernel(const int32_t* __restrict__ src_off,
                                    const int64_t* __restrict__ idx, int64_t n,
                                    int32_t* __restrict__ sizes)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t j = idx[i];
    sizes[i] = src_off[j + 1] - src_off[j];
  }
}

void gather_sizes(const int32_t* d_src_off, const int64_t* d_idx, int64_t n, int32_t* d_sizes,
                  hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(gather_sizes_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s, d_src_off, d_idx,
                     n, d_sizes);
  DJ_HIP_CALL(hipGetLastError());
}

/* sizes AND source char starts in one pass over the random offsets (the
 * 8 B line serves both); gather_chars_from_starts then streams the staged
 * starts sequentially instead of re-walking idx + src_off at random —
 * cuts the chars gather's line traffic roughly in half at TPC-H scale */
__global__ void gather_sizes_starts_kernel(const int32_t* __restrict__ src_off,
                                           const int64_t* __restrict__ idx, int64_t n,
                                           int32_t* __restrict__ sizes,
                                           int32_t* __restrict__ starts)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t j = idx[i];
    int32_t s0 = src_off[j];
    sizes[i] = src_off[j + 1] - s0;
    starts[i] = s0;
  }
}

void gather_sizes_starts(const int32_t* d_src_off, const int64_t* d_idx, int64_t n,
                         int32_t* d_sizes, int32_t* d_starts, hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(gather_sizes_starts_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s,
                     d_src_off, d_idx, n, d_sizes, d_starts);
  DJ_HIP_CALL(hipGetLastError());
}

/* per row: load the 1..3 aligned u64 words covering [s0, s0+len) once and
 * extract bytes from registers — a byte-loop re-loads the same line len
 * times (len ≈ 8 per row at TPC-H/config-4 string sizes, so this quarters
 * the load instructions; the byte STORES stay — adjacent rows share dst
 * words, so wide stores would race on the shared bytes). Safe to read the
 * full aligned window: hipMalloc allocations are >= 4 KiB aligned, so the
 * 8 B-aligned words of any valid [s0, s0+len) range stay in-allocation. */
__global__ void gather_chars_from_starts_kernel(const uint8_t* __restrict__ src_chars,
                                                const int32_t* __restrict__ starts, int64_t n,
                                                const int32_t* __restrict__ dst_off,
                                                uint8_t* __restrict__ dst_chars)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t s0 = (int64_t)starts[i];
    const int64_t d0 = dst_off[i];
    const int32_t len = dst_off[i + 1] - (int32_t)d0;
    if (len <= 0) continue;  // an empty row loads nothing (src_chars may be null)
    const uint64_t* words = (const uint64_t*)(src_chars + (s0 & ~(int64_t)7));
    int off = (int)(s0 & 7);  // first byte's position in words[0]
    uint64_t w = words[0];
    int wi = 0;
    for (int32_t k = 0; k < len; k++) {
      const int b = off + k;
      if ((b >> 3) != wi) {
        wi = b >> 3;
        w = words[wi];
      }
      dst_chars[d0 + k] = (uint8_t)(w >> ((b & 7) * 8));
    }
  }
}

void gather_chars_from_starts(const uint8_t* d_src_chars, const int32_t* d_starts, int64_t n,
                              const int32_t* d_dst_off, uint8_t* d_dst_chars, hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(gather_chars_from_starts_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s,
                     d_src_chars, d_starts, n, d_dst_off, d_dst_chars);
  DJ_HIP_CALL(hipGetLastError());
}

/* ---- STRING key columns: row hash (dj_strhash.h spec) ----
 *
 * One thread per row. A block walks tiles of HS_TILE_ROWS consecutive rows in
 * spans; a span's bytes are one contiguous chars range [off[row0],
 * off[row1]). The block takes the largest span (the rest of the tile, 1024,
 * 512 or 256 rows) whose range fits the LDS budget, stages it with coalesced
 * 16-byte loads and hashes its rows (thread t: rows t, t+256, ...) out of
 * LDS — short strings amortise the two dependent global round trips of a
 * span over 8 rows per thread. A 256-row span that does not fit (long
 * strings) reads global memory directly. The choice is made per span, so
 * per block.
 *
 * Neither path reads a byte outside the rows' own ranges: key columns are
 * caller-owned views and slices of shuffle outputs, so no allocation
 * alignment or padding is assumed. The staged path issues 16-byte loads only
 * for the 16-byte-aligned chunks lying wholly inside the range and copies
 * the < 16 head and tail bytes one by one; the direct path issues dword
 * loads only for aligned dwords wholly inside the row and assembles the
 * partial first/last dword from byte loads. A zero-length row loads nothing.
 *
 * The LDS image keeps each byte's global address modulo 16, so both paths
 * hash the same "aligned dword window" of a row: MurmurHash3's unaligned
 * 4-byte blocks come from two neighbouring aligned dwords and one
 * v_alignbyte. */

constexpr int HS_BLOCK = 256;
/* rows a block takes per outer step: 8 per thread when they stage as one span */
constexpr int HS_TILE_ROWS = 8 * HS_BLOCK;
/* 32 KiB of the 160 KiB CU LDS: 4-5 blocks stay resident per CU */
constexpr int HS_LDS_BYTES = 32 << 10;

namespace {

__device__ __forceinline__ uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3)));
#endif
}

/* Both murmur states from one pass over a row. fetch(j) returns aligned
 * dword j of the row's window (dword 0 holds the row's first byte at byte
 * position s); it is called only for dwords that hold at least one row byte,
 * and bytes of those dwords outside the row never reach the result. */
template <class Fetch>
__device__ __forceinline__ void murmur3_row2(Fetch fetch, uint32_t s, int32_t len,
                                             uint32_t seed_a, uint32_t seed_b, uint32_t& out_a,
                                             uint32_t& out_b)
{
  uint32_t ha = seed_a, hb = seed_b;
  const int32_t nwords = len > 0 ? (int32_t)(((int64_t)s + len + 3) >> 2) : 0;
  const int32_t nblocks = len >> 2;
  uint32_t lo = nwords > 0 ? fetch(0) : 0u;
  for (int32_t k = 0; k < nblocks; k++) {
    const uint32_t hi = (k + 1 < nwords) ? fetch(k + 1) : 0u;
    const uint32_t blk = align_bytes(hi, lo, s);
    ha = dj_murmur3_block(ha, blk);
    hb = dj_murmur3_block(hb, blk);
    lo = hi;
  }
  const int rem = len & 3;
  if (rem) {
    const uint32_t hi = (nblocks + 1 < nwords) ? fetch(nblocks + 1) : 0u;
    const uint32_t t = align_bytes(hi, lo, s) & ((1u << (8 * rem)) - 1u);
    ha = dj_murmur3_tail(ha, t);
    hb = dj_murmur3_tail(hb, t);
  }
  out_a = dj_fmix32(ha ^ (uint32_t)len);
  out_b = dj_fmix32(hb ^ (uint32_t)len);
}

}  // namespace

/* out64 != nullptr: dj_string_key64 layout (seed_a low half, seed_b high);
 * else out32 = the seed_a hash (the dj_hash_strings test hook) */
__global__ __launch_bounds__(HS_BLOCK) void hash_strings_kernel(
  const int32_t* __restrict__ offsets, const uint8_t* __restrict__ chars, int64_t n,
  int64_t ntiles, int force_direct, uint32_t seed_a, uint32_t seed_b,
  uint64_t* __restrict__ out64, uint32_t* __restrict__ out32)
{
  __shared__ uint4 stage4[HS_LDS_BYTES / 16];
  uint8_t* stage8 = (uint8_t*)stage4;
  const uint32_t* stage32 = (const uint32_t*)stage4;
  const uint32_t tid = threadIdx.x;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t tile0 = tile * HS_TILE_ROWS;
    const int64_t tile1 = tile0 + HS_TILE_ROWS < n ? tile0 + HS_TILE_ROWS : n;
    int64_t row0 = tile0;
    while (row0 < tile1) {
      /* everything up to the row loop is block-uniform: all threads read the
       * same offsets and take the same branches */
      const int32_t c0 = offsets[row0];
      const uintptr_t abeg = (uintptr_t)chars + (uintptr_t)(uint32_t)c0;
      const uintptr_t base16 = abeg & ~(uintptr_t)15;
      /* + 8: a row's last window dword may start up to 3 bytes before aend */
      const int64_t room = (int64_t)HS_LDS_BYTES - 8 - (int64_t)(abeg - base16);
      /* the largest span of rows (the whole rest of the tile, or 1024, 512,
       * 256 rows) whose chars fit the LDS budget; a 256-row span that does
       * not fit reads global memory directly. The candidate end offsets are
       * independent loads. */
      int64_t row1 = tile1;
      int32_t c1 = c0;
      bool staged = false;
      if (!force_direct) {
        int64_t re[4];
        int32_t ce[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          re[k] = row0 + (HS_TILE_ROWS >> k) < tile1 ? row0 + (HS_TILE_ROWS >> k) : tile1;
          ce[k] = offsets[re[k]];
        }
        row1 = re[3];
        c1 = ce[3];
#pragma unroll
        for (int k = 2; k >= 0; k--) {
          if ((int64_t)ce[k] - c0 <= room) {
            row1 = re[k];
            c1 = ce[k];
          }
        }
        staged = c1 > c0 && (int64_t)c1 - c0 <= room;
      }
      const uintptr_t aend = (uintptr_t)chars + (uintptr_t)(uint32_t)c1;

      if (staged) {
        const uintptr_t first16 = (abeg + 15) & ~(uintptr_t)15;
        const uintptr_t last16 = aend & ~(uintptr_t)15;
        const uintptr_t head_end = first16 < aend ? first16 : aend;
        const uintptr_t tail_beg = last16 > head_end ? last16 : head_end;
        if (first16 < last16) {
          const uint32_t nvec = (uint32_t)((last16 - first16) >> 4);
          const uint4* __restrict__ g = (const uint4*)first16;
          uint4* l = stage4 + ((first16 - base16) >> 4);
          for (uint32_t v = tid; v < nvec; v += HS_BLOCK) l[v] = g[v];
        }
        const uint32_t head_len = (uint32_t)(head_end - abeg);  // < 16
        const uint32_t tail_len = (uint32_t)(aend - tail_beg);  // < 16
        if (tid < head_len) stage8[(abeg - base16) + tid] = *(const uint8_t*)(abeg + tid);
        if (tid >= 32 && tid - 32 < tail_len)
          stage8[(tail_beg - base16) + (tid - 32)] = *(const uint8_t*)(tail_beg + (tid - 32));
        __syncthreads();
      }

      for (int64_t r = row0 + tid; r < row1; r += HS_BLOCK) {
        const int32_t o0 = offsets[r];
        const int32_t len = offsets[r + 1] - o0;
        uint32_t ha, hb;
        if (staged) {
          const uint32_t lb = (uint32_t)(abeg - base16) + (uint32_t)(o0 - c0);
          const uint32_t w0 = lb >> 2;
          murmur3_row2([&](int32_t j) { return stage32[w0 + (uint32_t)j]; }, lb & 3u, len,
                       seed_a, seed_b, ha, hb);
        } else {
          const uintptr_t ap = (uintptr_t)chars + (uintptr_t)(uint32_t)o0;
          const uintptr_t ae = ap + (uintptr_t)(uint32_t)len;
          const uintptr_t wb = ap & ~(uintptr_t)3;
          murmur3_row2(
            [&](int32_t j) {
              const uintptr_t wa = wb + 4 * (uintptr_t)(uint32_t)j;
              if (wa >= ap && wa + 4 <= ae) return *(const uint32_t*)wa;
              uint32_t v = 0;
#pragma unroll
              for (int b = 0; b < 4; b++) {
                const uintptr_t a = wa + b;
                if (a >= ap && a < ae) v |= (uint32_t)(*(const uint8_t*)a) << (8 * b);
              }
              return v;
            },
            (uint32_t)(ap & 3), len, seed_a, seed_b, ha, hb);
        }
        if (out64)
          out64[r] = (uint64_t)ha | ((uint64_t)hb << 32);
        else
          out32[r] = ha;
      }
      if (staged) __syncthreads();  // the next span restages the LDS image
      row0 = row1;
    }
  }
}

namespace {
void launch_hash_strings(const int32_t* d_offsets, const uint8_t* d_chars, int64_t n,
                         uint32_t seed_a, uint32_t seed_b, uint64_t* d_out64,
                         uint32_t* d_out32, hipStream_t s)
{
  if (n <= 0) return;
  /* A/B switch for the staged path (benchmark/string_key_bench.py) */
  static const int force_direct = getenv("DJ_STRHASH_FORCE_DIRECT") ? 1 : 0;
  const int64_t ntiles = (n + HS_TILE_ROWS - 1) / HS_TILE_ROWS;
  const int grid = (int)(ntiles < HS_GRID_CAP ? ntiles : HS_GRID_CAP);
  hipLaunchKernelGGL(hash_strings_kernel, dim3(grid), dim3(HS_BLOCK), 0, s, d_offsets, d_chars,
                     n, ntiles, force_direct, seed_a, seed_b, d_out64, d_out32);
  DJ_HIP_CALL(hipGetLastError());
}
}  // namespace

void hash_strings(const int32_t* d_offsets, const uint8_t* d_chars, int64_t n, uint64_t* d_out,
                  hipStream_t s)
{
  launch_hash_strings(d_offsets, d_chars, n, DJ_STRKEY_SEED_LO, DJ_STRKEY_SEED_HI, d_out,
                      nullptr, s);
}

void hash_strings_seeded(const int32_t* d_offsets, const uint8_t* d_chars, int64_t n,
                         uint32_t seed, uint32_t* d_out, hipStream_t s)
{
  launch_hash_strings(d_offsets, d_chars, n, seed, seed, nullptr, d_out, s);
}

GridSpan strings_grid_span(int family)
{
  switch (family) {
    case kSpanStringRows: return {(int64_t)SGRID_CAP * SBLOCK, 0};
    case kSpanStringSum: return {(int64_t)SUM_GRID_CAP * 256, 0};
    case kSpanStringScan: /* a block per SCAN_T-row tile, a partial per tile */
      return {(int64_t)SGRID_CAP * SCAN_T, (int64_t)SCAN_PASS * SCAN_T};
    case kSpanStringHash: return {(int64_t)HS_GRID_CAP * HS_TILE_ROWS, 0};
    default: return {0, 0};
  }
}

/* ---- collision filter over key tuples: integer-rep and STRING columns ---- */

/* lengths first, then bytes; reads exactly [a, a+la) and [b, b+la) and
 * nothing at all for two empty strings */
__device__ __forceinline__ bool string_equal(const uint8_t* a, int32_t la, const uint8_t* b,
                                             int32_t lb)
{
  if (la != lb) return false;
  for (int32_t k = 0; k < la; k++)
    if (a[k] != b[k]) return false;
  return true;
}

__global__ void filter_tuple_matches_mixed_kernel(TupleKeys keys, const int64_t* __restrict__ li,
                                                  const int64_t* __restrict__ ri, int64_t n,
                                                  int64_t* __restrict__ out_li,
                                                  int64_t* __restrict__ out_ri,
                                                  unsigned long long* __restrict__ count)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t a = li[i], b = ri[i];
    bool eq = true;
    for (int c = 0; c < keys.nk && eq; c++) {
      const TupleKeyCol& lc = keys.l[c];
      const TupleKeyCol& rc = keys.r[c];
      /* null_equality::EQUAL: null matches null and no valid element; the
       * value (and string size) stored under a null is never read */
      const bool lv = key_is_valid(lc.valid, a), rv = key_is_valid(rc.valid, b);
      if (!lv || !rv) {
        eq = lv == rv;
      } else if (lc.kind == kKeyStr) {
        const int32_t* lo = (const int32_t*)lc.data;
        const int32_t* ro = (const int32_t*)rc.data;
        const int32_t l0 = lo[a], r0 = ro[b];
        eq = string_equal(lc.chars + l0, lo[a + 1] - l0, rc.chars + r0, ro[b + 1] - r0);
      } else {
        eq = load_key_i64(lc.data, lc.kind, a) == load_key_i64(rc.data, rc.kind, b);
      }
    }
    if (eq) {
      unsigned long long pos = atomicAdd(count, 1ull);
      out_li[pos] = a;
      out_ri[pos] = b;
    }
  }
}

void filter_tuple_matches_mixed(const TupleKeys& keys, const int64_t* d_li, const int64_t* d_ri,
                                int64_t n, int64_t* d_out_li, int64_t* d_out_ri,
                                unsigned long long* d_count, hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(filter_tuple_matches_mixed_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s,
                     keys, d_li, d_ri, n, d_out_li, d_out_ri, d_count);
  DJ_HIP_CALL(hipGetLastError());
}

/* ---- deterministic test/bench string payload (string_payload.cu:50-94) ---- */

__global__ void test_string_sizes_kernel(const int64_t* __restrict__ keys, int64_t n,
                                         int32_t* __restrict__ sizes)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) sizes[i] = (int32_t)(keys[i] % 7 + 1);
}

__global__ void fill_test_strings_kernel(const int64_t* __restrict__ keys, int64_t n,
                                         const int32_t* __restrict__ offsets,
                                         uint8_t* __restrict__ chars)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int32_t o0 = offsets[i], o1 = offsets[i + 1];
    uint8_t ch = (uint8_t)('a' + keys[i] % 26);
    for (int32_t k = o0; k < o1; k++) chars[k] = ch;
  }
}

void make_test_string_sizes(const int64_t* d_keys, int64_t n, int32_t* d_sizes, hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(test_string_sizes_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s, d_keys, n,
                     d_sizes);
  DJ_HIP_CALL(hipGetLastError());
}

void fill_test_strings(const int64_t* d_keys, int64_t n, const int32_t* d_offsets,
                       uint8_t* d_chars, hipStream_t s)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(fill_test_strings_kernel, dim3(sgrid(n)), dim3(SBLOCK), 0, s, d_keys, n,
                     d_offsets, d_chars);
  DJ_HIP_CALL(hipGetLastError());
}

}  // namespace dj
