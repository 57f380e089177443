/*
 * dj_bitmask.hip — validity-mask kernels (cuDF mask layout: row i is bit
 * i % 32, LSB first, of uint32 word i / 32; 1 = valid; a null mask pointer
 * means "all valid").
 *
 *   gather_bitmasks        out bit i of column c = bit idx[i] of src_c, for up
 *                          to kMaxSchemaCols columns through one index array
 *   copy_bitmask_segments  concatenate bit ranges cut at arbitrary bit
 *                          offsets into one destination mask
 *   count_unset_bits       nulls among the first n bits of a mask
 *   key_row_validity       the AND of up to 4 masks (the rows of a key tuple
 *                          that hold no null) and the number of its 0 bits
 *
 * No kernel here does a read-modify-write or an atomic on a mask word: every
 * destination word is built whole by one lane and stored once. Bits past the
 * row count are never read as information (they are unspecified on input)
 * and are written as 0.
 */
#include "dj_error.hpp"
#include "dj_kernels.hpp"

#include <hip/hip_runtime.h>

namespace dj {

namespace {

constexpr int kMaskBlock = 256;
constexpr int kWave = 64;
/* blocks per launch at most; a grid-stride loop covers the rest */
constexpr int kMaskGridCap = 2048;

/* One wave owns 64 consecutive, 64-aligned output rows: lane l tests the
 * source bit of row chunk*64+l, one __ballot per column yields the two mask
 * words of the chunk, and lane 0 writes them with a single 8-byte store
 * (little-endian: rows 0..31 are the low word). Lanes past n vote 0, which
 * zeroes output bits [n, roundup(n, 64)). Null counts: popcount of the
 * complementary ballot, summed per block in LDS, one global atomicAdd per
 * block per column (onto the counter array, never onto a mask word). */
__global__ __launch_bounds__(kMaskBlock) void gather_bitmasks_kernel(
  BitmaskGatherDesc d, const int64_t* __restrict__ idx, int64_t n, int64_t nchunks,
  uint32_t* __restrict__ null_counts)
{
  __shared__ uint32_t s_nulls[kMaxSchemaCols];
  if (threadIdx.x < kMaxSchemaCols) s_nulls[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = ((int64_t)blockIdx.x * kMaskBlock + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (kMaskBlock / kWave);
  for (int64_t chunk = wave0; chunk < nchunks; chunk += nwaves) {
    const int64_t row = chunk * kWave + lane;
    const bool in = row < n;
    const int64_t j = in ? idx[row] : 0;
    for (int c = 0; c < d.ncols; c++) {
      const uint32_t* src = d.src[c];
      bool valid = in;
      if (in && src != nullptr) valid = (src[j >> 5] >> (j & 31)) & 1u;
      const unsigned long long v = __ballot(valid);
      const unsigned long long z = __ballot(in && !valid);
      if (lane == 0) {
        ((unsigned long long*)d.dst[c])[chunk] = v;
        if (z) atomicAdd(&s_nulls[c], (uint32_t)__popcll(z));
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < d.ncols && s_nulls[threadIdx.x])
    atomicAdd(&null_counts[threadIdx.x], s_nulls[threadIdx.x]);
}

/* `take` bits (1..32) of `src` starting at bit `sb`, in the low bits of the
 * result. Touches src word sb/32 and, only when the range crosses into it,
 * word sb/32 + 1 — both inside the words the range itself covers. */
__device__ __forceinline__ uint32_t extract_bits(const uint32_t* __restrict__ src, int64_t sb,
                                                 int take)
{
  const int64_t w = sb >> 5;
  const int sh = (int)(sb & 31);
  uint32_t v = src[w] >> sh;
  if (sh + take > 32) v |= src[w + 1] << (32 - sh);
  return take == 32 ? v : (v & ((1u << take) - 1u));
}

/* Destination-word-centric: thread w builds destination word w from every
 * segment overlapping bits [32w, 32w+32) — binary search for the first one,
 * then a walk (one word may be covered by many short segments, and
 * zero-length segments may sit anywhere). Words are stored whole; bits at or
 * past `total` are 0. */
__global__ __launch_bounds__(kMaskBlock) void copy_bitmask_segments_kernel(
  const uint32_t* const* __restrict__ seg_src, const int64_t* __restrict__ seg_src_bit,
  const int64_t* __restrict__ seg_dst_bit /* S+1, [S] = total */, int S, int64_t total,
  int64_t nwords, uint32_t* __restrict__ dst)
{
  int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; w < nwords; w += stride) {
    int64_t pos = w * 32;
    const int64_t end = pos + 32 < total ? pos + 32 : total;
    uint32_t word = 0;
    if (pos < end) {
      /* last segment whose start is <= pos: the non-empty one holding pos */
      int lo = 0, hi = S;  // first s in [0, S] with seg_dst_bit[s] > pos
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_dst_bit[mid] > pos)
          hi = mid;
        else
          lo = mid + 1;
      }
      int s = lo - 1;
      while (pos < end && s < S) {
        const int64_t s0 = seg_dst_bit[s], s1 = seg_dst_bit[s + 1];
        if (s1 <= pos) {  // zero-length segment
          s++;
          continue;
        }
        const int take = (int)((s1 < end ? s1 : end) - pos);
        const uint32_t* src = seg_src[s];
        const uint32_t bits = src != nullptr
                                ? extract_bits(src, seg_src_bit[s] + (pos - s0), take)
                                : (take == 32 ? 0xFFFFFFFFu : ((1u << take) - 1u));
        word |= bits << (int)(pos - w * 32);
        pos += take;
        if (pos >= s1) s++;
      }
    }
    dst[w] = word;
  }
}

__global__ __launch_bounds__(kMaskBlock) void count_unset_bits_kernel(
  const uint32_t* __restrict__ mask, int64_t n, int64_t nwords,
  unsigned long long* __restrict__ out)
{
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  uint32_t acc = 0;
  int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; w < nwords; w += stride) {
    const int64_t rem = n - w * 32;
    const uint32_t live = rem >= 32 ? 0xFFFFFFFFu : ((1u << (int)rem) - 1u);
    acc += (uint32_t)__popc(~mask[w] & live);
  }
  /* wave reduction, then one LDS add per wave and one global add per block */
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(&s_sum, acc);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(out, (unsigned long long)s_sum);
}

/* the masks of a key tuple's columns; nullptr = that column is all valid */
struct KeyMasks {
  const uint32_t* m[kMaxKeyMasks];
  int n;
};

/* Thread w builds destination word w: the AND of word w of every mask that is
 * there, cut to the rows below nrows, stored once. Reads (masks present) x
 * nrows / 8 bytes and writes nrows / 8; the 0 bits among nrows are summed per
 * wave, per block in LDS, and leave as one global atomicAdd per block onto
 * the counter (never onto a mask word). */
__global__ __launch_bounds__(kMaskBlock) void key_row_validity_kernel(
  KeyMasks km, int64_t nrows, int64_t nwords, uint32_t* __restrict__ dst,
  unsigned long long* __restrict__ nulls)
{
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  uint32_t acc = 0;
  int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; w < nwords; w += stride) {
    const int64_t rem = nrows - w * 32;
    const uint32_t live = rem >= 32 ? 0xFFFFFFFFu : ((1u << (int)rem) - 1u);
    uint32_t v = live;
    for (int c = 0; c < km.n; c++)
      if (km.m[c] != nullptr) v &= km.m[c][w];
    dst[w] = v;
    acc += (uint32_t)__popc(~v & live);
  }
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(&s_sum, acc);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(nulls, (unsigned long long)s_sum);
}

int mask_grid(int64_t items_per_thread_domain)
{
  int64_t blocks = (items_per_thread_domain + kMaskBlock - 1) / kMaskBlock;
  if (blocks > kMaskGridCap) blocks = kMaskGridCap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

}  // namespace

GridSpan bitmask_grid_span(int family)
{
  switch (family) {
    case kSpanMaskGather: /* a wave per 64-row chunk */
      return {(int64_t)kMaskGridCap * (kMaskBlock / kWave) * kWave, 0};
    case kSpanMaskWords: /* a thread per mask word */
      return {(int64_t)kMaskGridCap * kMaskBlock, 0};
    default: return {0, 0};
  }
}

void gather_bitmasks(const BitmaskGatherDesc& desc, const int64_t* d_idx, int64_t n,
                     uint32_t* d_null_counts, hipStream_t s, int cols_per_launch)
{
  DJ_CHECK_ERROR(desc.ncols >= 0 && desc.ncols <= kMaxSchemaCols,
                 "gather_bitmasks: at most 32 columns per call");
  if (desc.ncols == 0 || n <= 0) return;
  for (int c = 0; c < desc.ncols; c++)
    DJ_CHECK_ERROR(desc.dst[c] != nullptr && ((uintptr_t)desc.dst[c] & 7) == 0,
                   "gather_bitmasks: destination masks must be 8-byte aligned");
  const int64_t nchunks = (n + kWave - 1) / kWave;
  const int64_t blocks = (nchunks + kMaskBlock / kWave - 1) / (kMaskBlock / kWave);
  if (cols_per_launch < 1 || cols_per_launch > kMaxSchemaCols) cols_per_launch = kMaxSchemaCols;
  for (int c0 = 0; c0 < desc.ncols; c0 += cols_per_launch) {
    BitmaskGatherDesc part{};
    part.ncols = desc.ncols - c0 < cols_per_launch ? desc.ncols - c0 : cols_per_launch;
    for (int c = 0; c < part.ncols; c++) {
      part.src[c] = desc.src[c0 + c];
      part.dst[c] = desc.dst[c0 + c];
    }
    hipLaunchKernelGGL(gather_bitmasks_kernel,
                       dim3((int)(blocks < kMaskGridCap ? blocks : kMaskGridCap)),
                       dim3(kMaskBlock), 0, s, part, d_idx, n, nchunks, d_null_counts + c0);
    DJ_HIP_CALL(hipGetLastError());
  }
}

void copy_bitmask_segments(const void* d_segments, int S, int64_t total_bits, uint32_t* d_dst,
                           hipStream_t s)
{
  if (total_bits <= 0 || S <= 0) return;
  const int64_t nwords = (total_bits + 31) / 32;
  const uint32_t* const* src = (const uint32_t* const*)d_segments;
  const int64_t* src_bit = (const int64_t*)d_segments + S;
  const int64_t* dst_bit = (const int64_t*)d_segments + 2 * (int64_t)S;
  hipLaunchKernelGGL(copy_bitmask_segments_kernel, dim3(mask_grid(nwords)), dim3(kMaskBlock), 0,
                     s, src, src_bit, dst_bit, S, total_bits, nwords, d_dst);
  DJ_HIP_CALL(hipGetLastError());
}

void count_unset_bits(const uint32_t* d_mask, int64_t n, unsigned long long* d_count,
                      hipStream_t s)
{
  if (n <= 0 || d_mask == nullptr) return;
  const int64_t nwords = (n + 31) / 32;
  hipLaunchKernelGGL(count_unset_bits_kernel, dim3(mask_grid(nwords)), dim3(kMaskBlock), 0, s,
                     d_mask, n, nwords, d_count);
  DJ_HIP_CALL(hipGetLastError());
}

void key_row_validity(const uint32_t* const* masks, int nmasks, int64_t nrows, uint32_t* d_out,
                      unsigned long long* d_null_count, hipStream_t s)
{
  DJ_CHECK_ERROR(nmasks >= 1 && nmasks <= kMaxKeyMasks, "key_row_validity: 1..4 masks");
  if (nrows <= 0) return;
  DJ_CHECK_ERROR(masks != nullptr && d_out != nullptr && d_null_count != nullptr,
                 "key_row_validity: null pointer");
  KeyMasks km{};
  km.n = nmasks;
  for (int c = 0; c < nmasks; c++) km.m[c] = masks[c];
  const int64_t nwords = (nrows + 31) / 32;
  hipLaunchKernelGGL(key_row_validity_kernel, dim3(mask_grid(nwords)), dim3(kMaskBlock), 0, s, km,
                     nrows, nwords, d_out, d_null_count);
  DJ_HIP_CALL(hipGetLastError());
}

}  // namespace dj
