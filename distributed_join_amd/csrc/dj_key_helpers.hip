/*
 * dj_key_helpers.hip — the small row kernels of the host orchestration layer
 * (key widening / narrowing / fusing, placement hash of a nullable key,
 * STRING offset rebase, iota and fill) and their launchers (dj_kernels.hpp,
 * "key helper kernels"). A thread per row on a capped grid; a grid-stride
 * loop covers the rest.
 */
#include "dj_kernels.hpp"

#include "dj_hash.h"
#include "dj_rng.h"

namespace {

constexpr int kBlock = 256;
/* blocks per launch at most; a grid-stride loop covers the rest */
constexpr int kGridCap = 2048;

int grid_for_n(int64_t n)
{
  int64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > kGridCap) blocks = kGridCap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

__global__ void iota_i64_kernel(int64_t* dst, int64_t n)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = i;
}

__global__ void fill_i32_kernel(int32_t* dst, int64_t n, int32_t value)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = value;
}

/* narrow integer-rep key column -> the engine's int64 key (sign- or
 * zero-extended per dj::load_key_i64) */
__global__ void widen_key_kernel(const void* __restrict__ src, int kind, int64_t n,
                                 int64_t* __restrict__ dst)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = dj::load_key_i64(src, kind, i);
}

/* joined int64 key values back to a 1-/2-/4-byte key column (truncation
 * inverts either extension) */
__global__ void narrow_key_kernel(const int64_t* __restrict__ src, int64_t n, int width,
                                  void* __restrict__ dst)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t v = src[i];
    if (width == 4)
      ((int32_t*)dst)[i] = (int32_t)v;
    else if (width == 2)
      ((int16_t*)dst)[i] = (int16_t)v;
    else
      ((int8_t*)dst)[i] = (int8_t)v;
  }
}

/* fused multi-column key: h_i = chain of mix64 over the key tuple — the
 * single-key engine then partitions/joins on h as if it were the key, and
 * the caller filters hash-collision false positives against the real
 * columns afterwards (local_join). `weak` collapses h to 4 bits so tests can
 * exercise that filter deterministically. */
__global__ void fuse_keys_kernel(const int64_t* __restrict__ c0, const int64_t* __restrict__ c1,
                                 const int64_t* __restrict__ c2, const int64_t* __restrict__ c3,
                                 uint32_t kinds /*4 bits per col: dj::kKey* */, int ncols,
                                 int64_t n, int weak, int64_t* __restrict__ out,
                                 const uint32_t* __restrict__ m0 = nullptr,
                                 const uint32_t* __restrict__ m1 = nullptr,
                                 const uint32_t* __restrict__ m2 = nullptr,
                                 const uint32_t* __restrict__ m3 = nullptr)
{
  const int64_t* cols[4] = {c0, c1, c2, c3};
  const uint32_t* masks[4] = {m0, m1, m2, m3};
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int c = 0; c < ncols; c++) {
      /* a null element enters the chain as the null element hash; the value
       * stored under it is not read */
      int64_t v = dj::key_is_valid(masks[c], i)
                    ? dj::load_key_i64(cols[c], (int)((kinds >> (4 * c)) & 0xF), i)
                    : (int64_t)dj::kNullKeyHash;
      h = dj_mix64(h ^ (uint64_t)v);
    }
    out[i] = weak ? (int64_t)(h & 0xF) : (int64_t)h;
  }
}

/* placement hash of a single nullable integer-rep key column: dj_row_hash of
 * a valid element, the null element hash of a null one (never reading the
 * value under it) */
__global__ void nullable_key_hash_kernel(const void* __restrict__ src, int kind,
                                         const uint32_t* __restrict__ valid, int64_t n,
                                         int hash_fn, uint32_t seed, int64_t* __restrict__ out)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    out[i] = dj::key_is_valid(valid, i)
               ? (int64_t)dj_row_hash(dj::load_key_i64(src, kind, i), hash_fn, seed)
               : (int64_t)dj::kNullKeyHash;
}

/* rebase a part's offsets by a constant and append (STRING concat) */
__global__ void rebase_offsets_kernel(const int32_t* __restrict__ src, int64_t n, int32_t base,
                                      int32_t* __restrict__ dst)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i] + base;
}

}  // namespace

namespace dj {

/* this file's row kernels (grid_for_n): a thread per row (dj_kernels.hpp) */
GridSpan key_helper_grid_span(int family)
{
  if (family == kSpanKeyHelpers) return {(int64_t)kGridCap * kBlock, 0};
  return {0, 0};
}

void iota_i64(int64_t* d_dst, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(iota_i64_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_dst, n);
}

void fill_i32(int32_t* d_dst, int64_t n, int32_t value, hipStream_t s)
{
  hipLaunchKernelGGL(fill_i32_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_dst, n, value);
}

void widen_key(const void* d_src, int kind, int64_t n, int64_t* d_dst, hipStream_t s)
{
  hipLaunchKernelGGL(widen_key_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_src, kind, n,
                     d_dst);
}

void narrow_key(const int64_t* d_src, int64_t n, int width, void* d_dst, hipStream_t s)
{
  hipLaunchKernelGGL(narrow_key_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_src, n, width,
                     d_dst);
}

void fuse_key_columns(const int64_t* const d_cols[4], const uint32_t* const d_masks[4],
                      uint32_t kinds, int ncols, int64_t n, int weak, int64_t* d_out,
                      hipStream_t s)
{
  hipLaunchKernelGGL(fuse_keys_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_cols[0],
                     d_cols[1], d_cols[2], d_cols[3], kinds, ncols, n, weak, d_out, d_masks[0],
                     d_masks[1], d_masks[2], d_masks[3]);
}

void nullable_key_hash(const void* d_src, int kind, const uint32_t* d_valid, int64_t n,
                       int hash_fn, uint32_t seed, int64_t* d_out, hipStream_t s)
{
  hipLaunchKernelGGL(nullable_key_hash_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_src,
                     kind, d_valid, n, hash_fn, seed, d_out);
}

void rebase_offsets(const int32_t* d_src, int64_t n, int32_t base, int32_t* d_dst, hipStream_t s)
{
  hipLaunchKernelGGL(rebase_offsets_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, s, d_src, n,
                     base, d_dst);
}

}  // namespace dj
