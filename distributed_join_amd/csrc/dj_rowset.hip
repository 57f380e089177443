/*
 * dj_rowset.hip — row sets as bitmaps (cuDF bit layout: row i is bit i % 32,
 * LSB first, of uint32 word i / 32), the step between a join's pair list and
 * the rows an outer / semi / anti join keeps.
 *
 *   mark_rows    set bit idx[i] for every i < n; any index any number of
 *                times, from any number of lanes, waves and blocks at once
 *   select_rows  the indices i < nrows whose bit equals want_set, ascending,
 *                and their number
 *   compact_keyed_rows
 *                select_rows for the set bits that also carries a key: next
 *                to every selected row number goes keys[row]
 *
 * mark_rows is the only kernel of the library that does a read-modify-write
 * on a bitmap word: a no-return atomic OR, issued only for words that hold a
 * marked bit. select_rows and compact_keyed_rows build every output element
 * once, by rank.
 */
#include "dj_error.hpp"
#include "dj_kernels.hpp"

#include <hip/hip_runtime.h>

namespace dj {

namespace {

constexpr int kRowsetBlock = 256;
constexpr int kWave = 64;
/* blocks per launch at most; a grid-stride loop covers the rest */
constexpr int kRowsetGridCap = 4096;

/* ------------------------------------------------------------- mark_rows
 *
 * One index per lane per step, read as a coalesced 8-byte-per-lane stream.
 *
 * kMarkMerge: lanes of a wave whose indices fall into the same word combine
 * their bits before memory is touched. A suffix OR over six shuffle steps
 * (lane l takes the bits of lane l + d when that lane names the same word)
 * leaves, in the first lane of every run of equal words, the OR of the whole
 * run; only lanes whose predecessor names another word go on. Equal words in
 * lanes that are not neighbours are still correct — each run head issues its
 * own OR — so no sort and no match loop is needed. A join's pair list brings
 * a left row's m matches in neighbouring positions, which is the case this
 * catches; indices that are random with respect to row number merge nothing.
 *
 * kMarkCheck: a run head first loads the word (no read-modify-write) and
 * issues the atomic only when the word lacks one of its bits. Bits are only
 * ever set, so a word read before another lane's OR lands can only lack
 * bits, which costs a redundant atomic and never a missed one. A semi join
 * of multiplicity m finds the bit set m - 1 times out of m, and the bitmap
 * (nrows / 8 bytes) is small enough to stay in L2. Measured on MI355X
 *  the check never wins: the no-return atomic OR on an
 * L2-resident word costs what the load costs, so the engine runs the merge
 * alone (kMarkDefault) and the check stays as a variant for the benchmark.
 *
 * No word is written that holds no marked bit: the atomic's operand is never
 * 0 and names the word of an index that was passed. */
template <int MODE>
__global__ __launch_bounds__(kRowsetBlock) void mark_rows_kernel(
  const int64_t* __restrict__ idx, int64_t n, uint32_t* bits)
{
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kRowsetBlock;
  /* whole waves walk together, so that the shuffles see all 64 lanes */
  const int64_t n_up = (n + kWave - 1) / kWave * kWave;
  for (int64_t i = (int64_t)blockIdx.x * kRowsetBlock + threadIdx.x; i < n_up; i += stride) {
    const bool in = i < n;
    const int64_t j = in ? idx[i] : 0;
    /* a lane past n names the word -1, which no index has, and no bit */
    long long w = in ? (long long)(j >> 5) : -1ll;
    uint32_t b = in ? 1u << (int)(j & 31) : 0u;
    bool head = in;
    if (MODE & kMarkMerge) {
      const long long prev_w = __shfl_up(w, 1);
      head = in && (lane == 0 || prev_w != w);
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const long long ow = __shfl_down(w, d);
        const uint32_t ob = __shfl_down(b, d);
        if (lane + d < kWave && ow == w) b |= ob;
      }
    }
    if (head) {
      uint32_t* p = bits + w;
      if (MODE & kMarkCheck) {
        /* relaxed agent-scope load: served by L2, where the atomics land */
        const uint32_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur & b) != b) atomicOr(p, b);
      } else {
        atomicOr(p, b);
      }
    }
  }
}

/* ----------------------------------------------------------- select_rows
 *
 * A tile is kTileRows = 8192 consecutive rows: 256 mask words, one per
 * thread of a block.
 *   1. tile_count: popcount of the tile's selected bits -> counts[tile]
 *   2. tile_scan:  one block turns counts[] into exclusive int64 offsets in
 *                  place and writes the grand total to *d_count
 *   3. tile_write: each thread ranks its word inside the tile (wave scan via
 *                  shuffles, wave totals through LDS), drops the tile-local
 *                  row numbers of its bits into an LDS list at their rank,
 *                  and the block streams the list out as base + local, one
 *                  coalesced 8-byte-per-lane store stream per tile.
 * The bitmap is read twice (nrows / 8 bytes each time, the second time from
 * L2 at the sizes a join produces); every output element is written once.
 *
 * compact_keyed_rows is the same three phases with KEYED = true in the third:
 * the lane that stores out[base + k] = row also stores out_keys[base + k] =
 * keys[row]. The rows of a tile ascend with k, so the key reads of a tile
 * walk forward through one window of kTileRows * 8 = 64 KiB, and the key
 * stores are the same coalesced stream as the index stores. Per selected row
 * that is 8 bytes read and 16 written: nrows / 8 + 24 * selected bytes for
 * the whole call, counting the bitmap once (its second read is L2's). */
constexpr int kTileWords = kRowsetBlock;
constexpr int64_t kTileRows = (int64_t)kTileWords * 32;

/* thread's word of the tile with the wanted bits as 1 and everything at or
 * past nrows as 0 */
__device__ __forceinline__ uint32_t selected_word(const uint32_t* __restrict__ bits,
                                                  int64_t word, int64_t nrows, bool want_set)
{
  const int64_t rem = nrows - word * 32;
  if (rem <= 0) return 0u;
  uint32_t v = bits[word];
  if (!want_set) v = ~v;
  return rem >= 32 ? v : (v & ((1u << (int)rem) - 1u));
}

__global__ __launch_bounds__(kRowsetBlock) void tile_count_kernel(
  const uint32_t* __restrict__ bits, int64_t nrows, int64_t ntiles, bool want_set,
  int64_t* __restrict__ counts)
{
  __shared__ uint32_t s_sum;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    uint32_t c = (uint32_t)__popc(
      selected_word(bits, tile * kTileWords + threadIdx.x, nrows, want_set));
    for (int off = kWave / 2; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & (kWave - 1)) == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) counts[tile] = (int64_t)s_sum;
    __syncthreads();
  }
}

/* counts[0..ntiles) -> exclusive offsets in place, total -> *d_count. One
 * block; each thread owns a contiguous chunk, so the scan is two serial
 * passes over the chunk around one block-wide scan of the chunk sums. */
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void tile_scan_kernel(int64_t* __restrict__ counts,
                                                               int64_t ntiles,
                                                               int64_t* __restrict__ d_count)
{
  __shared__ int64_t s_part[kScanBlock];
  const int64_t chunk = (ntiles + kScanBlock - 1) / kScanBlock;
  const int64_t lo = (int64_t)threadIdx.x * chunk;
  const int64_t hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  int64_t sum = 0;
  for (int64_t t = lo; t < hi; t++) sum += counts[t];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  /* Hillis-Steele inclusive scan of the 1024 chunk sums */
  for (int d = 1; d < kScanBlock; d <<= 1) {
    const int64_t add = (int)threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
    __syncthreads();
    s_part[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t run = s_part[threadIdx.x] - sum;
  for (int64_t t = lo; t < hi; t++) {
    const int64_t c = counts[t];
    counts[t] = run;
    run += c;
  }
  if (threadIdx.x == kScanBlock - 1) *d_count = s_part[kScanBlock - 1];
}

template <bool KEYED>
__global__ __launch_bounds__(kRowsetBlock) void tile_write_kernel(
  const uint32_t* __restrict__ bits, int64_t nrows, int64_t ntiles, bool want_set,
  const int64_t* __restrict__ tile_base, int64_t* __restrict__ out,
  const int64_t* __restrict__ keys, int64_t* __restrict__ out_keys)
{
  __shared__ uint16_t s_local[kTileRows];  // 16 KiB: tile-local row numbers by rank
  __shared__ uint32_t s_wave[kRowsetBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t word = selected_word(bits, tile * kTileWords + threadIdx.x, nrows, want_set);
    const uint32_t c = (uint32_t)__popc(word);
    /* inclusive scan inside the wave */
    uint32_t incl = c;
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t rank = incl - c, total = 0;
    for (int k = 0; k < kRowsetBlock / kWave; k++) {
      if (k < wave) rank += s_wave[k];
      total += s_wave[k];
    }
    /* ascending inside the word: lowest bit first */
    while (word) {
      const int bit = __ffs((int)word) - 1;
      word &= word - 1;
      s_local[rank++] = (uint16_t)(threadIdx.x * 32 + bit);  // rank < total <= kTileRows
    }
    __syncthreads();
    const int64_t base = tile_base[tile];
    const int64_t row0 = tile * kTileRows;
    for (uint32_t k = threadIdx.x; k < total; k += kRowsetBlock) {
      const int64_t row = row0 + s_local[k];  // a set bit below nrows
      out[base + k] = row;
      if (KEYED) out_keys[base + k] = keys[row];
    }
    __syncthreads();  // s_local and s_wave are reused by the next tile
  }
}

int64_t select_tiles(int64_t nrows) { return (nrows + kTileRows - 1) / kTileRows; }

template <int MODE>
void launch_mark(const int64_t* d_idx, int64_t n, uint32_t* d_bits, hipStream_t s)
{
  int64_t blocks = (n + kRowsetBlock - 1) / kRowsetBlock;
  if (blocks > kRowsetGridCap) blocks = kRowsetGridCap;
  hipLaunchKernelGGL(mark_rows_kernel<MODE>, dim3((int)blocks), dim3(kRowsetBlock), 0, s, d_idx,
                     n, d_bits);
  DJ_HIP_CALL(hipGetLastError());
}

}  // namespace

void mark_rows(const int64_t* d_idx, int64_t n, uint32_t* d_bits, hipStream_t s, int mode)
{
  if (n <= 0) return;
  DJ_CHECK_ERROR(d_idx != nullptr && d_bits != nullptr, "mark_rows: null pointer");
  switch (mode) {
    case 0: launch_mark<0>(d_idx, n, d_bits, s); break;
    case kMarkMerge: launch_mark<kMarkMerge>(d_idx, n, d_bits, s); break;
    case kMarkCheck: launch_mark<kMarkCheck>(d_idx, n, d_bits, s); break;
    case kMarkMerge | kMarkCheck: launch_mark<kMarkMerge | kMarkCheck>(d_idx, n, d_bits, s); break;
    default: DJ_CHECK_ERROR(false, "mark_rows: unknown mode");
  }
}

int64_t select_rows_tile_rows() { return kTileRows; }

GridSpan rowset_grid_span(int family)
{
  switch (family) {
    case kSpanMarkRows: /* a thread per index */
      return {(int64_t)kRowsetGridCap * kRowsetBlock, 0};
    case kSpanSelectRows: /* a block per tile; tile_scan's chunk is 1 up to kScanBlock tiles */
      return {(int64_t)kRowsetGridCap * kTileRows, (int64_t)kScanBlock * kTileRows};
    default: return {0, 0};
  }
}

size_t select_rows_scratch_bytes(int64_t nrows)
{
  const int64_t ntiles = select_tiles(nrows > 0 ? nrows : 0);
  return (size_t)(ntiles > 0 ? ntiles : 1) * sizeof(int64_t);
}

namespace {

/* the three phases; d_keys / d_out_keys non-null selects the keyed write */
void select_impl(const uint32_t* d_bits, int64_t nrows, bool want_set, const int64_t* d_keys,
                 int64_t* d_out_idx, int64_t* d_out_keys, int64_t* d_count, hipStream_t s,
                 void* d_scratch)
{
  const int64_t ntiles = select_tiles(nrows);
  const int grid = (int)(ntiles < kRowsetGridCap ? ntiles : kRowsetGridCap);
  int64_t* tiles = (int64_t*)d_scratch;
  hipLaunchKernelGGL(tile_count_kernel, dim3(grid), dim3(kRowsetBlock), 0, s, d_bits, nrows,
                     ntiles, want_set, tiles);
  DJ_HIP_CALL(hipGetLastError());
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, tiles, ntiles, d_count);
  DJ_HIP_CALL(hipGetLastError());
  if (d_keys != nullptr)
    hipLaunchKernelGGL(tile_write_kernel<true>, dim3(grid), dim3(kRowsetBlock), 0, s, d_bits,
                       nrows, ntiles, want_set, (const int64_t*)tiles, d_out_idx, d_keys,
                       d_out_keys);
  else
    hipLaunchKernelGGL(tile_write_kernel<false>, dim3(grid), dim3(kRowsetBlock), 0, s, d_bits,
                       nrows, ntiles, want_set, (const int64_t*)tiles, d_out_idx,
                       (const int64_t*)nullptr, (int64_t*)nullptr);
  DJ_HIP_CALL(hipGetLastError());
}

}  // namespace

void select_rows(const uint32_t* d_bits, int64_t nrows, bool want_set, int64_t* d_out_idx,
                 int64_t* d_count, hipStream_t s, void* d_scratch)
{
  DJ_CHECK_ERROR(d_count != nullptr, "select_rows: null count pointer");
  if (nrows <= 0) {
    DJ_HIP_CALL(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
    return;
  }
  DJ_CHECK_ERROR(d_bits != nullptr && d_out_idx != nullptr && d_scratch != nullptr,
                 "select_rows: null pointer");
  select_impl(d_bits, nrows, want_set, nullptr, d_out_idx, nullptr, d_count, s, d_scratch);
}

void compact_keyed_rows(const uint32_t* d_bits, int64_t nrows, const int64_t* d_keys,
                        int64_t* d_out_idx, int64_t* d_out_keys, int64_t* d_count,
                        hipStream_t s, void* d_scratch)
{
  DJ_CHECK_ERROR(d_count != nullptr, "compact_keyed_rows: null count pointer");
  if (nrows <= 0) {
    DJ_HIP_CALL(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
    return;
  }
  DJ_CHECK_ERROR(d_bits != nullptr && d_keys != nullptr && d_out_idx != nullptr &&
                   d_out_keys != nullptr && d_scratch != nullptr,
                 "compact_keyed_rows: null pointer");
  select_impl(d_bits, nrows, true, d_keys, d_out_idx, d_out_keys, d_count, s, d_scratch);
}

}  // namespace dj
