/*
 * dj_cpp_api.hip — the C++ drop-in surface (include/distributed_join.hpp,
 * shuffle_on.hpp, all_to_all_comm.hpp, communicator.hpp,
 * distribute_table.hpp) over the gfx950 kernels in dj_kernels.hip and RCCL
 * over xGMI. See each public header for the reference interface mirrored.
 */
#include "dj_error.hpp"
#include "dj_kernels.hpp"
#include "dj_runtime.hpp"
#include "dj_timing.hpp"

#include "../../include/all_to_all_comm.hpp"
#include "../../include/communicator.hpp"
#include "../../include/compression.hpp"
#include "../../include/distribute_table.hpp"
#include "../../include/distributed_join.hpp"
#include "../../include/distributed_join.h"
#include "../../include/shuffle_on.hpp"

#include "dj_hash.h"
#include "dj_rng.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <iostream>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

/* ---------------------------------------------------------------- helpers */

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

/* small owning device buffer (pool-backed: hipMallocAsync on the compute
 * stream + host sync — the RMM-pool role of the reference's setup.cpp:51-67;
 * frees via hipFree, which device-syncs, keeping cross-stream reuse safe) */
/* Caching device allocator — the RMM-pool role of the reference's
 * setup.cpp:51-67. hipMalloc-backed, size-binned free list; freed blocks
 * are cached and reused (hipMalloc/hipFree per call would device-sync and
 * dominate the step time; ROCm's default hipMallocAsync mempool failed at
 * GB-scale blocks on gfx950). Reuse is safe because every free in this
 * layer happens after a host-synchronized phase boundary. */
class CachingAllocator {
 public:
  void* alloc(size_t bytes)
  {
    bytes = (bytes + 255) & ~(size_t)255;
    {
      std::lock_guard<std::mutex> g(m);
      auto it = free_list.lower_bound(bytes);
      if (it != free_list.end() && it->first <= bytes * 2 + (64 << 10)) {
        void* p = it->second;
        live[p] = it->first;
        free_list.erase(it);
        return p;
      }
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) {
      trim();
      e = hipMalloc(&p, bytes);
    }
    DJ_CHECK_ERROR(e == hipSuccess, "device allocator: out of memory");
    std::lock_guard<std::mutex> g(m);
    live[p] = bytes;
    return p;
  }
  void dealloc(void* p)
  {
    if (!p) return;
    std::lock_guard<std::mutex> g(m);
    auto it = live.find(p);
    DJ_CHECK_ERROR(it != live.end(), "device allocator: unknown pointer freed");
    free_list.emplace(it->second, p);
    live.erase(it);
  }
  void trim()
  {
    std::lock_guard<std::mutex> g(m);
    for (auto& kv : free_list) (void)hipFree(kv.second);
    free_list.clear();
  }

 private:
  std::mutex m;
  std::multimap<size_t, void*> free_list;
  std::unordered_map<void*, size_t> live;
};

CachingAllocator& pool()
{
  static CachingAllocator a;
  return a;
}

void* pool_alloc(size_t bytes) { return pool().alloc(bytes); }
void pool_free(void* p) { pool().dealloc(p); }

struct DBuf {
  void* p{nullptr};
  DBuf() = default;
  explicit DBuf(size_t bytes)
  {
    if (bytes) p = pool_alloc(bytes);
  }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DBuf& operator=(DBuf&& o) noexcept
  {
    if (this != &o) {
      pool_free(p);
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~DBuf() { pool_free(p); }
  int64_t* i64() { return (int64_t*)p; }
};

void sync_streams()
{
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_stream()));
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
}

/* one source range of dj::copy_bitmask_segments: nbits bits of `src` (nullptr
 * = all valid) from bit src_bit on; destination ranges follow one another */
struct BitSeg {
  const uint32_t* src;
  int64_t src_bit;
  int64_t nbits;
};

/* dst bits [0, sum nbits) = the segments back to back, on `st`. Returns the
 * device segment table, which must outlive the kernel: keep it until the
 * stream has been synchronized. */
DBuf copy_bit_segments(std::vector<BitSeg> const& segs, uint32_t* dst, hipStream_t st)
{
  const size_t S = segs.size();
  std::vector<int64_t> blk(3 * S + 1);
  int64_t total = 0;
  for (size_t i = 0; i < S; i++) {
    blk[i] = (int64_t)(uintptr_t)segs[i].src;
    blk[S + i] = segs[i].src_bit;
    blk[2 * S + i] = total;
    total += segs[i].nbits;
  }
  blk[3 * S] = total;
  DBuf d(blk.size() * 8);
  if (total > 0) {
    DJ_HIP_CALL(hipMemcpy(d.p, blk.data(), blk.size() * 8, hipMemcpyHostToDevice));
    dj::copy_bitmask_segments(d.p, (int)S, total, dst, st);
  }
  return d;
}

/* int64 view of a key column (widening INT32; spec: dj_hash.h operates on
 * int64 keys — INT32 keys are widened, identity placement k % G preserved) */
/* fused multi-column key: h_i = chain of mix64 over the key tuple — the
 * single-key engine then partitions/joins on h as if it were the key, and
 * the caller filters hash-collision false positives against the real
 * columns afterwards (local_inner_join). DJ_TEST_WEAK_FUSE collapses
 * h to 4 bits so tests can exercise that filter deterministically. */
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

bool is_string(cudf::column_view col) { return col.type().id() == cudf::type_id::STRING; }

/* dj::kKey* kind of an integer-rep key column; FLOAT32/FLOAT64 keys refuse
 * loudly (cuDF normalises -0.0/NaN before hashing float keys; that is not
 * implemented — INTEGRATION.md "Known restrictions") */
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

bool is_new_type(cudf::data_type t) { return (int)t.id() >= (int)cudf::type_id::INT16; }

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

/* bit c set: column c carries a validity mask (columns 0..31: callers refuse
 * a wider table that has any mask, see the AllToAllCommunicator constructor) */
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

/* -> DBuf of n fused int64 keys for the given key columns (<= 4; integer-rep
 * or STRING). A STRING column enters the chain as its dj_string_key64 row
 * hash (dj_strhash.h), computed into a temporary 64-bit column. */
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
    hipLaunchKernelGGL(fuse_keys_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, st, ptrs[0],
                       ptrs[1], ptrs[2], ptrs[3], kinds, (int)on.size(), n, weak, out.i64(),
                       masks[0], masks[1], masks[2], masks[3]);
    DJ_HIP_CALL(hipGetLastError());
    /* the row-hash temporaries go back to the pool on return */
    if (!str_keys.empty()) DJ_HIP_CALL(hipStreamSynchronize(st));
  }
  return out;
}

/* the engine's int64 view of an integer-rep key column: the column itself
 * when it is 64-bit, else widened on `st` into `dst` (col.size() int64s the
 * caller allocated — nothing is allocated here) */
const int64_t* key_as_i64(cudf::column_view col, int64_t* dst, hipStream_t st)
{
  const int kind = key_kind(col.type());
  if (kind == dj::kKeyI64) return col.head<int64_t>();
  hipLaunchKernelGGL(widen_key_kernel, dim3(grid_for_n(col.size())), dim3(kBlock), 0, st,
                     col.head<void>(), kind, (int64_t)col.size(), dst);
  return dst;
}

/* same on the compute stream, allocating `tmp` when the column needs widening */
const int64_t* key_as_i64(cudf::column_view col, DBuf& tmp)
{
  if (key_kind(col.type()) != dj::kKeyI64) tmp = DBuf((size_t)col.size() * 8);
  return key_as_i64(col, tmp.i64(), dj_rt_stream());
}

/* a table view over two INT64 device arrays */
cudf::table_view view_i64_pair(const void* c0, const void* c1, int64_t n)
{
  const cudf::data_type i64(cudf::type_id::INT64);
  return cudf::table_view({cudf::column_view(i64, (cudf::size_type)n, c0),
                           cudf::column_view(i64, (cudf::size_type)n, c1)});
}

/* the hot shape: exactly two INT64 columns, one of them the key, and no
 * validity mask (a table with any mask takes the general paths) */
bool is_i64_pair(cudf::table_view t, cudf::size_type key_col)
{
  return t.num_columns() == 2 && (key_col == 0 || key_col == 1) &&
         t.column(0).type().id() == cudf::type_id::INT64 &&
         t.column(1).type().id() == cudf::type_id::INT64 && !t.column(0).nullable() &&
         !t.column(1).nullable();
}

/* both sides of a join have it with the key in front: the engine's four
 * outputs then ARE the result columns (payloads travel through the join) */
bool joins_i64_pairs(cudf::table_view left, cudf::table_view right, cudf::size_type left_key,
                     cudf::size_type right_key)
{
  return left_key == 0 && right_key == 0 && is_i64_pair(left, 0) && is_i64_pair(right, 0);
}

void validate_compression(std::vector<ColumnCompressionOptions> const& opts)
{
  for (auto& o : opts) {
    if (!o.children_compression_options.empty())
      validate_compression(o.children_compression_options);
    if (o.compression_method == CompressionMethod::none) continue;
    if (o.compression_method == CompressionMethod::lz4)
      throw std::runtime_error("lz4 compression is not implemented (cascaded or none)");
    if (o.cascaded_format.num_RLEs < 0 || o.cascaded_format.num_RLEs > 1)
      throw std::runtime_error("cascaded num_RLEs must be 0 or 1 (one RLE pass; "
                               "dj_compress.hip wire format)");
    if (o.cascaded_format.num_deltas < 0 || o.cascaded_format.num_deltas > 1)
      throw std::runtime_error("cascaded num_deltas must be 0 or 1");
  }
}
/* typed check: like the reference's cascaded dispatch (declared for the
 * signed/unsigned integer types only), FLOAT32/FLOAT64/BOOL8 columns refuse
 * a cascaded option instead of packing their bit patterns */
void validate_compression(cudf::table_view t, std::vector<ColumnCompressionOptions> const& opts)
{
  validate_compression(opts);
  for (cudf::size_type c = 0; c < t.num_columns() && (size_t)c < opts.size(); c++) {
    const cudf::data_type ty = t.column(c).type();
    if (opts[c].compression_method == CompressionMethod::cascaded &&
        ty.id() != cudf::type_id::STRING && !cudf::is_cascaded_supported(ty))
      throw std::runtime_error("Unsupported type for cascaded compressor");
  }
}
/* The GENERIC plan API (append_to_all_to_all_comm_buffers + all_to_all_comm
 * + postprocess_all_to_all_comm) refuses cascaded options BY DESIGN, not as
 * a stub: the reference exchanges compressed slice sizes over an MPI
 * side-channel while the caller's NCCL group is open
 * (all_to_all_comm.cpp:420-478 + communicate_sizes via MPI); RCCL has no
 * such side-channel, and grouped p2p cannot post data recvs whose counts
 * arrive in the same group. Compressed wires therefore run through the
 * self-contained paths — AllToAllCommunicator::launch_communication,
 * shuffle_on, distributed_inner_join — which own their group discipline
 * and DO execute cascaded end to end (the paths the reference's benchmarks
 * exercise). See INTEGRATION.md "Known restrictions". */
void check_no_compression(std::vector<ColumnCompressionOptions> const& opts)
{
  for (auto& o : opts)
    if (o.compression_method != CompressionMethod::none)
      throw std::runtime_error(
        "this entry point executes uncompressed buffers only; use "
        "AllToAllCommunicator::launch_communication for cascaded compression");
}

Communicator* g_default_comm = nullptr;

/* size-1 stand-in so the C++ API works single-process without RCCL */
class LocalCommunicator : public Communicator {
 public:
  LocalCommunicator()
  {
    mpi_rank = 0;
    mpi_size = 1;
  }
  void initialize() override {}
  void start() override {}
  void stop() override { sync_streams(); }
  void send(const void*, int64_t, int, int) override
  {
    DJ_CHECK_ERROR(false, "LocalCommunicator cannot send (single process)");
  }
  void recv(void*, int64_t, int, int) override
  {
    DJ_CHECK_ERROR(false, "LocalCommunicator cannot recv (single process)");
  }
  void finalize() override {}
  bool group_by_batch() override { return true; }
};

}  // namespace

/* this file's row kernels (grid_for_n): a thread per row (dj_kernels.hpp) */
dj::GridSpan dj::key_helper_grid_span(int family)
{
  if (family == dj::kSpanKeyHelpers) return {(int64_t)kGridCap * kBlock, 0};
  return {0, 0};
}

/* --------------------------------------------------------- cudf::column */

namespace cudf {

column::column(data_type type, size_type size) : _type(type), _size(size)
{
  size_t bytes = (size_t)size * size_of(type);
  if (bytes) _data = pool_alloc(bytes);
}

column::column(data_type type, size_type size, void* adopt) : _type(type), _size(size), _data(adopt)
{
}

column::column(size_type size, int64_t chars_bytes)
  : _type(data_type(type_id::STRING)), _size(size), _chars_size(chars_bytes)
{
  _data = pool_alloc(((size_t)size + 1) * sizeof(int32_t));
  /* an empty STRING column is complete as built: offsets = {0} */
  if (size == 0) DJ_HIP_CALL(hipMemset(_data, 0, sizeof(int32_t)));
  if (chars_bytes) _chars = pool_alloc((size_t)chars_bytes);
}

column::column(column&& o) noexcept
  : _type(o._type),
    _size(o._size),
    _data(o._data),
    _chars(o._chars),
    _chars_size(o._chars_size),
    _null_mask(o._null_mask),
    _null_count(o._null_count)
{
  o._data = nullptr;
  o._chars = nullptr;
  o._size = 0;
  o._chars_size = 0;
  o._null_mask = nullptr;
  o._null_count = 0;
}

column& column::operator=(column&& o) noexcept
{
  if (this != &o) {
    if (_data) pool_free(_data);
    if (_chars) pool_free(_chars);
    if (_null_mask) pool_free(_null_mask);
    _type = o._type;
    _size = o._size;
    _data = o._data;
    _chars = o._chars;
    _chars_size = o._chars_size;
    _null_mask = o._null_mask;
    _null_count = o._null_count;
    o._data = nullptr;
    o._chars = nullptr;
    o._size = 0;
    o._chars_size = 0;
    o._null_mask = nullptr;
    o._null_count = 0;
  }
  return *this;
}

column::~column()
{
  if (_data) pool_free(_data);
  if (_chars) pool_free(_chars);
  if (_null_mask) pool_free(_null_mask);
}

void column::set_null_mask(void* adopt, size_type null_count)
{
  if (_null_mask && _null_mask != adopt) pool_free(_null_mask);
  _null_mask = (bitmask_type*)adopt;
  _null_count = adopt ? null_count : 0;
}

bitmask_type* column::allocate_null_mask()
{
  /* never empty, so that a 0-row column can still be nullable() */
  set_null_mask(pool_alloc(std::max<size_t>(bitmask_allocation_size_bytes(_size), 64)),
                UNKNOWN_NULL_COUNT);
  return _null_mask;
}

size_type column::null_count() const
{
  if (_null_count != UNKNOWN_NULL_COUNT) return _null_count;
  if (_null_mask == nullptr || _size == 0) return _null_count = 0;
  hipStream_t st = dj_rt_stream();
  DBuf cnt(8);
  DJ_HIP_CALL(hipMemsetAsync(cnt.p, 0, 8, st));
  dj::count_unset_bits(_null_mask, _size, (unsigned long long*)cnt.p, st);
  unsigned long long h = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&h, cnt.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return _null_count = (size_type)h;
}

}  // namespace cudf

/* ----------------------------------------------------------- Communicator */

struct RCCLCommunicatorImpl {
  ncclComm_t comm{nullptr};
  hipStream_t stream{nullptr};
};

int rccl_unique_id_size() { return (int)sizeof(ncclUniqueId); }

void rccl_unique_id(void* out_bytes)
{
  ncclUniqueId id;
  DJ_RCCL_CALL(ncclGetUniqueId(&id));
  memcpy(out_bytes, &id, sizeof(id));
}

RCCLCommunicator::RCCLCommunicator(int rank, int size, const void* id_bytes)
{
  impl = new RCCLCommunicatorImpl;
  mpi_rank = rank;
  mpi_size = size;
  DJ_HIP_CALL(hipGetDevice(&current_device));
  ncclUniqueId id;
  memcpy(&id, id_bytes, sizeof(id));
  DJ_RCCL_CALL(ncclCommInitRank(&impl->comm, size, id, rank));
  impl->stream = dj_rt_comm_stream();
  g_default_comm = this;
}

void RCCLCommunicator::initialize() {}

void RCCLCommunicator::start() { DJ_RCCL_CALL(ncclGroupStart()); }

void RCCLCommunicator::stop()
{
  DJ_RCCL_CALL(ncclGroupEnd());
  DJ_HIP_CALL(hipStreamSynchronize(impl->stream));
}

void RCCLCommunicator::send(const void* buf, int64_t count, int element_size, int dest)
{
  if (count <= 0) return;
  DJ_RCCL_CALL(ncclSend(buf, (size_t)count * element_size, ncclInt8, dest, impl->comm,
                        impl->stream));
}

void RCCLCommunicator::recv(void* buf, int64_t count, int element_size, int source)
{
  if (count <= 0) return;
  DJ_RCCL_CALL(ncclRecv(buf, (size_t)count * element_size, ncclInt8, source, impl->comm,
                        impl->stream));
}

void RCCLCommunicator::finalize()
{
  if (impl->comm) {
    DJ_RCCL_CALL(ncclCommDestroy(impl->comm));
    impl->comm = nullptr;
  }
}

RCCLCommunicator::~RCCLCommunicator()
{
  if (g_default_comm == this) g_default_comm = nullptr;
  delete impl;
}

Communicator* default_communicator()
{
  static LocalCommunicator local;
  return g_default_comm ? g_default_comm : &local;
}

/* ------------------------------------------------------------ compression */

std::vector<ColumnCompressionOptions> generate_compression_options_distributed(
  cudf::table_view input, bool compression)
{
  if (!compression)
    return std::vector<ColumnCompressionOptions>(
      (size_t)input.num_columns(), ColumnCompressionOptions(CompressionMethod::none));
  /* fixed policy standing in for the reference's nvcomp auto-selector
   * (compression.hpp:253-292): bitpack-only cascaded for fixed-width columns
   * and the row-size wire of STRING columns; chars are never compressed
   * (reference policy, compression.cpp:44-60) */
  std::vector<ColumnCompressionOptions> opts;
  nvcompCascadedFormatOpts bp{};
  bp.num_RLEs = 0;
  bp.num_deltas = 0;
  bp.use_bp = 1;
  for (cudf::size_type c = 0; c < input.num_columns(); c++) {
    const cudf::data_type ty = input.column(c).type();
    if (ty.id() == cudf::type_id::STRING || cudf::is_cascaded_supported(ty))
      opts.emplace_back(CompressionMethod::cascaded, bp);
    else
      opts.emplace_back(CompressionMethod::none);  // FLOAT32/FLOAT64/BOOL8
  }
  return opts;
}

std::vector<ColumnCompressionOptions> generate_none_compression_options(cudf::table_view input)
{
  std::vector<ColumnCompressionOptions> opts;
  for (cudf::size_type c = 0; c < input.num_columns(); c++) {
    if (input.column(c).type().id() == cudf::type_id::STRING) {
      std::vector<ColumnCompressionOptions> kids(
        2, ColumnCompressionOptions(CompressionMethod::none));
      opts.emplace_back(CompressionMethod::none, nvcompCascadedFormatOpts{}, kids);
    } else {
      opts.emplace_back(CompressionMethod::none);
    }
  }
  return opts;
}

namespace {

/* sampling selector over our executable cascaded schemes ({0|1 RLE} x
 * {0|1 deltas} + bitpack): picks the scheme with the smaller estimated
 * packed total on a host-side sample, in the role of nvcomp's
 * CascadedSelector (reference compression.hpp:253-292,
 * compression.cpp:36-69). Selection is data-dependent, not parity-pinned
 * (nvcomp is absent). */
nvcompCascadedFormatOpts select_cascaded_on_sample(const void* d_data, int64_t n, int esize)
{
  nvcompCascadedFormatOpts o{};
  o.use_bp = 1;
  const int64_t sample = std::min<int64_t>(n, 65536);
  if (sample < 2) return o;
  std::vector<int64_t> h((size_t)sample);
  if (esize == 8) {
    DJ_HIP_CALL(hipMemcpy(h.data(), d_data, (size_t)sample * 8, hipMemcpyDeviceToHost));
  } else {
    /* narrower elements enter as the codec loads them: sign-extended */
    std::vector<int8_t> raw((size_t)sample * esize);
    DJ_HIP_CALL(hipMemcpy(raw.data(), d_data, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < sample; i++)
      h[(size_t)i] = esize == 4   ? (int64_t)((const int32_t*)raw.data())[i]
                     : esize == 2 ? (int64_t)((const int16_t*)raw.data())[i]
                                  : (int64_t)raw[(size_t)i];
  }
  auto zigzag = [](int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); };
  auto packed_bits = [&](const std::vector<int64_t>& v, bool delta) {
    uint64_t total = 0;
    const int64_t m = (int64_t)v.size();
    for (int64_t g = 0; g < m; g += 32) {
      int w = 0;
      const int64_t e = std::min<int64_t>(g + 32, m);
      for (int64_t i = g; i < e; i++) {
        int64_t d = delta ? (i ? v[(size_t)i] - v[(size_t)i - 1] : v[0]) : v[(size_t)i];
        uint64_t z = zigzag(d) | 1;
        w = std::max(w, 64 - __builtin_clzll(z));
      }
      total += (uint64_t)w * 32;
    }
    return total;
  };
  /* RLE candidate: run values + run lengths on the sample */
  std::vector<int64_t> rvals, rlens;
  rvals.reserve((size_t)sample);
  for (int64_t i = 0; i < sample; i++) {
    if (i == 0 || h[(size_t)i] != h[(size_t)i - 1]) {
      rvals.push_back(h[(size_t)i]);
      rlens.push_back(1);
    } else {
      rlens.back()++;
    }
  }
  struct Cand {
    int rle, delta;
    uint64_t bits;
  };
  std::vector<Cand> cands;
  cands.push_back({0, 0, packed_bits(h, false)});
  cands.push_back({0, 1, packed_bits(h, true)});
  if ((int64_t)rvals.size() * 2 < sample) {  // only worth considering on runs
    uint64_t lbits = packed_bits(rlens, false);
    cands.push_back({1, 0, packed_bits(rvals, false) + lbits});
    cands.push_back({1, 1, packed_bits(rvals, true) + lbits});
  }
  const Cand* best = &cands[0];
  for (const auto& c : cands)
    if (c.bits < best->bits) best = &c;
  o.num_RLEs = best->rle;
  o.num_deltas = best->delta;
  return o;
}

}  // namespace

std::vector<ColumnCompressionOptions> generate_auto_select_compression_options(
  cudf::table_view input_table)
{
  /* reference compression.cpp:36-69: per-column sampling selection; STRING
   * columns: select on the offsets child, never compress chars */
  std::vector<ColumnCompressionOptions> opts;
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    cudf::column_view col = input_table.column(c);
    if (col.type().id() == cudf::type_id::STRING) {
      std::vector<ColumnCompressionOptions> kids;
      kids.emplace_back(
        CompressionMethod::cascaded,
        select_cascaded_on_sample(col.child(0).head<int32_t>(), col.size() + 1, 4));
      kids.emplace_back(CompressionMethod::none);
      opts.emplace_back(CompressionMethod::none, nvcompCascadedFormatOpts{}, kids);
    } else if (!cudf::is_cascaded_supported(col.type())) {
      /* FLOAT32/FLOAT64/BOOL8: not cascaded-supported, as in the reference */
      opts.emplace_back(CompressionMethod::none);
    } else {
      opts.emplace_back(
        CompressionMethod::cascaded,
        select_cascaded_on_sample(col.head<char>(), col.size(), cudf::size_of(col.type())));
    }
  }
  return opts;
}

ColumnCompressionOptions broadcast_compression_options(cudf::column_view input_column,
                                                       ColumnCompressionOptions input_options,
                                                       Communicator* comm)
{
  /* reference compression.cpp:95-130 used MPI_Bcast on MPI_COMM_WORLD; here
   * rank 0's choices travel over the given Communicator (grouped send/recv
   * of a POD through device staging — RCCL transports device buffers
   * only) */
  struct Pod {
    int method, rles, deltas, bp;
  };
  Pod pod{(int)input_options.compression_method, input_options.cascaded_format.num_RLEs,
          input_options.cascaded_format.num_deltas, input_options.cascaded_format.use_bp};
  if (comm->mpi_size > 1) {
    DBuf stage(sizeof(Pod));
    if (comm->mpi_rank == 0)
      DJ_HIP_CALL(hipMemcpy(stage.p, &pod, sizeof(Pod), hipMemcpyHostToDevice));
    comm->start();
    if (comm->mpi_rank == 0) {
      for (int r = 1; r < comm->mpi_size; r++) comm->send(stage.p, sizeof(Pod), 1, r);
    } else {
      comm->recv(stage.p, sizeof(Pod), 1, 0);
    }
    comm->stop();
    DJ_HIP_CALL(hipMemcpy(&pod, stage.p, sizeof(Pod), hipMemcpyDeviceToHost));
  }
  nvcompCascadedFormatOpts fmt{};
  fmt.num_RLEs = pod.rles;
  fmt.num_deltas = pod.deltas;
  fmt.use_bp = pod.bp;
  std::vector<ColumnCompressionOptions> kids;
  if (input_column.type().id() == cudf::type_id::STRING) {
    for (size_t k = 0; k < 2; k++) {
      ColumnCompressionOptions child;
      if (comm->mpi_rank == 0) {
        DJ_CHECK_ERROR(input_options.children_compression_options.size() == 2,
                       "STRING compression options need 2 children");
        child = input_options.children_compression_options[k];
      }
      kids.push_back(broadcast_compression_options(input_column.child((cudf::size_type)k),
                                                   child, comm));
    }
  }
  return ColumnCompressionOptions((CompressionMethod)pod.method, fmt, kids);
}

std::vector<ColumnCompressionOptions> broadcast_compression_options(
  cudf::table_view input_table, std::vector<ColumnCompressionOptions> input_options,
  Communicator* comm)
{
  std::vector<ColumnCompressionOptions> out;
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    ColumnCompressionOptions col_opts;
    if (comm->mpi_rank == 0) col_opts = input_options[(size_t)c];
    out.push_back(broadcast_compression_options(input_table.column(c), col_opts, comm));
  }
  return out;
}

ColumnCompressionOptions broadcast_compression_options(cudf::column_view input_column,
                                                       ColumnCompressionOptions input_options)
{
  return broadcast_compression_options(input_column, input_options, default_communicator());
}

std::vector<ColumnCompressionOptions> broadcast_compression_options(
  cudf::table_view input_table, std::vector<ColumnCompressionOptions> input_options)
{
  return broadcast_compression_options(input_table, input_options, default_communicator());
}

/* ------------------------------------------------------ CommunicationGroup */

CommunicationGroup::CommunicationGroup(int grid_size, int stride)
  : CommunicationGroup(grid_size, stride, default_communicator()->mpi_rank)
{
}

CommunicationGroup::CommunicationGroup(int grid_size_, int stride_, int mpi_rank_)
  : mpi_rank(mpi_rank_), grid_size(grid_size_), stride(stride_)
{
  DJ_CHECK_ERROR(stride > 0 && grid_size % stride == 0,
                 "Group size should be a multiple of stride");
  group_start = mpi_rank / grid_size * grid_size + mpi_rank % stride;
}

/* ------------------------------------------------------- communicate_sizes */

namespace {

/* communicate_sizes, optionally carrying `extra` (33 bits) above bit 30 of
 * every count: the internal exchange of AllToAllCommunicator, whose counts
 * are size_type rows, agrees on column nullability this way without a
 * message of its own. peer_extra (G entries) receives every rank's word. */
void exchange_sizes(std::vector<int64_t> const& send_offset, std::vector<int64_t>& recv_offset,
                    CommunicationGroup comm_group, Communicator* communicator, bool fold,
                    uint64_t extra, std::vector<uint64_t>* peer_extra)
{
  const int G = comm_group.size();
  const int me = comm_group.get_local_idx();
  std::vector<int64_t> send_counts(G);
  for (int i = 0; i < G; i++) {
    send_counts[i] = send_offset[i + 1] - send_offset[i];
    if (fold) {
      DJ_CHECK_ERROR(send_counts[i] >= 0 && send_counts[i] <= (int64_t)INT32_MAX,
                     "all-to-all: a slice's row count exceeds size_type");
      if (i != me) send_counts[i] |= (int64_t)(extra << 31);
    }
  }
  std::vector<int64_t> recv_counts(G, 0);
  recv_counts[me] = send_counts[me];
  if (peer_extra) {
    peer_extra->assign(G, 0);
    (*peer_extra)[me] = extra;
  }
  if (G > 1) {
    /* counts move through the communicator via a small device staging
     * buffer (the reference kept them on MPI host buffers,
     * all_to_all_comm.cpp:68-69; RCCL wants device memory) */
    DBuf d_send((size_t)G * 8), d_recv((size_t)G * 8);
    DJ_HIP_CALL(hipMemcpyAsync(d_send.p, send_counts.data(), (size_t)G * 8,
                               hipMemcpyHostToDevice, dj_rt_comm_stream()));
    DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
    communicator->start();
    for (int i = 0; i < G; i++) {
      if (i == me) continue;
      int peer = comm_group.get_global_rank(i);
      communicator->send(d_send.i64() + i, 1, 8, peer);
      communicator->recv(d_recv.i64() + i, 1, 8, peer);
    }
    communicator->stop();
    std::vector<int64_t> got(G);
    DJ_HIP_CALL(hipMemcpyAsync(got.data(), d_recv.p, (size_t)G * 8, hipMemcpyDeviceToHost,
                               dj_rt_comm_stream()));
    DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
    for (int i = 0; i < G; i++) {
      if (i == me) continue;
      recv_counts[i] = fold ? (got[i] & (int64_t)0x7FFFFFFF) : got[i];
      if (fold && peer_extra) (*peer_extra)[i] = (uint64_t)got[i] >> 31;
    }
  }
  recv_offset.resize(G + 1);
  recv_offset[0] = 0;
  for (int i = 0; i < G; i++) recv_offset[i + 1] = recv_offset[i] + recv_counts[i];
}

}  // namespace

void communicate_sizes(std::vector<int64_t> const& send_offset,
                       std::vector<int64_t>& recv_offset,
                       CommunicationGroup comm_group,
                       Communicator* communicator)
{
  exchange_sizes(send_offset, recv_offset, comm_group, communicator, false, 0, nullptr);
}

void communicate_sizes(std::vector<cudf::size_type> const& send_offset,
                       std::vector<int64_t>& recv_offset,
                       CommunicationGroup comm_group,
                       Communicator* communicator)
{
  std::vector<int64_t> wide(send_offset.begin(), send_offset.end());
  communicate_sizes(wide, recv_offset, comm_group, communicator);
}

void warmup_all_to_all(Communicator* communicator)
{
  /* mirrors all_to_all_comm.cpp:191-233: a throwaway all-to-all to
   * establish RCCL channels before the timed region */
  const int G = communicator->mpi_size;
  if (G <= 1) return;
  const int64_t per_peer = 1 << 18;
  DBuf d_send((size_t)G * per_peer * 8), d_recv((size_t)G * per_peer * 8);
  communicator->start();
  for (int p = 0; p < G; p++) {
    if (p == communicator->mpi_rank) continue;
    communicator->send(d_send.i64() + p * per_peer, per_peer, 8, p);
    communicator->recv(d_recv.i64() + p * per_peer, per_peer, 8, p);
  }
  communicator->stop();
}

/* --------------------------------------------------------- all_to_all plan */

void append_to_all_to_all_comm_buffers(cudf::table_view input,
                                       cudf::mutable_table_view output,
                                       std::vector<cudf::size_type> const& send_offsets,
                                       std::vector<int64_t> const& recv_offsets,
                                       std::vector<AllToAllCommBuffer>& all_to_all_comm_buffers,
                                       std::vector<ColumnCompressionOptions> compression_options)
{
  check_no_compression(compression_options);
  check_no_masks(input, "append_to_all_to_all_comm_buffers");
  for (cudf::size_type c = 0; c < input.num_columns(); c++) {
    DJ_CHECK_ERROR(cudf::size_of(input.column(c).type()) > 0,
                   "all-to-all: fixed-width columns only through the generic plan API");
    std::vector<int64_t> soff(send_offsets.begin(), send_offsets.end());
    all_to_all_comm_buffers.emplace_back(
      input.column(c).head<int8_t>(), output.column(c).head<int8_t>(), soff, recv_offsets,
      input.column(c).type(), compression_options[c].compression_method,
      compression_options[c].cascaded_format);
  }
}

void all_to_all_comm(std::vector<AllToAllCommBuffer>& all_to_all_comm_buffers,
                     CommunicationGroup comm_group,
                     Communicator* communicator,
                     bool include_current_rank,
                     bool report_timing,
                     void* preallocated_pinned_buffer)
{
  (void)report_timing;
  (void)preallocated_pinned_buffer;
  const int G = comm_group.size();
  const int me = comm_group.get_local_idx();
  for (auto& buf : all_to_all_comm_buffers) {
    const int esize = cudf::size_of(buf.dtype);
    for (int i = 0; i < G; i++) {
      int64_t scount = buf.send_offsets[i + 1] - buf.send_offsets[i];
      int64_t rcount = buf.recv_offsets[i + 1] - buf.recv_offsets[i];
      const int8_t* src = (const int8_t*)buf.send_buffer + buf.send_offsets[i] * esize;
      int8_t* dst = (int8_t*)buf.recv_buffer + buf.recv_offsets[i] * esize;
      if (i == me) {
        if (include_current_rank && scount > 0) {
          /* self-partition: direct D2D on the comm stream (the reference's
           * explicit copy, all_to_all_comm.cpp:610-653) */
          DJ_HIP_CALL(hipMemcpyAsync(dst, src, (size_t)scount * esize,
                                     hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
        }
        continue;
      }
      int peer = comm_group.get_global_rank(i);
      communicator->send(src, scount, esize, peer);
      communicator->recv(dst, rcount, esize, peer);
    }
  }
}

void postprocess_all_to_all_comm(std::vector<AllToAllCommBuffer>& all_to_all_comm_buffers,
                                 CommunicationGroup comm_group,
                                 Communicator* communicator,
                                 bool include_current_rank,
                                 bool report_timing)
{
  /* nothing to do: the generic plan path transfers raw buffers only
   * (cascaded refused at append — see check_no_compression above); string
   * columns and compressed wires run through launch_communication, which
   * does its own receiver-side decompress + offsets rebuild */
  (void)all_to_all_comm_buffers;
  (void)comm_group;
  (void)communicator;
  (void)include_current_rank;
  (void)report_timing;
}

/* ---------------------------------------------------- AllToAllCommunicator */

/* per string column: char-offset boundaries per peer + device row-size
 * buffers (reference all_to_all_comm.hpp:349-360 members; sizes, not
 * offsets, go on the wire — offsets rebuilt receiver-side by scan,
 * strings_column.cu:111-131) */
struct AllToAllCommunicator::StringsState {
  std::vector<std::vector<int64_t>> send_char_offsets;  // [col][G+1]
  std::vector<std::vector<int64_t>> recv_char_offsets;  // [col][G+1]
  std::vector<DBuf> sizes_to_send;                      // [col] int32[n]
  std::vector<DBuf> sizes_received;                     // [col] int32[n_recv]
};

AllToAllCommunicator::AllToAllCommunicator(
  cudf::table_view input_table_,
  std::vector<cudf::size_type> offsets,
  CommunicationGroup comm_group_,
  Communicator* communicator_,
  std::vector<ColumnCompressionOptions> compression_options_,
  bool explicit_copy_to_current_rank_)
  : AllToAllCommunicator(input_table_, std::move(offsets), comm_group_, communicator_,
                         std::move(compression_options_), explicit_copy_to_current_rank_, 0u)
{
}

AllToAllCommunicator::AllToAllCommunicator(
  cudf::table_view input_table_,
  std::vector<cudf::size_type> offsets,
  CommunicationGroup comm_group_,
  Communicator* communicator_,
  std::vector<ColumnCompressionOptions> compression_options_,
  bool explicit_copy_to_current_rank_,
  uint32_t route_tag)
  : input_table(input_table_),
    comm_group(comm_group_),
    communicator(communicator_),
    explicit_copy_to_current_rank(explicit_copy_to_current_rank_),
    send_offsets(std::move(offsets)),
    compression_options(std::move(compression_options_))
{
  validate_compression(input_table, compression_options);
  DJ_CHECK_ERROR((int)send_offsets.size() == comm_group.size() + 1,
                 "AllToAllCommunicator: offsets must have comm_group.size()+1 entries");
  /* row counts, with this rank's per-column nullability (and the caller's
   * route tag) folded above them: the ranks must agree on which columns ship
   * a mask, or the slice sizes of the exchange would not pair up. A column
   * is shipped with a mask when it has one on ANY rank of the group; a rank
   * whose column has none sends all-valid slices. */
  {
    const int ncols = input_table.num_columns();
    DJ_CHECK_ERROR(!any_nullable(input_table) || ncols <= dj::kMaxSchemaCols,
                   "all-to-all: nullable columns need a table of at most 32 columns");
    const uint32_t my_bits = nullable_bits(input_table);
    DJ_CHECK_ERROR(!(route_tag & 2u) || ncols < 32, "all-to-all: route tag needs a free bit");
    const uint64_t extra = (uint64_t)(route_tag & 1u) | ((uint64_t)my_bits << 1) |
                           ((uint64_t)((route_tag >> 1) & 1u) << 32);
    std::vector<int64_t> wide(send_offsets.begin(), send_offsets.end());
    std::vector<uint64_t> peers;
    exchange_sizes(wide, recv_offsets, comm_group, communicator, true, extra, &peers);
    const uint32_t col_bits = ncols >= 32 ? 0xFFFFFFFFu : ((1u << ncols) - 1u);
    for (uint64_t e : peers) {
      nullable_cols |= (uint32_t)(e >> 1) & col_bits;
      const uint32_t tag = (uint32_t)(e & 1u) | (ncols < 32 ? (uint32_t)((e >> 32) & 1u) << 1 : 0u);
      DJ_CHECK_ERROR(tag == route_tag,
                     "all-to-all: the ranks of the group passed different route tags. In "
                     "distributed_inner_join this means they disagree on whether a key column "
                     "(or a column of a 2 x INT64 table) is nullable, which selects the join "
                     "route; pass a mask (all valid) for that column on every rank");
    }
  }

  /* strings columns: exchange per-peer char byte counts; precompute the row
   * sizes to send (gather_string_offsets + calculate_string_sizes_from_offsets
   * roles, strings_column.cu:39-109) */
  const int G = comm_group.size();
  const int64_t n = input_table.num_rows();
  const int64_t n_recv = recv_offsets.back();
  hipStream_t st = dj_rt_stream();
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    if (input_table.column(c).type().id() != cudf::type_id::STRING) {
      if (strings) {
        strings->send_char_offsets.emplace_back();
        strings->recv_char_offsets.emplace_back();
        strings->sizes_to_send.emplace_back();
        strings->sizes_received.emplace_back();
      }
      continue;
    }
    if (!strings) {
      strings = std::make_shared<StringsState>();
      for (cudf::size_type cc = 0; cc < c; cc++) {
        strings->send_char_offsets.emplace_back();
        strings->recv_char_offsets.emplace_back();
        strings->sizes_to_send.emplace_back();
        strings->sizes_received.emplace_back();
      }
    }
    auto col = input_table.column(c);
    /* row sizes first: launch_communication copies the self slice of them on
     * the COMM stream, which is not ordered after this compute-stream
     * kernel — the stream syncs of the boundary reads below complete it
     * before the constructor returns */
    DBuf sizes((size_t)(n > 0 ? n : 1) * 4);
    dj::sizes_from_offsets(col.head<int32_t>(), n, (int32_t*)sizes.p, st);
    /* char offsets at the G+1 send row boundaries */
    std::vector<int64_t> soff(G + 1);
    for (int k = 0; k <= G; k++) {
      int32_t v = 0;
      DJ_HIP_CALL(hipMemcpyAsync(&v, col.head<int32_t>() + send_offsets[k], 4,
                                 hipMemcpyDeviceToHost, st));
      DJ_HIP_CALL(hipStreamSynchronize(st));
      soff[k] = v;
    }
    std::vector<int64_t> roff;
    communicate_sizes(soff, roff, comm_group, communicator);
    /* the received column keeps the int32 offsets convention: refuse loudly
     * if the gathered slices' chars exceed it (same cap as the reference's
     * cuDF 0.19; the receiver-side scan would otherwise wrap) */
    DJ_CHECK_ERROR(roff.empty() || roff.back() <= (int64_t)INT32_MAX,
                   "all-to-all: received string chars exceed 2^31 (int32 offsets limit)");
    strings->send_char_offsets.push_back(std::move(soff));
    strings->recv_char_offsets.push_back(std::move(roff));
    strings->sizes_to_send.push_back(std::move(sizes));
    strings->sizes_received.push_back(DBuf((size_t)(n_recv > 0 ? n_recv : 1) * 4));
  }
  (void)st;
}

AllToAllCommunicator::AllToAllCommunicator(
  cudf::table_view input_table_,
  std::vector<cudf::size_type> offsets,
  Communicator* communicator_,
  std::vector<ColumnCompressionOptions> compression_options_,
  bool explicit_copy_to_current_rank_)
  : AllToAllCommunicator(input_table_,
                         std::move(offsets),
                         CommunicationGroup(communicator_->mpi_size, 1, communicator_->mpi_rank),
                         communicator_,
                         std::move(compression_options_),
                         explicit_copy_to_current_rank_)
{
}

std::unique_ptr<cudf::table> AllToAllCommunicator::allocate_communicated_table()
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  cudf::size_type nrows = (cudf::size_type)recv_offsets.back();
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    if (input_table.column(c).type().id() == cudf::type_id::STRING)
      cols.push_back(std::make_unique<cudf::column>(
        nrows, strings->recv_char_offsets[c].back()));
    else
      cols.push_back(std::make_unique<cudf::column>(input_table.column(c).type(), nrows));
    /* filled by launch_communication's merge, self slice included */
    if ((nullable_cols >> c) & 1u) cols.back()->allocate_null_mask();
  }
  auto out = std::make_unique<cudf::table>(std::move(cols));
  if (explicit_copy_to_current_rank) {
    /* copy the self partition now, outside launch_communication, so the
     * comm phase moves only remote slices (all_to_all_comm.cpp:701-729) */
    const int me = comm_group.get_local_idx();
    for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
      int64_t scount = (int64_t)send_offsets[me + 1] - send_offsets[me];
      if (scount <= 0) continue;
      if (input_table.column(c).type().id() == cudf::type_id::STRING) {
        /* self slice of row SIZES into sizes_received + chars slice */
        DJ_HIP_CALL(hipMemcpyAsync(
          (int32_t*)strings->sizes_received[c].p + recv_offsets[me],
          (const int32_t*)strings->sizes_to_send[c].p + send_offsets[me],
          (size_t)scount * 4, hipMemcpyDeviceToDevice, dj_rt_stream()));
        int64_t cbytes =
          strings->send_char_offsets[c][me + 1] - strings->send_char_offsets[c][me];
        if (cbytes > 0)
          DJ_HIP_CALL(hipMemcpyAsync(
            (uint8_t*)out->get_column(c).chars() + strings->recv_char_offsets[c][me],
            (const uint8_t*)input_table.column(c).chars() +
              strings->send_char_offsets[c][me],
            (size_t)cbytes, hipMemcpyDeviceToDevice, dj_rt_stream()));
      } else {
        const int esize = cudf::size_of(input_table.column(c).type());
        DJ_HIP_CALL(hipMemcpyAsync(
          (int8_t*)out->get_column(c).head() + recv_offsets[me] * esize,
          input_table.column(c).head<int8_t>() + (int64_t)send_offsets[me] * esize,
          (size_t)scount * esize, hipMemcpyDeviceToDevice, dj_rt_stream()));
      }
    }
    DJ_HIP_CALL(hipStreamSynchronize(dj_rt_stream()));
  }
  return out;
}

void AllToAllCommunicator::launch_communication(cudf::mutable_table_view communicated_table,
                                                bool report_timing,
                                                void* preallocated_pinned_buffer)
{
  const int G = comm_group.size();
  const int me = comm_group.get_local_idx();
  const bool include_self = !explicit_copy_to_current_rank;
  hipStream_t st = dj_rt_stream();
  std::vector<int64_t> soff(send_offsets.begin(), send_offsets.end());

  /* wire plan: per column one or two buffers, each either plain or
   * cascaded-compressed (the reference's compression branch,
   * all_to_all_comm.cpp:358-478: compress -> exchange compressed sizes ->
   * exchange compressed slices -> decompress receiver-side) */
  struct Plain {
    const int8_t* src;
    int8_t* dst;
    int esize;
    const std::vector<int64_t>* soff;
    const std::vector<int64_t>* roff;
  };
  struct Comp {
    const uint8_t* src;       // uncompressed source buffer
    uint8_t* dst;             // uncompressed destination
    int esize;
    int rles, delta, bp;
    const std::vector<int64_t>* soff;  // element offsets (source)
    const std::vector<int64_t>* roff;  // element offsets (destination)
    DBuf comp;                         // compressed send slices (bound-sized slots)
    std::vector<size_t> slot;          // slot byte offsets (G+1)
    std::vector<int64_t> csize;        // compressed bytes per peer
    std::vector<int64_t> csend_off;    // prefix of csize (G+1)
    std::vector<int64_t> crecv_off;    // recv byte offsets (G+1)
    DBuf comp_recv;
  };
  std::vector<Plain> plains;
  std::vector<Comp> comps;
  auto add_buffer = [&](const void* src, void* dst, int esize,
                        const std::vector<int64_t>* so, const std::vector<int64_t>* ro,
                        const ColumnCompressionOptions& opt) {
    if (opt.compression_method == CompressionMethod::cascaded) {
      Comp c;
      c.src = (const uint8_t*)src;
      c.dst = (uint8_t*)dst;
      c.esize = esize;
      c.rles = opt.cascaded_format.num_RLEs;
      c.delta = opt.cascaded_format.num_deltas;
      c.bp = opt.cascaded_format.use_bp;
      c.soff = so;
      c.roff = ro;
      comps.push_back(std::move(c));
    } else {
      plains.push_back(Plain{(const int8_t*)src, (int8_t*)dst, esize, so, ro});
    }
  };

  /* per-column element-offset vectors must outlive the exchange */
  std::vector<std::vector<int64_t>> offsets_storage;
  offsets_storage.reserve(input_table.num_columns() * 2 + 2);
  offsets_storage.push_back(soff);
  const std::vector<int64_t>* rows_soff = &offsets_storage.back();
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    auto in = input_table.column(c);
    auto out = communicated_table.column(c);
    if (in.type().id() == cudf::type_id::STRING) {
      /* sizes on the wire take the OFFSETS CHILD's options — the reference
       * applies children[0] to the offsets buffer (all_to_all_comm.cpp:
       * 269-279); generate_auto_select emits parent=none, child[0]=cascaded,
       * so using the parent here would silently send sizes uncompressed.
       * Chars (children[1]) are never compressed (compression.cpp:44-60). */
      const ColumnCompressionOptions& sizes_opt =
        compression_options[c].children_compression_options.empty()
          ? compression_options[c]
          : compression_options[c].children_compression_options[0];
      add_buffer(strings->sizes_to_send[c].p, strings->sizes_received[c].p, 4, rows_soff,
                 &recv_offsets, sizes_opt);
      plains.push_back(Plain{(const int8_t*)in.chars(), (int8_t*)out.chars(), 1,
                             &strings->send_char_offsets[c], &strings->recv_char_offsets[c]});
    } else {
      add_buffer(in.head<int8_t>(), out.head<int8_t>(), cudf::size_of(in.type()), rows_soff,
                 &recv_offsets, compression_options[c]);
    }
  }

  /* validity masks of the columns nullable anywhere in the group: each
   * peer's row slice is cut out of the column's mask into a word-aligned
   * packed slice of one staging buffer (dj::copy_bitmask_segments) and
   * travels raw, as uint32 words, behind the data buffers; the receiver
   * merges the G slices at recv_offsets below. Never compressed. The self
   * slice does not travel: the merge reads it from the input mask. */
  struct MaskWire {
    cudf::size_type col;
    DBuf send_stage, recv_stage;
    std::vector<int64_t> swo, rwo;  // word offsets per peer (G+1), self empty
  };
  std::vector<MaskWire> mwires;
  std::vector<DBuf> seg_tables;
  mwires.reserve((size_t)input_table.num_columns());
  for (cudf::size_type c = 0; c < input_table.num_columns() && nullable_cols; c++) {
    if (!((nullable_cols >> c) & 1u)) continue;
    DJ_CHECK_ERROR(communicated_table.column(c).null_mask() != nullptr,
                   "launch_communication: the communicated table lacks the mask of a nullable "
                   "column (allocate it with allocate_communicated_table)");
    mwires.emplace_back();
    MaskWire& w = mwires.back();
    w.col = c;
    w.swo.assign(G + 1, 0);
    w.rwo.assign(G + 1, 0);
    std::vector<BitSeg> segs;
    const uint32_t* mask = input_table.column(c).null_mask();
    for (int i = 0; i < G; i++) {
      const int64_t scount = i == me ? 0 : soff[i + 1] - soff[i];
      const int64_t rcount = i == me ? 0 : recv_offsets[i + 1] - recv_offsets[i];
      const int64_t swords = (scount + 31) / 32;
      w.swo[i + 1] = w.swo[i] + swords;
      w.rwo[i + 1] = w.rwo[i] + (rcount + 31) / 32;
      segs.push_back(BitSeg{mask, soff[i], scount});
      segs.push_back(BitSeg{nullptr, 0, swords * 32 - scount});  // pad to the word
    }
    w.send_stage = DBuf((size_t)std::max<int64_t>(w.swo[G], 1) * 4);
    w.recv_stage = DBuf((size_t)std::max<int64_t>(w.rwo[G], 1) * 4);
    seg_tables.push_back(copy_bit_segments(segs, (uint32_t*)w.send_stage.p, st));
    plains.push_back(Plain{(const int8_t*)w.send_stage.p, (int8_t*)w.recv_stage.p, 4, &w.swo,
                           &w.rwo});
  }
  if (!mwires.empty()) DJ_HIP_CALL(hipStreamSynchronize(st));

  /* compress send slices (compute stream), then read final sizes */
  int64_t max_recv_count = 0;
  if (!comps.empty()) {
    int64_t max_send_count = 1;
    for (auto& c : comps)
      for (int i = 0; i < G; i++)
        max_send_count = std::max(max_send_count, (*c.soff)[i + 1] - (*c.soff)[i]);
    DBuf cscratch(dj::compress_scratch_bytes(max_send_count));
    for (auto& c : comps) {
      c.slot.resize(G + 1);
      size_t acc = 0;
      for (int i = 0; i < G; i++) {
        c.slot[i] = acc;
        int64_t cnt = (*c.soff)[i + 1] - (*c.soff)[i];
        acc += (dj::compress_bound(cnt, c.esize) + 255) & ~(size_t)255;
      }
      c.slot[G] = acc;
      c.comp = DBuf(acc);
      for (int i = 0; i < G; i++) {
        if (i == me && !include_self) continue;
        int64_t cnt = (*c.soff)[i + 1] - (*c.soff)[i];
        dj::compress_slice_async(c.src + (*c.soff)[i] * c.esize, cnt, c.esize, c.rles,
                                 c.delta, c.bp, (uint8_t*)c.comp.p + c.slot[i], cscratch.p,
                                 st);
      }
    }
    DJ_HIP_CALL(hipStreamSynchronize(st));
    for (auto& c : comps) {
      c.csize.assign(G, 0);
      c.csend_off.assign(G + 1, 0);
      for (int i = 0; i < G; i++) {
        if (!(i == me && !include_self)) {
          dj::CompSliceHeader h;
          DJ_HIP_CALL(hipMemcpy(&h, (uint8_t*)c.comp.p + c.slot[i], sizeof(h),
                                hipMemcpyDeviceToHost));
          /* wire slices are padded to 4 bytes (inside the slot's bound) so
           * every received slice's packed words stay dword-aligned behind a
           * raw 1-/2-byte slice of odd length */
          c.csize[i] = ((int64_t)dj::compressed_size_from_header(h, c.esize) + 3) & ~(int64_t)3;
        }
        c.csend_off[i + 1] = c.csend_off[i] + c.csize[i];
      }
      /* exchange compressed byte counts (communicate_sizes over bytes) */
      communicate_sizes(c.csend_off, c.crecv_off, comm_group, communicator);
      c.comp_recv = DBuf((size_t)std::max<int64_t>(c.crecv_off.back(), 1));
      for (int i = 0; i < G; i++)
        max_recv_count = std::max(max_recv_count, (*c.roff)[i + 1] - (*c.roff)[i]);
    }
  }

  {
    dj_timing::Scope t(DJ_PHASE_COMM, dj_rt_comm_stream());
    communicator->start();
    for (auto& b : plains) {
      for (int i = 0; i < G; i++) {
        int64_t scount = (*b.soff)[i + 1] - (*b.soff)[i];
        int64_t rcount = (*b.roff)[i + 1] - (*b.roff)[i];
        const int8_t* src = b.src + (*b.soff)[i] * b.esize;
        int8_t* dst = b.dst + (*b.roff)[i] * b.esize;
        if (i == me) {
          if (include_self && scount > 0)
            DJ_HIP_CALL(hipMemcpyAsync(dst, src, (size_t)scount * b.esize,
                                       hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
          continue;
        }
        int peer = comm_group.get_global_rank(i);
        communicator->send(src, scount, b.esize, peer);
        communicator->recv(dst, rcount, b.esize, peer);
      }
    }
    for (auto& c : comps) {
      for (int i = 0; i < G; i++) {
        int64_t rbytes = c.crecv_off[i + 1] - c.crecv_off[i];
        if (i == me) {
          if (include_self && c.csize[i] > 0)
            DJ_HIP_CALL(hipMemcpyAsync((uint8_t*)c.comp_recv.p + c.crecv_off[i],
                                       (uint8_t*)c.comp.p + c.slot[i], (size_t)c.csize[i],
                                       hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
          continue;
        }
        int peer = comm_group.get_global_rank(i);
        communicator->send((uint8_t*)c.comp.p + c.slot[i], c.csize[i], 1, peer);
        communicator->recv((uint8_t*)c.comp_recv.p + c.crecv_off[i], rbytes, 1, peer);
      }
    }
    communicator->stop();  // blocks the host (all_to_all_comm.hpp:331 contract)
  }

  /* decompress received slices */
  if (!comps.empty()) {
    DBuf scratch(dj::compress_scratch_bytes(std::max<int64_t>(max_recv_count, 1)));
    for (auto& c : comps) {
      for (int i = 0; i < G; i++) {
        int64_t rbytes = c.crecv_off[i + 1] - c.crecv_off[i];
        int64_t rcount = (*c.roff)[i + 1] - (*c.roff)[i];
        if (rbytes == 0 || rcount == 0) continue;
        dj::CompSliceHeader h;
        DJ_HIP_CALL(hipMemcpy(&h, (uint8_t*)c.comp_recv.p + c.crecv_off[i], sizeof(h),
                              hipMemcpyDeviceToHost));
        DJ_CHECK_ERROR((int64_t)h.count == rcount,
                       "cascaded: received slice count mismatch");
        dj::decompress_slice_async((uint8_t*)c.comp_recv.p + c.crecv_off[i], h, c.esize,
                                   c.dst + (*c.roff)[i] * c.esize, scratch.p, st);
      }
    }
    DJ_HIP_CALL(hipStreamSynchronize(st));
    if (report_timing) {
      int64_t raw = 0, wire = 0;
      for (auto& c : comps) {
        for (int i = 0; i < G; i++) {
          if (i == me) continue;
          raw += ((*c.soff)[i + 1] - (*c.soff)[i]) * c.esize;
          wire += c.csize[i];
        }
      }
      if (raw > 0)
        std::cout << "Rank " << communicator->mpi_rank << ": cascaded wire "
                  << wire / 1.0e6 << "MB from " << raw / 1.0e6 << "MB ("
                  << (double)raw / (wire ? wire : 1) << "x)" << std::endl;
    }
  }
  (void)preallocated_pinned_buffer;

  /* receiver-side: merge the received mask slices, and this rank's own
   * slice, into the column's mask at recv_offsets; the column counts its
   * nulls when next asked (its mutable view forgot the count) */
  for (auto& w : mwires) {
    std::vector<BitSeg> segs;
    for (int i = 0; i < G; i++) {
      const int64_t rcount = recv_offsets[i + 1] - recv_offsets[i];
      if (i == me)
        segs.push_back(BitSeg{input_table.column(w.col).null_mask(), soff[me], rcount});
      else
        segs.push_back(BitSeg{(const uint32_t*)w.recv_stage.p + w.rwo[i], 0, rcount});
    }
    seg_tables.push_back(
      copy_bit_segments(segs, communicated_table.column(w.col).null_mask(), st));
  }
  if (!mwires.empty()) DJ_HIP_CALL(hipStreamSynchronize(st));

  /* receiver-side: rebuild string offsets from the received sizes by scan
   * with offset[0]=0 (strings_column.cu:111-131) */
  if (strings) {
    const int64_t n_recv = recv_offsets.back();
    for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
      if (input_table.column(c).type().id() != cudf::type_id::STRING) continue;
      DBuf scr(dj::offsets_from_sizes_scratch_bytes(n_recv));
      dj::offsets_from_sizes((const int32_t*)strings->sizes_received[c].p, n_recv,
                             communicated_table.column(c).head<int32_t>(), scr.p, st);
      DJ_HIP_CALL(hipStreamSynchronize(st));  // scr freed on return; scan must be done
    }
  }
}

/* ----------------------------------------------------- partition + join core */

namespace {

/* gather a STRING column by a row-index permutation: sizes gather -> scan ->
 * chars gather (the reference's thrust::gather + scan strings recipe,
 * strings_column.cu:39-131, as one reusable step). null_tail > 0 appends
 * that many empty rows behind the n gathered ones (the null right-hand cells
 * of a left join): their offsets all equal the chars total. */
std::unique_ptr<cudf::column> gather_string_column(cudf::column_view src, const int64_t* d_idx,
                                                   int64_t n, int64_t null_tail = 0)
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
  if (null_tail > 0)
    hipLaunchKernelGGL(fill_i32_kernel, dim3(grid_for_n(null_tail)), dim3(kBlock), 0, st,
                       (int32_t*)col->head() + n + 1, null_tail, total);
  dj::gather_chars_from_starts((const uint8_t*)src.chars(), (const int32_t*)starts.p, n,
                               (const int32_t*)col->head(), (uint8_t*)col->chars(), st);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return col;
}

/* output assembly: append to `cols` one n-row column per column of `src`,
 * row i = src row idx[i]. All fixed-width columns go through ONE
 * dj::gather_table call (the width-generic kernel, dj_kernels.hip "table
 * gather"); STRING columns keep gather_string_column. The key column
 * (key_col >= 0) is not gathered: its joined values already sit in key_vals
 * as int64 (each random-line gather of 240 M rows costs ~5 ms; adopting the
 * key buffer is free, narrowing to the key's own width is a streaming copy).
 *
 * null_tail >= 0 builds the right-hand side of a left join: every column has
 * n + null_tail rows, the tail rows are null cells (zero bytes, empty
 * strings), and EVERY column carries a mask, whether its source had one or
 * not and also when null_tail is 0. The default, -1, is the plain gather. */
void gather_table_columns(cudf::table_view src, DBuf& idx, int64_t n, cudf::size_type key_col,
                          DBuf* key_vals, std::vector<std::unique_ptr<cudf::column>>& cols,
                          hipStream_t st, int64_t null_tail = -1)
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
  if (key_dst != nullptr && n > 0)
    hipLaunchKernelGGL(narrow_key_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, st, key_src, n,
                       key_width, key_dst);
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

/* stable hash-partition of an arbitrary table into nparts contiguous ranges:
 * permutation computed on (key, iota) with the stable wave-ballot kernel,
 * then one gather per column. 2-column all-INT64 tables skip the gathers
 * (keys+payload move directly through the partition scatter). */
struct PartitionedTable {
  std::unique_ptr<cudf::table> tbl;
  std::vector<cudf::size_type> offsets;  // nparts+1
};

/* ext_keys: when non-null, placement uses this caller-provided key array
 * (fused multi-column keys) instead of column key_col */
PartitionedTable partition_table(cudf::table_view in, cudf::size_type key_col, int nparts,
                                 int hash_fn, uint32_t seed,
                                 const int64_t* ext_keys = nullptr)
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
    hipLaunchKernelGGL(iota_i64_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0, st, iota.i64(), n);
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

/* the placement step of shuffle_on: the rows of `input` grouped into nparts
 * contiguous ranges by the hash of their key. Multi-column keys, and any
 * STRING key, place on the fused key chain (our spec, dj_hash.h —
 * MurmurHash3 placement is parity-unpinned) */
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
      hipLaunchKernelGGL(nullable_key_hash_kernel, dim3(grid_for_n(n)), dim3(kBlock), 0,
                         dj_rt_stream(), col.head<void>(), key_kind(col.type()),
                         col.null_mask(), n, hash_fn, seed, fused.i64());
    return partition_table(input, on[0], nparts, DJ_HASH_IDENTITY, 0, fused.i64());
  }
  return partition_table(input, on[0], nparts, hash_fn, seed, fused.p ? fused.i64() : nullptr);
}

/* what one bucket join leaves on the device besides its rows: the match
 * counter and the engine's two flags, in one block so that a single 16-byte
 * copy reads them back */
struct JoinMeta {
  int64_t count;     // matches found (may exceed the capacity written)
  int error;         // sentinel (-1) keys seen and skipped
  int any_overflow;  // skewed buckets skipped
};
static_assert(sizeof(JoinMeta) == 16 && offsetof(JoinMeta, count) == 0 &&
                offsetof(JoinMeta, error) == 8 && offsetof(JoinMeta, any_overflow) == 12,
              "JoinMeta is read back from the device as one 16-byte block");

/* engine outputs of one join, `cap` rows each: o0/o2 the joined key values
 * (left/right), o1/o3 the payloads — source row indices unless the tables
 * are int64 pairs (joins_i64_pairs) */
struct JoinOut {
  DBuf o0, o1, o2, o3, meta;
  int64_t cap{0};
  JoinOut() = default;
  explicit JoinOut(int64_t cap_)
    : o0((size_t)cap_ * 8),
      o1((size_t)cap_ * 8),
      o2((size_t)cap_ * 8),
      o3((size_t)cap_ * 8),
      meta(sizeof(JoinMeta)),
      cap(cap_)
  {
  }
  /* first-try capacity for rn probe rows; the engine counts every match but
   * writes only the first cap, so a count above it means redo */
  static int64_t default_cap(int64_t rn) { return std::max<int64_t>(rn + (rn >> 3), 1024); }
  int64_t* counter() { return &((JoinMeta*)meta.p)->count; }
  int* error() { return &((JoinMeta*)meta.p)->error; }
  int* any_overflow() { return &((JoinMeta*)meta.p)->any_overflow; }
  void clear(hipStream_t st) { DJ_HIP_CALL(hipMemsetAsync(meta.p, 0, sizeof(JoinMeta), st)); }
};

/* the bucketed-LDS engine with its capacity retry: rerun at the exact size
 * when the matches outnumber the first-try capacity. Host-synchronous. */
std::pair<JoinOut, int64_t> run_bucket_join(const int64_t* lk, const int64_t* lp, int64_t ln,
                                            const int64_t* rk, const int64_t* rp, int64_t rn)
{
  hipStream_t st = dj_rt_stream();
  DBuf scratch((size_t)dj_bucket_join_scratch_bytes(ln, rn));
  int64_t cap = JoinOut::default_cap(rn);
  for (;;) {
    JoinOut out(cap);
    out.clear(st);
    dj_bucket_local_join(lk, lp, ln, rk, rp, rn, out.o0.i64(), out.o1.i64(), out.o2.i64(),
                         out.o3.i64(), cap, out.counter(), out.error(), scratch.p);
    JoinMeta m;
    DJ_HIP_CALL(hipMemcpyAsync(&m, out.meta.p, sizeof(m), hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
    DJ_CHECK_ERROR(m.error == 0, "join: sentinel flag not cleared by the bucket path");
    if (m.count <= cap) return {std::move(out), m.count};
    cap = m.count;
  }
}

/* appends one 0-row column per column of t; masked where the source is, or
 * everywhere (the right-hand side of a left join) */
void append_empty_columns(cudf::table_view t, bool all_masked,
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

/* the empty table with a join's output schema: left's columns, then right's */
std::unique_ptr<cudf::table> empty_join_result(cudf::table_view left, cudf::table_view right)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  append_empty_columns(left, false, cols);
  append_empty_columns(right, false, cols);
  return std::make_unique<cudf::table>(std::move(cols));
}

/* the first n rows of the engine's four outputs as four INT64 columns */
std::unique_ptr<cudf::table> adopt_i64x4(JoinOut& out, int64_t n)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (DBuf* d : {&out.o0, &out.o1, &out.o2, &out.o3}) {
    cols.push_back(std::make_unique<cudf::column>(cudf::data_type(cudf::type_id::INT64),
                                                  (cudf::size_type)n, d->p));
    d->p = nullptr;
  }
  return std::make_unique<cudf::table>(std::move(cols));
}

/* nout joined rows -> left-cols + right-cols. int64 pairs adopt the engine's
 * outputs as they are. Otherwise o1/o3 hold source row indices and every
 * column is gathered — EXCEPT a single integer key column (left_key /
 * right_key >= 0), whose joined values already sit in o0/o2 and are adopted
 * or narrowed instead (see gather_table_columns) */
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
std::unique_ptr<cudf::table> assemble_left_kind(join_kind kind, cudf::table_view left,
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
  int64_t nsel = 0;

  if (kind != join_kind::LEFT) {
    DBuf sel((size_t)ln * 8);
    dj::select_rows((const uint32_t*)bits.p, ln, kind == join_kind::LEFT_SEMI, sel.i64(),
                    count.i64(), st, scratch.p);
    DJ_HIP_CALL(hipMemcpyAsync(&nsel, count.p, 8, hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
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
  DJ_HIP_CALL(hipMemcpyAsync(&nsel, count.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  DJ_CHECK_ERROR(nout + nsel <= INT32_MAX, "left join: output exceeds 2^31 rows");
  gather_table_columns(left, out.o1, nout + nsel, -1, nullptr, cols, st);
  gather_table_columns(right, out.o3, nout, -1, nullptr, cols, st, nsel);
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return std::make_unique<cudf::table>(std::move(cols));
}

dj::TupleKeyCol tuple_key_col(cudf::column_view col)
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
KeyRowValidity key_row_validity(cudf::table_view t, std::vector<cudf::size_type> const& on,
                                hipStream_t st)
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
  unsigned long long h = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&h, cnt.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  v.nnull = (int64_t)h;
  if (v.nnull > 0) v.bits = nm == 1 ? masks[0] : (const uint32_t*)v.own.p;
  return v;
}

/* the engine's view of one side under UNEQUAL: the keys of the valid-key
 * rows and, as the payload, their row numbers in the table */
struct CompactedKeys {
  DBuf keys, rows;
  int64_t n{0};
};

CompactedKeys compact_valid_keys(KeyRowValidity const& v, const int64_t* keys, int64_t nrows,
                                 hipStream_t st)
{
  CompactedKeys c;
  c.n = nrows - v.nnull;
  if (c.n <= 0) return c;
  c.keys = DBuf((size_t)c.n * 8);
  c.rows = DBuf((size_t)c.n * 8);
  DBuf scratch(dj::select_rows_scratch_bytes(nrows)), count(8);
  dj::compact_keyed_rows(v.bits, nrows, keys, c.rows.i64(), c.keys.i64(), count.i64(), st,
                         scratch.p);
  int64_t got = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&got, count.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  DJ_CHECK_ERROR(got == c.n, "join: a key column's null_count disagrees with its mask");
  return c;
}

/* local join of two tables via the bucketed-LDS engine. INNER returns
 * left-cols + right-cols with keys duplicated, row order unspecified; the
 * other kinds build the same pair list and hand it to assemble_left_kind.
 * A single integer key column is the engine's key as it is (widened when
 * narrow). Composite keys, and STRING keys even alone, bucket-join on the
 * fused key chain (fuse_keys: the row hash stands in for a string) with
 * row-index payloads, then drop fused-hash collisions against the real
 * columns — the single-key engine does the heavy lifting; only
 * placement/equality semantics widen. (Reference: cudf::inner_join on
 * arbitrary left_on/right_on, distributed_join.cpp:71-132.) */
std::unique_ptr<cudf::table> local_join(
  join_kind kind, cudf::table_view left, cudf::table_view right,
  std::vector<cudf::size_type> const& lon, std::vector<cudf::size_type> const& ron,
  cudf::null_equality compare_nulls = cudf::null_equality::EQUAL)
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
    DJ_HIP_CALL(hipMemcpyAsync(&nout, out.counter(), 8, hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
    if (nout == 0 && inner) return empty_join_result(left, right);
    out.o1 = std::move(li2);
    out.o3 = std::move(ri2);
  }
  if (!inner) return assemble_left_kind(kind, left, right, out, nout, li_cap);
  return assemble_join_output(left, right, out, nout, left_key, right_key);
}

std::unique_ptr<cudf::table> local_inner_join(cudf::table_view left, cudf::table_view right,
                                              std::vector<cudf::size_type> const& lon,
                                              std::vector<cudf::size_type> const& ron)
{
  return local_join(join_kind::INNER, left, right, lon, ron);
}

/* null_equality::UNEQUAL over several ranks: a table cut, before anything is
 * communicated, into `valid`, its rows without a null in their key tuple
 * (same schema, mask presence included), and, when asked for, `null_rows`,
 * the others in the form the rank appends to its result: the table's columns
 * and, with pad_with, behind them that table's columns as all-null cells, as
 * a LEFT join pads an unmatched row. Both are null when no key column holds
 * a null: the caller goes on with the table it has. One full gather of the
 * table through the ascending row list of select_rows. */
struct StrippedTable {
  std::unique_ptr<cudf::table> valid, null_rows;
};

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

/* rebase a part's offsets by a constant and append (STRING concat) */
__global__ void rebase_offsets_kernel(const int32_t* __restrict__ src, int64_t n, int32_t base,
                                      int32_t* __restrict__ dst)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i] + base;
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
          hipLaunchKernelGGL(rebase_offsets_kernel, dim3(grid_for_n(nrows + 1)), dim3(kBlock),
                             0, st, (const int32_t*)p->get_column(c).head(), nrows + 1,
                             (int32_t)char_off, (int32_t*)col->head() + row_off);
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

/* what batch finalisation needs of a pipeline batch; both pipelines' Batch
 * structs extend it with their own staging */
struct BatchJoin {
  std::unique_ptr<AllToAllCommunicator> latoa, ratoa;
  std::unique_ptr<cudf::table> lrecv, rrecv;  // this rank's share of the batch
  JoinOut out;                                // its join, enqueued by the pipeline
};

/* the end of both batched pipelines, once the compute stream has drained:
 * per batch read the counts, redo the rare failures, assemble the columns;
 * then concatenate. A batch with an empty side had nothing enqueued and its
 * meta block is all zero. The redo goes synchronously through
 * local_inner_join, whose bucket path joins sentinel (-1) keys out-of-band
 * (neg1_cross_join), re-joins skewed buckets via the global-table fallback
 * and sizes the output exactly. The flags are looked at BEFORE the count:
 * the enqueued join skips -1 keys and oversized buckets, so its count can be
 * 0 while the redo still finds rows. */
template <class Batch>
std::unique_ptr<cudf::table> finalize_batches(std::vector<Batch>& batches,
                                              cudf::size_type left_key,
                                              cudf::size_type right_key, bool report_timing,
                                              int rank)
{
  std::vector<std::unique_ptr<cudf::table>> results;
  for (BatchJoin& bt : batches) {
    const cudf::table_view l = bt.lrecv->view(), r = bt.rrecv->view();
    JoinMeta meta;
    DJ_HIP_CALL(hipMemcpy(&meta, bt.out.meta.p, sizeof(meta), hipMemcpyDeviceToHost));
    if (l.num_rows() == 0 || r.num_rows() == 0)
      results.push_back(empty_join_result(l, r));
    else if (meta.error || meta.any_overflow || meta.count > bt.out.cap)
      results.push_back(local_inner_join(l, r, {left_key}, {right_key}));
    else if (meta.count == 0)
      results.push_back(empty_join_result(l, r));
    else
      results.push_back(assemble_join_output(l, r, bt.out, meta.count, left_key, right_key));
  }
  const auto t_cat0 = std::chrono::steady_clock::now();
  auto result = concat_tables(results);
  if (report_timing && batches.size() > 1)
    std::cout << "Rank " << rank << ": concatenation takes "
              << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                           t_cat0)
                   .count()
              << "ms" << std::endl;
  return result;
}

}  // namespace

/* access hook for the fused path (friend declared in all_to_all_comm.hpp) */
struct AllToAllCommunicatorAccess {
  static const std::vector<int64_t>& recv_offsets(const AllToAllCommunicator& a)
  {
    return a.recv_offsets;
  }
  /* an AllToAllCommunicator whose row-count exchange carries the join's
   * route tag (join_route_tag below) */
  static std::unique_ptr<AllToAllCommunicator> make(
    cudf::table_view t, std::vector<cudf::size_type> offsets, CommunicationGroup group,
    Communicator* communicator, std::vector<ColumnCompressionOptions> const& opts,
    bool explicit_copy, uint32_t route_tag)
  {
    return std::unique_ptr<AllToAllCommunicator>(new AllToAllCommunicator(
      t, std::move(offsets), group, communicator, opts, explicit_copy, route_tag));
  }
};

/* The route distributed_inner_join takes depends on nullability, which each
 * rank sees only of its own tables: bit 0 = a key column is nullable (shuffle
 * + local join on the fused key chain), bit 1 = two-column tables carrying a
 * mask (which keeps 2 x INT64 tables off the fused wire path). Every route
 * starts with the row-count exchange of an AllToAllCommunicator over the
 * left table, one count per peer whatever the route, so the tag rides it and
 * ranks that disagree stop loudly there instead of pairing mismatched
 * messages. */
static uint32_t join_route_tag(cudf::table_view left, cudf::table_view right,
                               std::vector<cudf::size_type> const& lon,
                               std::vector<cudf::size_type> const& ron)
{
  uint32_t tag = 0;
  if (any_nullable_key(left, lon) || any_nullable_key(right, ron)) tag |= 1u;
  if (left.num_columns() == 2 && right.num_columns() == 2 &&
      (any_nullable(left) || any_nullable(right)))
    tag |= 2u;
  return tag;
}

static std::unique_ptr<cudf::table> shuffle_on_tagged(
  cudf::table_view const& input, std::vector<cudf::size_type> const& on_columns,
  CommunicationGroup comm_group, Communicator* communicator,
  std::vector<ColumnCompressionOptions> compression_options, cudf::hash_id hash_function,
  uint32_t hash_seed, bool report_timing, void* preallocated_pinned_buffer, uint32_t route_tag);

namespace {

/* exchange per-peer int64 vectors (host) through the communicator */
void exchange_vecs(CommunicationGroup group, Communicator* communicator,
                   const std::vector<std::vector<int64_t>>& send,
                   std::vector<std::vector<int64_t>>& recv)
{
  const int G = group.size();
  const int me = group.get_local_idx();
  const int V = (int)send[0].size();
  recv.assign(G, std::vector<int64_t>(V, 0));
  recv[me] = send[me];
  if (G == 1) return;
  DBuf ds((size_t)G * V * 8), dr((size_t)G * V * 8);
  std::vector<int64_t> flat((size_t)G * V);
  for (int i = 0; i < G; i++)
    std::copy(send[i].begin(), send[i].end(), flat.begin() + (size_t)i * V);
  DJ_HIP_CALL(hipMemcpyAsync(ds.p, flat.data(), flat.size() * 8, hipMemcpyHostToDevice,
                             dj_rt_comm_stream()));
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
  communicator->start();
  for (int i = 0; i < G; i++) {
    if (i == me) continue;
    int peer = group.get_global_rank(i);
    communicator->send(ds.i64() + (size_t)i * V, V, 8, peer);
    communicator->recv(dr.i64() + (size_t)i * V, V, 8, peer);
  }
  communicator->stop();
  DJ_HIP_CALL(hipMemcpyAsync(flat.data(), dr.p, flat.size() * 8, hipMemcpyDeviceToHost,
                             dj_rt_comm_stream()));
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
  for (int i = 0; i < G; i++)
    if (i != me) recv[i].assign(flat.begin() + (size_t)i * V, flat.begin() + (size_t)(i + 1) * V);
}

/* the fused wire path (2 x INT64 columns, keys at column 0): ONE staged
 * scatter produces the rank/batch slices pre-grouped by PA groups; the
 * receiver runs pass B over per-peer segment lists straight into the LDS
 * join — the separate stable rank partition and bucket pass A disappear
 * (DESIGN.md §3 ablation: the partition passes dominated the step). */
std::unique_ptr<cudf::table> distributed_inner_join_fused(
  cudf::table_view left, cudf::table_view right, Communicator* communicator,
  CommunicationGroup group, std::vector<ColumnCompressionOptions> const& lopts,
  std::vector<ColumnCompressionOptions> const& ropts, int od, int PA, bool report_timing,
  void* pinned)
{
  hipStream_t st = dj_rt_stream();
  const int G = group.size();
  const int P = G * od * PA;
  const int64_t ln = left.num_rows(), rn = right.num_rows();

  /* fused partition of both tables (columnar outputs for the wire) */
  DBuf counts((size_t)dj::kBucketBlocks * P * 4), totals((size_t)P * 4);
  DBuf d_poff((size_t)(P + 1) * 8);
  DBuf lkp((size_t)std::max<int64_t>(ln, 1) * 8), lpp((size_t)std::max<int64_t>(ln, 1) * 8);
  DBuf rkp((size_t)std::max<int64_t>(rn, 1) * 8), rpp((size_t)std::max<int64_t>(rn, 1) * 8);
  std::vector<int64_t> lposf(P + 1, 0), rposf(P + 1, 0);
  {
    dj_timing::Scope t(DJ_PHASE_PART_SCATTER, st);
    dj::fused_partition(left.column(0).head<int64_t>(), left.column(1).head<int64_t>(), ln,
                        G * od, DJ_SEED_INTRA, PA, (uint32_t*)counts.p, (uint32_t*)totals.p,
                        d_poff.i64(), lkp.i64(), lpp.i64(), st);
    DJ_HIP_CALL(hipMemcpyAsync(lposf.data(), d_poff.p, (size_t)(P + 1) * 8,
                               hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
    dj::fused_partition(right.column(0).head<int64_t>(), right.column(1).head<int64_t>(), rn,
                        G * od, DJ_SEED_INTRA, PA, (uint32_t*)counts.p, (uint32_t*)totals.p,
                        d_poff.i64(), rkp.i64(), rpp.i64(), st);
    DJ_HIP_CALL(hipMemcpyAsync(rposf.data(), d_poff.p, (size_t)(P + 1) * 8,
                               hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
  }

  cudf::table_view lpart_view = view_i64_pair(lkp.p, lpp.p, ln);
  cudf::table_view rpart_view = view_i64_pair(rkp.p, rpp.p, rn);

  struct Batch : BatchJoin {
    std::vector<std::vector<int64_t>> lsub_recv, rsub_recv;  // [G][PA]
    DBuf lseg, rseg;       // device [G][PA+1]
    DBuf lgb, rgb;         // device [PA+1] group bases
    DBuf lpairs, rpairs;   // bucketed pairs
    DBuf loff, roff;       // int64[B+1]
    DBuf flags;            // u32[B]
    int F{0};
    int join_slots{2048};
    int64_t lrows{0}, rrows{0};
  };
  std::vector<Batch> batches(od);

  auto slice_of = [&](const std::vector<int64_t>& pofs, int b) {
    std::vector<cudf::size_type> sl(G + 1);
    for (int r = 0; r <= G; r++) sl[r] = (cudf::size_type)pofs[(size_t)(b * G + r) * PA];
    return sl;
  };
  auto subcounts_of = [&](const std::vector<int64_t>& pofs, int b) {
    std::vector<std::vector<int64_t>> sc(G, std::vector<int64_t>(PA));
    for (int r = 0; r < G; r++)
      for (int g = 0; g < PA; g++) {
        size_t base = (size_t)(b * G + r) * PA + g;
        sc[r][g] = pofs[base + 1] - pofs[base];
      }
    return sc;
  };

  /* pre-phase: exchanges + allocations */
  for (int b = 0; b < od; b++) {
    Batch& bt = batches[b];
    /* route tag 0: this path runs only on mask-free tables */
    bt.latoa = AllToAllCommunicatorAccess::make(lpart_view, slice_of(lposf, b), group,
                                                communicator, lopts, true, 0u);
    bt.ratoa = AllToAllCommunicatorAccess::make(rpart_view, slice_of(rposf, b), group,
                                                communicator, ropts, true, 0u);
    exchange_vecs(group, communicator, subcounts_of(lposf, b), bt.lsub_recv);
    exchange_vecs(group, communicator, subcounts_of(rposf, b), bt.rsub_recv);
    bt.lrecv = bt.latoa->allocate_communicated_table();
    bt.rrecv = bt.ratoa->allocate_communicated_table();
    bt.lrows = bt.lrecv->num_rows();
    bt.rrows = bt.rrecv->num_rows();
    /* seg bounds + group bases (host -> device) */
    auto build_segs = [&](const std::vector<std::vector<int64_t>>& sub,
                          const AllToAllCommunicator& atoa, DBuf& dseg, DBuf& dgb) {
      const auto& roff = AllToAllCommunicatorAccess::recv_offsets(atoa);
      std::vector<int64_t> seg((size_t)G * (PA + 1));
      std::vector<int64_t> gtot(PA + 1, 0);
      for (int r2 = 0; r2 < G; r2++) {
        int64_t acc = roff[r2];
        for (int g = 0; g <= PA; g++) {
          seg[(size_t)r2 * (PA + 1) + g] = acc;
          if (g < PA) acc += sub[r2][g];
        }
        for (int g = 0; g < PA; g++) gtot[g + 1] += sub[r2][g];
      }
      for (int g = 0; g < PA; g++) gtot[g + 1] += gtot[g];
      dseg = DBuf(seg.size() * 8);
      dgb = DBuf((size_t)(PA + 1) * 8);
      DJ_HIP_CALL(hipMemcpyAsync(dseg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice,
                                 st));
      DJ_HIP_CALL(hipMemcpyAsync(dgb.p, gtot.data(), (size_t)(PA + 1) * 8,
                                 hipMemcpyHostToDevice, st));
    };
    build_segs(bt.lsub_recv, *bt.latoa, bt.lseg, bt.lgb);
    build_segs(bt.rsub_recv, *bt.ratoa, bt.rseg, bt.rgb);
    DJ_HIP_CALL(hipStreamSynchronize(st));
    /* sub-bucket fanout: target ~760 rows per final bucket. F caps at 1024
     * (the staged span's one-group-per-thread scan); when buckets then run
     * big (e.g. G=8 od=1: 100M over PA*F=65536 => ~1526 rows) the join
     * switches to its 4096-slot table instead of overflowing every bucket. */
    int64_t maxn = std::max(bt.lrows, bt.rrows);
    int F = 64;
    while (F < 1024 && (int64_t)PA * F * 760 < maxn) F <<= 1;
    bt.F = F;
    if (const char* ff = getenv("DJ_FORCE_FUSED_F")) {
      /* TEST HOOK (tests/test_gpu_cpp_api.py::test_fused_big_buckets): force
       * a small fan-out so the 4096-slot join path is exercisable on one
       * GPU without an 8-rank 100M-row workload */
      int v = atoi(ff);
      if (v >= 64 && v <= 1024 && (v & (v - 1)) == 0) F = bt.F = v;
    }
    bt.join_slots = (maxn / ((int64_t)PA * F) > 1300) ? 4096 : 2048;
    int64_t B = (int64_t)PA * F;
    bt.lpairs = DBuf((size_t)std::max<int64_t>(bt.lrows, 1) * 16);
    bt.rpairs = DBuf((size_t)std::max<int64_t>(bt.rrows, 1) * 16);
    bt.loff = DBuf((size_t)(B + 1) * 8);
    bt.roff = DBuf((size_t)(B + 1) * 8);
    bt.flags = DBuf((size_t)B * 4);
    bt.out = JoinOut(JoinOut::default_cap(bt.rrows));
  }

  /* pipeline: comm(b) then enqueue passB+join(b); comm(b+1) overlaps */
  for (int b = 0; b < od; b++) {
    Batch& bt = batches[b];
    bt.latoa->launch_communication(bt.lrecv->mutable_view(), report_timing, pinned);
    bt.ratoa->launch_communication(bt.rrecv->mutable_view(), report_timing, pinned);
    bt.out.clear(st);
    if (bt.lrows == 0 || bt.rrows == 0) continue;
    int64_t B = (int64_t)PA * bt.F;
    DJ_HIP_CALL(hipMemsetAsync(bt.flags.p, 0, (size_t)B * 4, st));
    {
      dj_timing::Scope t(DJ_PHASE_BUCKET_SCATTER, st);
      dj::subpart_lists((const int64_t*)bt.lrecv->get_column(0).head(),
                        (const int64_t*)bt.lrecv->get_column(1).head(), bt.lseg.i64(), G, PA,
                        bt.F, bt.lgb.i64(), (longlong2*)bt.lpairs.p, bt.loff.i64(), st);
      dj::subpart_lists((const int64_t*)bt.rrecv->get_column(0).head(),
                        (const int64_t*)bt.rrecv->get_column(1).head(), bt.rseg.i64(), G, PA,
                        bt.F, bt.rgb.i64(), (longlong2*)bt.rpairs.p, bt.roff.i64(), st);
    }
    {
      dj_timing::Scope t(DJ_PHASE_JOIN_FUSED, st);
      dj::lds_join((const longlong2*)bt.lpairs.p, bt.loff.i64(),
                   (const longlong2*)bt.rpairs.p, bt.roff.i64(), (int)B, bt.join_slots,
                   bt.out.o0.i64(), bt.out.o1.i64(), bt.out.o2.i64(), bt.out.o3.i64(),
                   bt.out.cap, bt.out.counter(), (uint32_t*)bt.flags.p, bt.out.any_overflow(),
                   bt.out.error(), st);
    }
  }
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return finalize_batches(batches, 0, 0, false, communicator->mpi_rank);
}

}  // namespace

/* --------------------------------------------------- distributed_inner_join */


/* replicates the reference's divisor search exactly
 * (distributed_join.cpp:55-69, including its sqrt starting point) */
static int get_nvl_partition_size(int mpi_size, int nvlink_domain_size)
{
  if (nvlink_domain_size >= mpi_size) return mpi_size;
  for (int size = (int)ceil(sqrt((double)mpi_size)); size > 0; size--)
    if (mpi_size % size == 0 && size <= nvlink_domain_size) return size;
  return 1;
}

std::unique_ptr<cudf::table> distributed_inner_join(
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor,
  bool report_timing,
  void* preallocated_pinned_buffer,
  int nvlink_domain_size)
{
  DJ_CHECK_ERROR(left_on.size() == right_on.size() && !left_on.empty(),
                 "left_on/right_on must name the same number of key columns");
  DJ_CHECK_ERROR(left_on.size() <= 4, "up to 4 join key columns supported");
  validate_compression(left, left_compression_options);
  validate_compression(right, right_compression_options);
  check_key_pairs(left, right, left_on, right_on);
  const int world = communicator->mpi_size;
  const int nvl = get_nvl_partition_size(world, nvlink_domain_size < 1 ? 1 : nvlink_domain_size);

  /* 2-level hierarchy (distributed_join.cpp:152-199): when the join group is
   * smaller than the world, first shuffle both tables across domains (the
   * reference's InfiniBand stage, seed 87654321), then run the flat batched
   * pipeline within each domain (seed 12345678). On one xGMI node
   * nvlink_domain_size >= world collapses this to the flat path. */
  std::unique_ptr<cudf::table> l_ib, r_ib;
  if (nvl != world) {
    CommunicationGroup inter(world, nvl, communicator->mpi_rank);
    l_ib = shuffle_on(left, left_on, inter, communicator, left_compression_options,
                      cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTER, report_timing,
                      preallocated_pinned_buffer);
    r_ib = shuffle_on(right, right_on, inter, communicator, right_compression_options,
                      cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTER, report_timing,
                      preallocated_pinned_buffer);
    left = l_ib->view();
    right = r_ib->view();
  }
  if (nvl == 1) return local_inner_join(left, right, left_on, right_on);

  /* composite keys, any STRING key and any nullable key join on the fused
   * key chain; nullability is read after the inter-domain shuffle, which
   * gives a column a mask when it had one on any rank of that group */
  const uint32_t route_tag = join_route_tag(left, right, left_on, right_on);
  const bool fused_keys = left_on.size() > 1 || any_string_key(left, left_on) ||
                          any_string_key(right, right_on) || (route_tag & 1u);

  if (fused_keys) {
    /* multi-column keys, and STRING keys even alone, take the shuffle +
     * local-join route (placement on the fused key chain both sides,
     * collisions filtered in the local join); the batched od pipeline stays
     * single-integer-key — the hot shape the reference benchmarks */
    CommunicationGroup g2(nvl, 1, communicator->mpi_rank);
    auto ls = shuffle_on_tagged(left, left_on, g2, communicator, left_compression_options,
                                cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTRA, report_timing,
                                preallocated_pinned_buffer, route_tag);
    auto rs = shuffle_on_tagged(right, right_on, g2, communicator, right_compression_options,
                                cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTRA, report_timing,
                                preallocated_pinned_buffer, route_tag);
    return local_inner_join(ls->view(), rs->view(), left_on, right_on);
  }

  const int G = nvl;
  CommunicationGroup group(nvl, 1, communicator->mpi_rank);
  const int nparts = G * over_decom_factor;
  DJ_CHECK_ERROR(nparts <= dj::kMaxPartitions,
                 "join-group size x over_decom_factor must be <= 1024");

  /* fused wire path for the hot shape (2 x INT64 columns, key at 0):
   * partitions carry the bucket grouping on the wire, removing the separate
   * stable rank partition and bucket pass A */
  const cudf::size_type left_key = left_on[0], right_key = right_on[0];
  const bool fast2 = joins_i64_pairs(left, right, left_key, right_key);
  if (fast2) {
    int pa = 1;
    while (pa * 2 * nparts <= 1024) pa *= 2;
    if (pa >= 4)
      return distributed_inner_join_fused(left, right, communicator, group,
                                          left_compression_options, right_compression_options,
                                          over_decom_factor, pa, report_timing,
                                          preallocated_pinned_buffer);
  }

  /* report_timing mirrors the reference's per-phase prints
   * (distributed_join.cpp:120-130, 235-240) */
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  auto t_part0 = now();

  /* rank-level stable partition, seed 12345678 (distributed_join.cpp:211-226) */
  PartitionedTable lpart =
    partition_table(left, left_key, nparts, DJ_HASH_MURMUR3, DJ_SEED_INTRA);
  PartitionedTable rpart =
    partition_table(right, right_key, nparts, DJ_HASH_MURMUR3, DJ_SEED_INTRA);
  if (report_timing)
    std::cout << "Rank " << communicator->mpi_rank << ": hash partition takes "
              << ms(t_part0, now()) << "ms" << std::endl;

  /* --- pre-phase: size exchanges + every allocation (pool allocs sync the
   * compute stream, so none happen inside the pipeline) --- */
  struct Batch : BatchJoin {
    DBuf lkw, rkw;  // widened keys, where the key column is narrower than 64 bits
    int64_t ln{0}, rn{0};
  };
  std::vector<Batch> batches(over_decom_factor);
  int64_t max_ln = 1, max_rn = 1;
  for (int b = 0; b < over_decom_factor; b++) {
    Batch& bt = batches[b];
    std::vector<cudf::size_type> lslice(lpart.offsets.begin() + b * G,
                                        lpart.offsets.begin() + b * G + G + 1);
    std::vector<cudf::size_type> rslice(rpart.offsets.begin() + b * G,
                                        rpart.offsets.begin() + b * G + G + 1);
    bt.latoa = AllToAllCommunicatorAccess::make(lpart.tbl->view(), lslice, group, communicator,
                                                left_compression_options, true, route_tag);
    bt.ratoa = AllToAllCommunicatorAccess::make(rpart.tbl->view(), rslice, group, communicator,
                                                right_compression_options, true, route_tag);
    bt.lrecv = bt.latoa->allocate_communicated_table();
    bt.rrecv = bt.ratoa->allocate_communicated_table();
    bt.ln = bt.lrecv->num_rows();
    bt.rn = bt.rrecv->num_rows();
    max_ln = std::max(max_ln, bt.ln);
    max_rn = std::max(max_rn, bt.rn);
    bt.out = JoinOut(JoinOut::default_cap(bt.rn));
    if (bt.ln && cudf::size_of(left.column(left_key).type()) < 8)
      bt.lkw = DBuf((size_t)bt.ln * 8);
    if (bt.rn && cudf::size_of(right.column(right_key).type()) < 8)
      bt.rkw = DBuf((size_t)bt.rn * 8);
  }
  DBuf scratch((size_t)dj_bucket_join_scratch_bytes(max_ln, max_rn));
  hipStream_t st = dj_rt_stream();

  /* --- pipeline: comm of batch b on the comm stream overlaps the join of
   * batch b-1 on the compute stream (the host blocks only in
   * launch_communication's stop; join kernels are enqueued without syncs) —
   * replaces the reference's join thread + atomic-flag busy wait
   * (distributed_join.cpp:283-329) with stream ordering --- */
  auto t_pipe0 = now();
  for (int b = 0; b < over_decom_factor; b++) {
    Batch& bt = batches[b];
    auto t_comm0 = now();
    bt.latoa->launch_communication(bt.lrecv->mutable_view(), report_timing,
                                   preallocated_pinned_buffer);
    bt.ratoa->launch_communication(bt.rrecv->mutable_view(), report_timing,
                                   preallocated_pinned_buffer);
    if (report_timing)
      std::cout << "Rank " << communicator->mpi_rank << ": all-to-all communication (batch "
                << b << ") takes " << ms(t_comm0, now()) << "ms" << std::endl;
    bt.out.clear(st);
    if (bt.ln == 0 || bt.rn == 0) continue;
    const cudf::table_view l = bt.lrecv->view(), r = bt.rrecv->view();
    /* narrow keys widen into the buffers of the pre-phase; int64 pairs carry
     * their payloads through the join, every other shape the row index,
     * which the partition kernels synthesize (pay == nullptr) */
    const int64_t* lk = key_as_i64(l.column(left_key), bt.lkw.i64(), st);
    const int64_t* rk = key_as_i64(r.column(right_key), bt.rkw.i64(), st);
    const int64_t* lp = fast2 ? l.column(1).head<int64_t>() : nullptr;
    const int64_t* rp = fast2 ? r.column(1).head<int64_t>() : nullptr;
    dj_bucket_local_join_enqueue(lk, lp, bt.ln, rk, rp, bt.rn, bt.out.o0.i64(),
                                 bt.out.o1.i64(), bt.out.o2.i64(), bt.out.o3.i64(), bt.out.cap,
                                 bt.out.counter(), bt.out.error(), bt.out.any_overflow(),
                                 scratch.p);
  }
  DJ_HIP_CALL(hipStreamSynchronize(st));
  if (report_timing)
    std::cout << "Rank " << communicator->mpi_rank
              << ": communication + local join pipeline takes " << ms(t_pipe0, now()) << "ms"
              << std::endl;

  return finalize_batches(batches, left_key, right_key, report_timing, communicator->mpi_rank);
}

/* ------------------------------------------- left / left semi / left anti */

std::unique_ptr<cudf::table> distributed_join(
  join_kind kind,
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor,
  bool report_timing,
  void* preallocated_pinned_buffer,
  int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  const bool sql = compare_nulls == cudf::null_equality::UNEQUAL;
  if (kind == join_kind::INNER && !sql)
    return distributed_inner_join(left, right, left_on, right_on, communicator,
                                  std::move(left_compression_options),
                                  std::move(right_compression_options), over_decom_factor,
                                  report_timing, preallocated_pinned_buffer, nvlink_domain_size);
  DJ_CHECK_ERROR(kind == join_kind::INNER || kind == join_kind::LEFT ||
                   kind == join_kind::LEFT_SEMI || kind == join_kind::LEFT_ANTI,
                 "distributed_join: unknown join kind");
  DJ_CHECK_ERROR(left_on.size() == right_on.size() && !left_on.empty(),
                 "left_on/right_on must name the same number of key columns");
  DJ_CHECK_ERROR(left_on.size() <= 4, "up to 4 join key columns supported");
  validate_compression(left, left_compression_options);
  validate_compression(right, right_compression_options);
  check_key_pairs(left, right, left_on, right_on);

  /* a semi / anti join asks of the right table only whether a key exists:
   * its other columns stay home, before any stage that communicates */
  std::vector<cudf::size_type> ron = right_on;
  if (kind == join_kind::LEFT_SEMI || kind == join_kind::LEFT_ANTI) {
    std::vector<cudf::column_view> key_cols;
    std::vector<ColumnCompressionOptions> key_opts;
    for (size_t k = 0; k < right_on.size(); k++) {
      key_cols.push_back(right.column(right_on[k]));
      if ((size_t)right_on[k] < right_compression_options.size())
        key_opts.push_back(right_compression_options[(size_t)right_on[k]]);
      ron[k] = (cudf::size_type)k;
    }
    if (key_opts.size() != key_cols.size()) key_opts.clear();
    right = cudf::table_view(std::move(key_cols));
    right_compression_options = std::move(key_opts);
  }

  const int world = communicator->mpi_size;
  /* one rank: the local join keeps the null-key rows out of the engine
   * itself, without compacting a column */
  if (world == 1) return local_join(kind, left, right, left_on, ron, compare_nulls);

  /* null_equality::UNEQUAL over several ranks: null-key rows never reach the
   * communicator. Each rank strips its tables to their valid-key rows before
   * the first stage that communicates (a local step that leaves the schema,
   * mask presence included, as it is, so the route and its tag are those of
   * the EQUAL join of the stripped tables) and, for LEFT and LEFT_ANTI,
   * appends its own null-key left rows to its result. */
  if (sql) {
    const bool keep = kind == join_kind::LEFT || kind == join_kind::LEFT_ANTI;
    StrippedTable l =
      strip_null_keys(left, left_on, keep, kind == join_kind::LEFT ? &right : nullptr);
    StrippedTable r = strip_null_keys(right, ron, false, nullptr);
    if (l.valid) left = l.valid->view();
    if (r.valid) right = r.valid->view();
    auto joined =
      distributed_join(kind, left, right, left_on, ron, communicator, left_compression_options,
                       right_compression_options, over_decom_factor, report_timing,
                       preallocated_pinned_buffer, nvlink_domain_size);
    if (!l.null_rows) return joined;
    std::vector<std::unique_ptr<cudf::table>> parts;
    parts.push_back(std::move(joined));
    parts.push_back(std::move(l.null_rows));
    return concat_tables(parts);
  }

  const int nvl = get_nvl_partition_size(world, nvlink_domain_size < 1 ? 1 : nvlink_domain_size);
  /* the same inter-domain stage as the inner join's (seed 87654321) */
  std::unique_ptr<cudf::table> l_ib, r_ib;
  if (nvl != world) {
    CommunicationGroup inter(world, nvl, communicator->mpi_rank);
    l_ib = shuffle_on(left, left_on, inter, communicator, left_compression_options,
                      cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTER, report_timing,
                      preallocated_pinned_buffer);
    r_ib = shuffle_on(right, ron, inter, communicator, right_compression_options,
                      cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTER, report_timing,
                      preallocated_pinned_buffer);
    left = l_ib->view();
    right = r_ib->view();
  }
  if (nvl == 1) return local_join(kind, left, right, left_on, ron);

  /* shuffle + local join, the route composite and nullable keys take in the
   * inner join: after the shuffle every right row that could match a left
   * row sits on that row's rank, so matched / unmatched is decided locally.
   * Every rank takes this route whatever its masks, so there is no route to
   * disagree on (tag 0); over_decom_factor has no effect here. */
  CommunicationGroup g2(nvl, 1, communicator->mpi_rank);
  auto ls = shuffle_on_tagged(left, left_on, g2, communicator, left_compression_options,
                              cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTRA, report_timing,
                              preallocated_pinned_buffer, 0u);
  auto rs = shuffle_on_tagged(right, ron, g2, communicator, right_compression_options,
                              cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTRA, report_timing,
                              preallocated_pinned_buffer, 0u);
  return local_join(kind, ls->view(), rs->view(), left_on, ron);
}

std::unique_ptr<cudf::table> distributed_left_join(
  cudf::table_view left, cudf::table_view right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options, int over_decom_factor,
  bool report_timing, void* preallocated_pinned_buffer, int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  return distributed_join(join_kind::LEFT, left, right, left_on, right_on, communicator,
                          std::move(left_compression_options),
                          std::move(right_compression_options), over_decom_factor,
                          report_timing, preallocated_pinned_buffer, nvlink_domain_size,
                          compare_nulls);
}

std::unique_ptr<cudf::table> distributed_left_semi_join(
  cudf::table_view left, cudf::table_view right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options, int over_decom_factor,
  bool report_timing, void* preallocated_pinned_buffer, int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  return distributed_join(join_kind::LEFT_SEMI, left, right, left_on, right_on, communicator,
                          std::move(left_compression_options),
                          std::move(right_compression_options), over_decom_factor,
                          report_timing, preallocated_pinned_buffer, nvlink_domain_size,
                          compare_nulls);
}

std::unique_ptr<cudf::table> distributed_left_anti_join(
  cudf::table_view left, cudf::table_view right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options, int over_decom_factor,
  bool report_timing, void* preallocated_pinned_buffer, int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  return distributed_join(join_kind::LEFT_ANTI, left, right, left_on, right_on, communicator,
                          std::move(left_compression_options),
                          std::move(right_compression_options), over_decom_factor,
                          report_timing, preallocated_pinned_buffer, nvlink_domain_size,
                          compare_nulls);
}


/* ------------------------------------------------------------- shuffle_on */

static std::unique_ptr<cudf::table> shuffle_on_tagged(
  cudf::table_view const& input, std::vector<cudf::size_type> const& on_columns,
  CommunicationGroup comm_group, Communicator* communicator,
  std::vector<ColumnCompressionOptions> compression_options, cudf::hash_id hash_function,
  uint32_t hash_seed, bool report_timing, void* preallocated_pinned_buffer, uint32_t route_tag)
{
  DJ_CHECK_ERROR(on_columns.size() >= 1, "shuffle_on: at least one key column");
  const int hash_fn =
    hash_function == cudf::hash_id::HASH_IDENTITY ? DJ_HASH_IDENTITY : DJ_HASH_MURMUR3;
  DJ_CHECK_ERROR(on_columns.size() <= 4, "shuffle_on: up to 4 key columns supported");
  validate_compression(input, compression_options);
  PartitionedTable part = place_rows(input, on_columns, comm_group.size(), hash_fn, hash_seed);
  auto atoa = AllToAllCommunicatorAccess::make(part.tbl->view(), part.offsets, comm_group,
                                               communicator, compression_options, false,
                                               route_tag);
  auto out = atoa->allocate_communicated_table();
  atoa->launch_communication(out->mutable_view(), report_timing, preallocated_pinned_buffer);
  return out;
}

std::unique_ptr<cudf::table> shuffle_on(cudf::table_view const& input,
                                        std::vector<cudf::size_type> const& on_columns,
                                        CommunicationGroup comm_group,
                                        Communicator* communicator,
                                        std::vector<ColumnCompressionOptions> compression_options,
                                        cudf::hash_id hash_function,
                                        uint32_t hash_seed,
                                        bool report_timing,
                                        void* preallocated_pinned_buffer)
{
  return shuffle_on_tagged(input, on_columns, comm_group, communicator,
                           std::move(compression_options), hash_function, hash_seed,
                           report_timing, preallocated_pinned_buffer, 0u);
}

std::unique_ptr<cudf::table> shuffle_on(cudf::table_view const& input,
                                        std::vector<cudf::size_type> const& on_columns,
                                        Communicator* communicator,
                                        std::vector<ColumnCompressionOptions> compression_options,
                                        cudf::hash_id hash_function,
                                        uint32_t hash_seed,
                                        bool report_timing,
                                        void* preallocated_pinned_buffer)
{
  return shuffle_on(input, on_columns,
                    CommunicationGroup(communicator->mpi_size, 1, communicator->mpi_rank),
                    communicator, std::move(compression_options), hash_function, hash_seed,
                    report_timing, preallocated_pinned_buffer);
}

/* --------------------------------------------------------- distribute_table */

using dj::kMaxSchemaCols;

std::unique_ptr<cudf::table> distribute_table(cudf::table_view global_table,
                                              Communicator* communicator)
{
  const int G = communicator->mpi_size;
  const int rank = communicator->mpi_rank;
  hipStream_t st = dj_rt_stream();
  check_no_masks(global_table, "distribute_table");

  /* schema + per-rank row counts: root sends [nrows_r, ncols, dtype ids...] */
  std::vector<int64_t> header(2 + kMaxSchemaCols, 0);
  if (rank == 0) {
    DJ_CHECK_ERROR(global_table.num_columns() <= kMaxSchemaCols, "too many columns");
    header[1] = global_table.num_columns();
    for (cudf::size_type c = 0; c < global_table.num_columns(); c++)
      header[2 + c] = (int64_t)global_table.column(c).type().id();
  }
  int64_t total = rank == 0 ? global_table.num_rows() : 0;
  DBuf d_hdr((size_t)header.size() * 8 * (rank == 0 ? G : 1));
  if (G > 1) {
    if (rank == 0) {
      std::vector<int64_t> all;
      for (int r = 0; r < G; r++) {
        int64_t rows_r = total / G + (r < total % G ? 1 : 0);
        header[0] = rows_r;
        all.insert(all.end(), header.begin(), header.end());
      }
      DJ_HIP_CALL(hipMemcpyAsync(d_hdr.p, all.data(), all.size() * 8, hipMemcpyHostToDevice, st));
      DJ_HIP_CALL(hipStreamSynchronize(st));
    }
    communicator->start();
    if (rank == 0) {
      for (int r = 1; r < G; r++)
        communicator->send(d_hdr.i64() + (size_t)r * header.size(), header.size(), 8, r);
    } else {
      communicator->recv(d_hdr.i64(), header.size(), 8, 0);
    }
    communicator->stop();
    if (rank != 0) {
      DJ_HIP_CALL(hipMemcpyAsync(header.data(), d_hdr.p, header.size() * 8,
                                 hipMemcpyDeviceToHost, st));
      DJ_HIP_CALL(hipStreamSynchronize(st));
    } else {
      header[0] = total / G + (0 < total % G ? 1 : 0);
    }
  } else {
    header[0] = total;
  }

  const int64_t my_rows = header[0];
  const int ncols = (int)header[1];
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (int c = 0; c < ncols; c++)
    cols.push_back(std::make_unique<cudf::column>(
      cudf::data_type((cudf::type_id)header[2 + c]), (cudf::size_type)my_rows));
  auto local = std::make_unique<cudf::table>(std::move(cols));

  /* row data: root sends each rank its contiguous slice */
  communicator->start();
  if (rank == 0) {
    int64_t row0 = 0;
    for (int r = 0; r < G; r++) {
      int64_t rows_r = total / G + (r < total % G ? 1 : 0);
      for (int c = 0; c < ncols; c++) {
        const int esize = cudf::size_of(global_table.column(c).type());
        const int8_t* src = global_table.column(c).head<int8_t>() + row0 * esize;
        if (r == 0) {
          DJ_HIP_CALL(hipMemcpyAsync(local->get_column(c).head(), src, (size_t)rows_r * esize,
                                     hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
        } else {
          communicator->send(src, rows_r, esize, r);
        }
      }
      row0 += rows_r;
    }
  } else {
    for (int c = 0; c < ncols; c++) {
      const int esize = cudf::size_of(local->get_column(c).type());
      communicator->recv(local->get_column(c).head(), my_rows, esize, 0);
    }
  }
  communicator->stop();
  return local;
}

std::unique_ptr<cudf::table> collect_tables(cudf::table_view table, Communicator* communicator)
{
  const int G = communicator->mpi_size;
  const int rank = communicator->mpi_rank;
  CommunicationGroup group(G, 1, rank);
  check_no_masks(table, "collect_tables");

  /* per-rank row counts to root via communicate_sizes (send all rows to
   * local rank 0) */
  std::vector<int64_t> send_offset(G + 1, (int64_t)table.num_rows());
  send_offset[0] = 0;
  std::vector<int64_t> recv_offset;
  communicate_sizes(send_offset, recv_offset, group, communicator);

  std::unique_ptr<cudf::table> merged;
  if (rank == 0) {
    std::vector<std::unique_ptr<cudf::column>> cols;
    for (cudf::size_type c = 0; c < table.num_columns(); c++)
      cols.push_back(std::make_unique<cudf::column>(table.column(c).type(),
                                                    (cudf::size_type)recv_offset.back()));
    merged = std::make_unique<cudf::table>(std::move(cols));
  }

  communicator->start();
  for (cudf::size_type c = 0; c < table.num_columns(); c++) {
    const int esize = cudf::size_of(table.column(c).type());
    if (rank == 0) {
      for (int r = 0; r < G; r++) {
        int64_t count = recv_offset[r + 1] - recv_offset[r];
        int8_t* dst = (int8_t*)merged->get_column(c).head() + recv_offset[r] * esize;
        if (r == 0) {
          DJ_HIP_CALL(hipMemcpyAsync(dst, table.column(c).head<int8_t>(),
                                     (size_t)count * esize, hipMemcpyDeviceToDevice,
                                     dj_rt_comm_stream()));
        } else {
          communicator->recv(dst, count, esize, r);
        }
      }
    } else {
      communicator->send(table.column(c).head<int8_t>(), table.num_rows(), esize, 0);
    }
  }
  communicator->stop();
  return merged;  // nullptr on non-root ranks
}

/* --------------------------- C ABI over the C++ orchestration (for the
 * Python measurement harness; additive — SURVEY.md §8b) ------------------ */

namespace {

/* dj_col_desc[nc] (include/distributed_join.h) -> table view of n rows */
cudf::table_view view_from_descs(const dj_col_desc* cols, int nc, int64_t n)
{
  using cudf::data_type;
  using cudf::type_id;
  std::vector<cudf::column_view> v;
  for (int c = 0; c < nc; c++) {
    if ((type_id)cols[c].type_id == type_id::STRING)
      v.emplace_back(data_type(type_id::STRING), (cudf::size_type)n, cols[c].data,
                     cols[c].chars, cols[c].chars_bytes);
    else
      v.emplace_back(data_type((type_id)cols[c].type_id), (cudf::size_type)n, cols[c].data);
  }
  return cudf::table_view(v);
}

/* dj_ncol_desc[nc] -> table view of n rows, masks attached */
cudf::table_view view_from_ndescs(const dj_ncol_desc* cols, int nc, int64_t n)
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

/* DJ_HASH_* of the C header -> cudf::hash_id */
cudf::hash_id to_hash_id(int hash_function)
{
  return hash_function == DJ_HASH_IDENTITY ? cudf::hash_id::HASH_IDENTITY
                                           : cudf::hash_id::HASH_MURMUR3;
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

/* RCCL self-test: world-1 ncclCommInitRank + grouped self send/recv through
 * the real RCCLCommunicator start/send/recv/stop path (the same calls the
 * N>1 exchange makes per peer slice). Validates RCCL init + group + stream
 * semantics on a single GPU before any multi-GPU run. Returns 0 on success,
 * 1 on payload mismatch (RCCL/HIP errors abort via DJ_*_CALL). */
int dj_rccl_selftest(int64_t n)
{
  std::vector<uint8_t> idb((size_t)rccl_unique_id_size());
  rccl_unique_id(idb.data());
  RCCLCommunicator comm(0, 1, idb.data());
  std::vector<uint8_t> h_src((size_t)n), h_dst((size_t)n, 0);
  for (int64_t i = 0; i < n; i++) h_src[(size_t)i] = (uint8_t)(dj_mix64((uint64_t)i) & 0xFF);
  void *d_src = nullptr, *d_dst = nullptr;
  DJ_HIP_CALL(hipMalloc(&d_src, (size_t)n));
  DJ_HIP_CALL(hipMalloc(&d_dst, (size_t)n));
  DJ_HIP_CALL(hipMemcpy(d_src, h_src.data(), (size_t)n, hipMemcpyHostToDevice));
  DJ_HIP_CALL(hipMemset(d_dst, 0, (size_t)n));
  comm.start();
  comm.send(d_src, n, 1, 0);
  comm.recv(d_dst, n, 1, 0);
  comm.stop();
  DJ_HIP_CALL(hipMemcpy(h_dst.data(), d_dst, (size_t)n, hipMemcpyDeviceToHost));
  DJ_HIP_CALL(hipFree(d_src));
  DJ_HIP_CALL(hipFree(d_dst));
  comm.finalize();
  return h_src == h_dst ? 0 : 1;
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
  int32_t total = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&total, offsets + n, 4, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
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
  using cudf::column_view;
  using cudf::data_type;
  using cudf::type_id;
  cudf::table_view left(
    {column_view(data_type(type_id::INT64), (cudf::size_type)ln, d_lk),
     column_view(data_type(type_id::STRING), (cudf::size_type)ln, l_offsets, l_chars,
                 l_chars_bytes)});
  cudf::table_view right(
    {column_view(data_type(type_id::INT64), (cudf::size_type)rn, d_rk),
     column_view(data_type(type_id::STRING), (cudf::size_type)rn, r_offsets, r_chars,
                 r_chars_bytes)});
  auto opts = generate_compression_options_distributed(left, false);
  auto result = distributed_inner_join(left, right, {0}, {0}, (Communicator*)comm, opts, opts,
                                       over_decom, report_timing != 0, nullptr, 1);
  return result.release();
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
  auto left = view_from_descs(lcols, nl, ln);
  auto right = view_from_descs(rcols, nr, rn);
  std::vector<cudf::size_type> lo(lon, lon + nkeys), ro(ron, ron + nkeys);
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  auto result = distributed_inner_join(left, right, lo, ro, (Communicator*)comm, lopts,
                                       ropts, over_decom, report_timing != 0, nullptr, 1);
  return result.release();
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
 * ones included (placement on the fused key chain, dj_hash.h).
 * compression: 0 = none, 1 = the fixed bitpack policy
 * (generate_compression_options_distributed), 2 = sampling auto-select
 * (generate_auto_select_compression_options), 3 = an explicit bitpack
 * cascaded option on EVERY column, whatever its type (reaches the option
 * validation: a loud error on FLOAT32/FLOAT64/BOOL8 columns). */
void* dj_cpp_shuffle_on_cols(void* comm, const dj_col_desc* cols, int nc, int64_t n,
                             const int32_t* on, int nkeys, int hash_function, uint32_t seed,
                             int compression)
{
  cudf::table_view input = view_from_descs(cols, nc, n);
  std::vector<cudf::size_type> keys(on, on + nkeys);
  std::vector<ColumnCompressionOptions> opts;
  if (compression == 2) {
    opts = generate_auto_select_compression_options(input);
  } else if (compression == 3) {
    nvcompCascadedFormatOpts bp{};
    bp.use_bp = 1;
    opts.assign((size_t)nc, ColumnCompressionOptions(CompressionMethod::cascaded, bp));
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

/* test hook: the placement step of shuffle_on alone (place_rows, the very
 * function shuffle_on calls before its all-to-all). Partitions the table
 * into nparts contiguous ranges and writes the nparts+1 row offsets to
 * h_offsets. Lets one GPU check placement against the dj_hash.h spec for
 * nparts > 1. */
void* dj_cpp_partition_cols(const dj_col_desc* cols, int nc, int64_t n, const int32_t* on,
                            int nkeys, int nparts, int hash_function, uint32_t seed,
                            int64_t* h_offsets)
{
  DJ_CHECK_ERROR(nkeys >= 1 && nkeys <= 4, "partition: 1..4 key columns");
  DJ_CHECK_ERROR(nparts >= 1 && nparts <= dj::kMaxPartitions, "partition: 1..1024 parts");
  std::vector<cudf::size_type> keys(on, on + nkeys);
  PartitionedTable part =
    place_rows(view_from_descs(cols, nc, n), keys, nparts,
               hash_function == DJ_HASH_IDENTITY ? DJ_HASH_IDENTITY : DJ_HASH_MURMUR3, seed);
  for (int i = 0; i <= nparts; i++) h_offsets[i] = part.offsets[(size_t)i];
  return part.tbl.release();
}

/* the nullable-descriptor forms of the three entry points above */
void* dj_cpp_distributed_inner_join_ncols_multi(void* comm, const dj_ncol_desc* lcols, int nl,
                                                int64_t ln, const dj_ncol_desc* rcols, int nr,
                                                int64_t rn, const int32_t* lon,
                                                const int32_t* ron, int nkeys, int over_decom,
                                                int report_timing)
{
  auto left = view_from_ndescs(lcols, nl, ln);
  auto right = view_from_ndescs(rcols, nr, rn);
  std::vector<cudf::size_type> lo(lon, lon + nkeys), ro(ron, ron + nkeys);
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  auto result = distributed_inner_join(left, right, lo, ro, (Communicator*)comm, lopts,
                                       ropts, over_decom, report_timing != 0, nullptr, 1);
  return result.release();
}

void* dj_cpp_shuffle_on_ncols(void* comm, const dj_ncol_desc* cols, int nc, int64_t n,
                              const int32_t* on, int nkeys, int hash_function, uint32_t seed,
                              int compression)
{
  cudf::table_view input = view_from_ndescs(cols, nc, n);
  std::vector<cudf::size_type> keys(on, on + nkeys);
  auto opts = generate_compression_options_distributed(input, compression != 0);
  auto result = shuffle_on(input, keys, (Communicator*)comm, opts, to_hash_id(hash_function),
                           seed, false, nullptr);
  return result.release();
}

void* dj_cpp_partition_ncols(const dj_ncol_desc* cols, int nc, int64_t n, const int32_t* on,
                             int nkeys, int nparts, int hash_function, uint32_t seed,
                             int64_t* h_offsets)
{
  DJ_CHECK_ERROR(nkeys >= 1 && nkeys <= 4, "partition: 1..4 key columns");
  DJ_CHECK_ERROR(nparts >= 1 && nparts <= dj::kMaxPartitions, "partition: 1..1024 parts");
  std::vector<cudf::size_type> keys(on, on + nkeys);
  PartitionedTable part =
    place_rows(view_from_ndescs(cols, nc, n), keys, nparts,
               hash_function == DJ_HASH_IDENTITY ? DJ_HASH_IDENTITY : DJ_HASH_MURMUR3, seed);
  for (int i = 0; i <= nparts; i++) h_offsets[i] = part.offsets[(size_t)i];
  return part.tbl.release();
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
  unsigned long long h = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&h, cnt.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return (int64_t)h;
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
  auto left = view_from_ndescs(lcols, nl, ln);
  auto right = view_from_ndescs(rcols, nr, rn);
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
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipEventRecord(e0, st));
    dj::mark_rows(d_idx, n, (uint32_t*)d_bits, st, mode < 0 ? dj::kMarkDefault : mode);
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
}

int64_t dj_select_rows(const void* d_bits, int64_t nrows, int want_set, int64_t* d_out_idx,
                       int reps, double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  DBuf scratch(dj::select_rows_scratch_bytes(nrows)), count(8);
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipEventRecord(e0, st));
    dj::select_rows((const uint32_t*)d_bits, nrows, want_set != 0, d_out_idx, count.i64(), st,
                    scratch.p);
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
  int64_t h = 0;
  DJ_HIP_CALL(hipMemcpy(&h, count.p, 8, hipMemcpyDeviceToHost));
  return h;
}

int64_t dj_compact_keyed_rows(const void* d_bits, int64_t nrows, const int64_t* d_keys,
                              int64_t* d_out_idx, int64_t* d_out_keys, int reps, double* h_ms)
{
  hipStream_t st = dj_rt_stream();
  DBuf scratch(dj::select_rows_scratch_bytes(nrows)), count(8);
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipEventRecord(e0, st));
    dj::compact_keyed_rows((const uint32_t*)d_bits, nrows, d_keys, d_out_idx, d_out_keys,
                           count.i64(), st, scratch.p);
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
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
  unsigned long long h = 0;
  DJ_HIP_CALL(hipMemcpyAsync(&h, cnt.p, 8, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return (int64_t)h;
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
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipEventRecord(e0, st));
    dj::gather_table(gc.data(), ncols, d_idx, n, mode, st);
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
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
  hipEvent_t e0, e1;
  DJ_HIP_CALL(hipEventCreate(&e0));
  DJ_HIP_CALL(hipEventCreate(&e1));
  for (int r = 0; r < (reps > 0 ? reps : 1); r++) {
    DJ_HIP_CALL(hipEventRecord(e0, st));
    dj::hash_strings((const int32_t*)d_offsets, (const uint8_t*)d_chars, n, d_out, st);
    DJ_HIP_CALL(hipEventRecord(e1, st));
    DJ_HIP_CALL(hipEventSynchronize(e1));
    float ms = 0.f;
    DJ_HIP_CALL(hipEventElapsedTime(&ms, e0, e1));
    if (h_ms) h_ms[r] = ms;
  }
  DJ_HIP_CALL(hipEventDestroy(e0));
  DJ_HIP_CALL(hipEventDestroy(e1));
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
