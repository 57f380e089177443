/*
 * dj_devmem.hip — device memory of the host orchestration layer: the caching
 * allocator behind DBuf and cudf::column, the stream syncs, the scalar
 * read-back and the mask segment copy (dj_host.hpp).
 */
#include "dj_host.hpp"

#include <map>
#include <mutex>
#include <unordered_map>

namespace dj_host {

namespace {

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

/* the process's one pool: reachable only through pool_alloc / pool_free below */
CachingAllocator& pool()
{
  static CachingAllocator a;
  return a;
}

}  // namespace

void* pool_alloc(size_t bytes) { return pool().alloc(bytes); }
void pool_free(void* p) { pool().dealloc(p); }

void sync_streams()
{
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_stream()));
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
}

void read_back_bytes(void* h, const void* d, size_t bytes, hipStream_t st)
{
  DJ_HIP_CALL(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st));
  DJ_HIP_CALL(hipStreamSynchronize(st));
}

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

}  // namespace dj_host
