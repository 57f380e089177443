/*
 * dj_comm.hip — the transports behind include/communicator.hpp:
 * RCCLCommunicator (grouped send/recv over xGMI), the default communicator
 * and the RCCL self-test. LocalCommunicator, the size-1 stand-in, is inline
 * in dj_host.hpp.
 */
#include "dj_host.hpp"
#include "dj_rng.h"

#include <rccl/rccl.h>

#include <cstring>

using namespace dj_host;

Communicator* dj_host::g_default_comm = nullptr;

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

/* RCCL self-test: world-1 ncclCommInitRank + grouped self send/recv through
 * the real RCCLCommunicator start/send/recv/stop path (the same calls the
 * N>1 exchange makes per peer slice). Validates RCCL init + group + stream
 * semantics on a single GPU before any multi-GPU run. Returns 0 on success,
 * 1 on payload mismatch (RCCL/HIP errors abort via DJ_*_CALL). */
extern "C" int dj_rccl_selftest(int64_t n)
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
