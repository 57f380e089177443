/*
 * loopback.hpp — the transport of the *_loopback programs: G ranks as host
 * threads on ONE GPU, each with a LoopbackComm, handing device buffers over
 * through an in-process mailbox with D2D copies. The mailbox counts every
 * send/recv call and byte.
 *
 * Needs only communicator.hpp, HIP and the standard library, so a program
 * that includes it can still be compiled against an older interface.
 */
#pragma once

#include "check.hpp" /* CHECK, FAIL */
#include "communicator.hpp"

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

struct Mailbox {
  struct Msg {
    const void* src;
    size_t bytes;
    bool consumed;
  };
  std::mutex m;
  std::condition_variable cv;
  std::map<std::tuple<int, int, long>, Msg> msgs;  // (src, dst, seq of the pair)
  std::map<std::pair<int, int>, long> send_seq, recv_seq;
  std::atomic<long long> sends{0}, recvs{0}, send_bytes{0}, recv_bytes{0};

  void post(int src, int dst, const void* buf, size_t bytes)
  {
    std::lock_guard<std::mutex> g(m);
    msgs[{src, dst, send_seq[{src, dst}]++}] = Msg{buf, bytes, false};
    cv.notify_all();
  }
  /* blocks until the matching send arrives, then D2D-copies it */
  void fetch(int src, int dst, void* out, size_t bytes)
  {
    std::unique_lock<std::mutex> g(m);
    const long seq = recv_seq[{src, dst}]++;
    cv.wait(g, [&] { return msgs.count({src, dst, seq}) != 0; });
    Msg& msg = msgs[{src, dst, seq}];
    if (msg.bytes != bytes) FAIL("loopback size mismatch %zu vs %zu", msg.bytes, bytes);
    if (bytes) CHECK(hipMemcpy(out, msg.src, bytes, hipMemcpyDeviceToDevice));
    msg.consumed = true;
    cv.notify_all();
  }
  void drain(int src)
  {
    std::unique_lock<std::mutex> g(m);
    cv.wait(g, [&] {
      for (auto& kv : msgs)
        if (std::get<0>(kv.first) == src && !kv.second.consumed) return false;
      return true;
    });
  }
};

/* user-style Communicator implementation against the public header */
class LoopbackComm : public Communicator {
 public:
  LoopbackComm(int rank, int size, Mailbox* mb) : mb_(mb)
  {
    mpi_rank = rank;
    mpi_size = size;
    current_device = 0;
  }
  void initialize() override {}
  void start() override {}
  void stop() override
  {
    /* block until every posted send was consumed and device work drained —
     * the blocking contract of Communicator::stop */
    mb_->drain(mpi_rank);
    CHECK(hipDeviceSynchronize());
  }
  void send(const void* buf, int64_t count, int element_size, int dest) override
  {
    CHECK(hipDeviceSynchronize());  // payload must be ready before posting
    mb_->sends++;
    mb_->send_bytes += (long long)count * element_size;
    mb_->post(mpi_rank, dest, buf, (size_t)count * element_size);
  }
  void recv(void* buf, int64_t count, int element_size, int source) override
  {
    mb_->recvs++;
    mb_->recv_bytes += (long long)count * element_size;
    mb_->fetch(source, mpi_rank, buf, (size_t)count * element_size);
  }
  void finalize() override {}
  bool group_by_batch() override { return true; }

 private:
  Mailbox* mb_;
};

/* body(rank, comm) on G threads, one LoopbackComm each; returns when all did */
template <class F>
static void run_ranks(int G, Mailbox* mb, F body)
{
  std::vector<std::thread> th;
  for (int r = 0; r < G; r++)
    th.emplace_back([&, r] {
      CHECK(hipSetDevice(0));
      LoopbackComm comm(r, G, mb);
      body(r, &comm);
    });
  for (auto& t : th) t.join();
}
