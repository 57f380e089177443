/*
 * harness_selftest.cpp — the shared code of the programs in this folder,
 * tested directly at the smallest shapes at which each piece can go wrong.
 *
 *   transport (loopback.hpp): G = 3 ranks; inside one start/stop every
 *     ordered pair exchanges three messages back to back, of 0, 1 and 4097
 *     bytes, whose contents are a formula of (src, dst, seq, position). Every
 *     received byte is checked, the poison behind each receive buffer must be
 *     untouched, and the mailbox's counters must read the closed form:
 *     sends = recvs = 3 * G * (G-1), bytes = 4098 * G * (G-1);
 *   host table (host_table.hpp): from_device(to_device(t)) == t cell for
 *     cell, mask and valid included, for n in {0, 1, 32, 33} (the edges of
 *     the mask word), columns INT8, INT16, INT32, INT64 with negative values
 *     and STRING with an empty and an 8-character string, each with and
 *     without a mask; for n >= 1 rows 0 and n-1 are null; row_hash changes
 *     when one validity bit flips;
 *   bucket model (bucket_model.hpp), host only: for F in {64, 256, 512, 1024}
 *     and PA in {4, 1024}, over 4096 hkey keys, bucket_of < PA * F and
 *     bucket_of / F == group_of.
 *
 * usage: harness_selftest
 * Build/run: tests/test_gpu_harness_selftest.py.
 */
#include "bucket_model.hpp"
#include "host_table.hpp"
#include "loopback.hpp"

#include <string>
#include <vector>

/* ---------------- transport ---------------- */

constexpr int kRanks = 3, kMsgs = 3;
constexpr size_t kMsgBytes[kMsgs] = {0, 1, 4097};
constexpr size_t kTail = 16; /* poison behind every receive buffer */

static unsigned char msg_byte(int src, int dst, int seq, size_t i)
{
  return (unsigned char)(src * 131 + dst * 31 + seq * 7 + i * 13 + (i >> 8));
}

static void check_transport()
{
  Mailbox mb;
  run_ranks(kRanks, &mb, [&](int r, Communicator* comm) {
    unsigned char *send[kRanks][kMsgs] = {}, *recv[kRanks][kMsgs] = {};
    for (int peer = 0; peer < kRanks; peer++) {
      if (peer == r) continue;
      for (int q = 0; q < kMsgs; q++) {
        const size_t n = kMsgBytes[q];
        std::vector<unsigned char> h(n);
        for (size_t i = 0; i < n; i++) h[i] = msg_byte(r, peer, q, i);
        /* the 0-byte message is sent from a null pointer */
        if (n) {
          CHECK(hipMalloc(&send[peer][q], n));
          CHECK(hipMemcpy(send[peer][q], h.data(), n, hipMemcpyHostToDevice));
        }
        CHECK(hipMalloc(&recv[peer][q], n + kTail));
        CHECK(hipMemset(recv[peer][q], kPoison, n + kTail));
      }
    }
    comm->start();
    for (int peer = 0; peer < kRanks; peer++) {
      if (peer == r) continue;
      for (int q = 0; q < kMsgs; q++) comm->send(send[peer][q], (int64_t)kMsgBytes[q], 1, peer);
    }
    for (int peer = 0; peer < kRanks; peer++) {
      if (peer == r) continue;
      for (int q = 0; q < kMsgs; q++) comm->recv(recv[peer][q], (int64_t)kMsgBytes[q], 1, peer);
    }
    comm->stop();
    for (int peer = 0; peer < kRanks; peer++) {
      if (peer == r) continue;
      for (int q = 0; q < kMsgs; q++) {
        const size_t n = kMsgBytes[q];
        std::vector<unsigned char> h(n + kTail);
        CHECK(hipMemcpy(h.data(), recv[peer][q], n + kTail, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++)
          if (h[i] != msg_byte(peer, r, q, i))
            FAIL("TRANSPORT: rank %d, message %d from %d: byte %zu is %d, want %d", r, q, peer, i,
                 (int)h[i], (int)msg_byte(peer, r, q, i));
        if (!all_poison(h.data() + n, kTail))
          FAIL("TRANSPORT: rank %d, message %d from %d wrote past its %zu bytes", r, q, peer, n);
        if (send[peer][q]) CHECK(hipFree(send[peer][q]));
        CHECK(hipFree(recv[peer][q]));
      }
    }
  });
  const long long calls = 3LL * kRanks * (kRanks - 1), bytes = 4098LL * kRanks * (kRanks - 1);
  if (mb.sends.load() != calls || mb.recvs.load() != calls || mb.send_bytes.load() != bytes ||
      mb.recv_bytes.load() != bytes)
    FAIL("TRANSPORT: counters sends=%lld recvs=%lld send_bytes=%lld recv_bytes=%lld, want %lld "
         "calls and %lld bytes",
         mb.sends.load(), mb.recvs.load(), mb.send_bytes.load(), mb.recv_bytes.load(), calls,
         bytes);
  printf("transport G=%d: %lld sends, %lld bytes: ok\n", kRanks, calls, bytes);
}

/* ---------------- host table ---------------- */

static HTable sample_table(size_t n, bool mask)
{
  const cudf::type_id types[] = {cudf::type_id::INT8, cudf::type_id::INT16, cudf::type_id::INT32,
                                 cudf::type_id::INT64, cudf::type_id::STRING};
  const int64_t base[] = {1, 300, 70000, 5000000000LL};
  HTable t;
  for (int c = 0; c < 5; c++) {
    HCol col;
    col.type = types[c];
    col.mask = mask;
    for (size_t i = 0; i < n; i++) {
      if (c < 4)  // negative on even rows, so row 0 and a 1-row table sign-extend
        col.v.push_back((i % 2 ? 1 : -1) * (base[c] + (int64_t)i));
      else
        col.s.push_back(i % 3 == 0 ? std::string() : i % 3 == 1 ? std::string("abcdefgh")
                                                               : str_of(i));
      col.valid.push_back(!(mask && (i == 0 || i == n - 1)));
    }
    t.push_back(col);
  }
  return t;
}

static void check_round_trip(size_t n, bool mask)
{
  const HTable t = sample_table(n, mask);
  const HTable back = from_device(*to_device(t));
  if (back.size() != t.size())
    FAIL("HOST TABLE: %zu columns came back, not %zu", back.size(), t.size());
  for (size_t c = 0; c < t.size(); c++) {
    if (back[c].type != t[c].type || back[c].mask != t[c].mask)
      FAIL("HOST TABLE n=%zu mask=%d: column %zu came back as type %d mask %d", n, (int)mask, c,
           (int)back[c].type, (int)back[c].mask);
    if (back[c].valid != t[c].valid || back[c].v != t[c].v || back[c].s != t[c].s)
      FAIL("HOST TABLE n=%zu mask=%d: column %zu differs after the round trip", n, (int)mask, c);
  }
  if (rows_of(back) != n) FAIL("HOST TABLE: rows_of %zu, not %zu", rows_of(back), n);
  printf("host table n=%zu mask=%d: ok\n", n, (int)mask);
}

static void check_row_hash()
{
  HTable t = sample_table(33, true);
  for (size_t c = 0; c < t.size(); c++)
    for (size_t i : {(size_t)0, (size_t)16, (size_t)32}) {
      const uint64_t before = row_hash(t, 0, t.size(), i);
      t[c].valid[i] ^= 1;
      if (row_hash(t, 0, t.size(), i) == before)
        FAIL("HOST TABLE: row_hash blind to the validity bit of column %zu, row %zu", c, i);
      t[c].valid[i] ^= 1;
      if (row_hash(t, 0, t.size(), i) != before) FAIL("HOST TABLE: row_hash not a function");
    }
  printf("row_hash validity: ok\n");
}

/* ---------------- bucket model ---------------- */

static void check_bucket_model()
{
  for (int F : {64, 256, 512, 1024})
    for (int PA : {4, 1024}) {
      for (uint64_t i = 0; i < 4096; i++) {
        const int64_t k = hkey(1, i);
        const uint32_t b = bucket_of(k, PA, F);
        if (b >= (uint32_t)PA * (uint32_t)F || b / (uint32_t)F != group_of(k, PA))
          FAIL("BUCKET MODEL F=%d PA=%d: key %llu in bucket %u, group %u", F, PA,
               (unsigned long long)i, b, group_of(k, PA));
      }
      printf("bucket model F=%d PA=%d: ok\n", F, PA);
    }
}

int main()
{
  check_bucket_model();
  CHECK(hipSetDevice(0));
  check_transport();
  for (size_t n : {(size_t)0, (size_t)1, (size_t)32, (size_t)33})
    for (bool mask : {false, true}) check_round_trip(n, mask);
  check_row_hash();
  printf("HARNESS SELFTEST OK\n");
  return 0;
}
