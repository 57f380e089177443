/*
 * null_loopback.cpp — validity masks across G ranks on ONE GPU. Ranks run as
 * host threads over a loopback implementation of the public Communicator
 * interface (the transport of stringkey_loopback.cpp), which here also counts
 * its send/recv calls and bytes.
 *
 * usage: null_loopback G rows_per_rank
 *
 * Checks (global tables of G * rows_per_rank rows, a formula of the row):
 *   1. shuffle_on on a nullable INT64 key: no row, value or validity bit is
 *      lost; every null-key row sits on rank 0xFFFFFFFF % G; a valid key
 *      lives on one rank;
 *   2. distributed_inner_join on a nullable key (null == null, the a*b cross
 *      product included; garbage under nulls equal to valid keys of the other
 *      side) against a host join of the global tables: row count and an
 *      order-insensitive checksum over every value and validity bit;
 *   3. the same with a non-nullable key, nullable payloads and
 *      over_decom_factor 2 (the batched pipeline);
 *   in 1-3 one rank passes one payload column WITHOUT a mask while the others
 *   pass masks: the output column still has a mask on every rank;
 *   4. distribute_table, collect_tables and the generic plan API refuse a
 *      nullable table with an exception, before any communication;
 *   5. mask-free tables: the Communicator sees exactly the send/recv calls
 *      and bytes it saw before masks existed. The program prints them as a
 *      "COUNTS" line; tests/test_gpu_nulls.py holds the values recorded from
 *      the commit before validity masks.
 *
 * Built with -DNULL_LOOPBACK_COUNTS_ONLY the program contains check 5 alone
 * and uses nothing newer than the mask-free interface (that is how the
 * recorded values were taken).
 *
 * Build/run: tests/test_gpu_nulls.py::test_null_loopback.
 */
#include "all_to_all_comm.hpp"
#include "communicator.hpp"
#include "compression.hpp"
#include "distribute_table.hpp"
#include "distributed_join.hpp"
#include "shuffle_on.hpp"

#include "../../distributed_join_amd/csrc/dj_rng.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#define CHECK(c)                                                      \
  do {                                                                \
    hipError_t e = (c);                                               \
    if (e != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    exit(1);             \
  } while (0)

/* ---------------- loopback transport (counting) ---------------- */

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
    mb_->drain(mpi_rank);
    CHECK(hipDeviceSynchronize());
  }
  void send(const void* buf, int64_t count, int element_size, int dest) override
  {
    CHECK(hipDeviceSynchronize());
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

static std::string str_of(uint64_t id)
{
  const int len = (int)(id % 9);
  std::string s((size_t)len, 'a');
  for (int k = 0; k < len; k++) s[(size_t)k] = (char)('a' + dj_mix64(id * 16 + (uint64_t)k) % 26);
  return s;
}

/* ---------------- check 5: mask-free call and byte counts ---------------- */

static std::unique_ptr<cudf::column> device_fixed(cudf::type_id type, const void* data,
                                                  int64_t rows, int width)
{
  auto col = std::make_unique<cudf::column>(cudf::data_type(type), (cudf::size_type)rows);
  if (rows) CHECK(hipMemcpy(col->head(), data, (size_t)rows * width, hipMemcpyHostToDevice));
  return col;
}

static std::unique_ptr<cudf::column> device_strings(const std::vector<std::string>& s)
{
  std::vector<int32_t> off(s.size() + 1, 0);
  std::string chars;
  for (size_t i = 0; i < s.size(); i++) {
    chars += s[i];
    off[i + 1] = (int32_t)chars.size();
  }
  auto col = std::make_unique<cudf::column>((cudf::size_type)s.size(), (int64_t)chars.size());
  CHECK(hipMemcpy(col->head(), off.data(), off.size() * 4, hipMemcpyHostToDevice));
  if (!chars.empty())
    CHECK(hipMemcpy(col->chars(), chars.data(), chars.size(), hipMemcpyHostToDevice));
  return col;
}

/* rows [row0, row0+rows) of a mask-free (INT64 key, INT32, STRING) table, or
 * of an (INT64 key, INT64) pair when `pair` */
static std::unique_ptr<cudf::table> plain_table(int64_t row0, int64_t rows, bool left, bool pair,
                                                int64_t distinct)
{
  std::vector<int64_t> key((size_t)rows), p64((size_t)rows);
  std::vector<int32_t> p32((size_t)rows);
  std::vector<std::string> ps((size_t)rows);
  for (int64_t t = 0; t < rows; t++) {
    const uint64_t g = (uint64_t)(row0 + t) + (left ? 0ull : 1000003ull);
    key[(size_t)t] = (int64_t)(dj_mix64(g) % (uint64_t)distinct);
    p64[(size_t)t] = (int64_t)g * 3;
    p32[(size_t)t] = (int32_t)(g * 7);
    ps[(size_t)t] = str_of(g);
  }
  std::vector<std::unique_ptr<cudf::column>> cols;
  cols.push_back(device_fixed(cudf::type_id::INT64, key.data(), rows, 8));
  if (pair) {
    cols.push_back(device_fixed(cudf::type_id::INT64, p64.data(), rows, 8));
  } else {
    cols.push_back(device_fixed(cudf::type_id::INT32, p32.data(), rows, 4));
    cols.push_back(device_strings(ps));
  }
  return std::make_unique<cudf::table>(std::move(cols));
}

static void count_mask_free(int G, int64_t R)
{
  const int64_t distinct = std::max<int64_t>(4, G * R / 3);
  Mailbox mb;
  std::atomic<long long> out_rows{0};
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    for (int pair = 0; pair < 2; pair++) {
      auto left = plain_table(r * R, R, true, pair != 0, distinct);
      auto right = plain_table(r * R, R, false, pair != 0, distinct);
      auto lo = generate_compression_options_distributed(left->view(), false);
      auto ro = generate_compression_options_distributed(right->view(), false);
      auto sh = shuffle_on(left->view(), {0}, comm, lo, cudf::hash_id::HASH_MURMUR3, 12345678u);
      auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, 2,
                                        false, nullptr, G);
      out_rows += sh->num_rows() + res->num_rows();
    }
  });
  printf("COUNTS G=%d R=%lld sends=%lld recvs=%lld send_bytes=%lld recv_bytes=%lld rows=%lld\n",
         G, (long long)R, mb.sends.load(), mb.recvs.load(), mb.send_bytes.load(),
         mb.recv_bytes.load(), out_rows.load());
}

#ifndef NULL_LOOPBACK_COUNTS_ONLY

/* ---------------- host tables with validity ---------------- */

struct HCol {
  cudf::type_id type;
  std::vector<int64_t> v;      // fixed-width values (garbage under a null)
  std::vector<std::string> s;  // STRING values (garbage under a null)
  std::vector<uint8_t> valid;
  bool mask;  // carries a mask on the device
};
using HTable = std::vector<HCol>;

static int width_of(cudf::type_id t) { return cudf::size_of(cudf::data_type(t)); }

static uint64_t fold(const std::string& s)
{
  uint64_t h = 1469598103934665603ull ^ s.size();
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

static uint64_t cell_hash(const HCol& c, size_t i)
{
  if (!c.valid[i]) return 0x6e756c6cull;
  return c.type == cudf::type_id::STRING ? fold(c.s[i]) : dj_mix64((uint64_t)c.v[i]);
}

/* hash of row i over columns [c0, c1): values and validity */
static uint64_t row_hash(const HTable& t, size_t c0, size_t c1, size_t i)
{
  uint64_t h = 0x12345;
  for (size_t c = c0; c < c1; c++) h = dj_mix64(h ^ cell_hash(t[c], i)) + (c - c0);
  return h;
}

static size_t rows_of(const HTable& t)
{
  return t.empty() ? 0 : t[0].valid.size();
}

static std::unique_ptr<cudf::table> to_device(const HTable& t)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (const HCol& c : t) {
    const size_t n = c.valid.size();
    std::unique_ptr<cudf::column> col;
    if (c.type == cudf::type_id::STRING) {
      col = device_strings(c.s);
    } else {
      const int w = width_of(c.type);
      std::vector<uint8_t> raw(n * (size_t)w);
      for (size_t i = 0; i < n; i++) memcpy(&raw[i * (size_t)w], &c.v[i], (size_t)w);  // LE
      col = device_fixed(c.type, raw.data(), (int64_t)n, w);
    }
    if (c.mask) {
      /* bits past the last row are unspecified: set them, nothing may care */
      std::vector<uint32_t> words((n + 31) / 32 + 1, 0xFFFFFFFFu);
      int nulls = 0;
      for (size_t i = 0; i < n; i++)
        if (!c.valid[i]) {
          words[i / 32] &= ~(1u << (i % 32));
          nulls++;
        }
      cudf::bitmask_type* m = col->allocate_null_mask();
      CHECK(hipMemcpy(m, words.data(), ((n + 31) / 32) * 4, hipMemcpyHostToDevice));
      col->set_null_count(nulls);
    }
    cols.push_back(std::move(col));
  }
  return std::make_unique<cudf::table>(std::move(cols));
}

static HTable from_device(const cudf::table& t)
{
  HTable out;
  const size_t n = (size_t)t.num_rows();
  for (cudf::size_type ci = 0; ci < t.num_columns(); ci++) {
    const cudf::column& col = t.get_column(ci);
    HCol c;
    c.type = col.type().id();
    c.mask = col.nullable();
    c.valid.assign(n, 1);
    if (c.mask) {
      std::vector<uint32_t> words((n + 31) / 32);
      if (n) CHECK(hipMemcpy(words.data(), col.null_mask(), words.size() * 4, hipMemcpyDeviceToHost));
      int nulls = 0;
      for (size_t i = 0; i < n; i++) {
        c.valid[i] = (words[i / 32] >> (i % 32)) & 1u;
        nulls += !c.valid[i];
      }
      if (col.null_count() != nulls)
        FAIL("column %d: null_count %d, mask has %d nulls", ci, col.null_count(), nulls);
    } else if (col.null_count() != 0) {
      FAIL("column %d: null_count %d without a mask", ci, col.null_count());
    }
    if (c.type == cudf::type_id::STRING) {
      std::vector<int32_t> off(n + 1);
      CHECK(hipMemcpy(off.data(), col.head(), (n + 1) * 4, hipMemcpyDeviceToHost));
      std::string ch((size_t)col.chars_size(), '\0');
      if (col.chars_size())
        CHECK(hipMemcpy(&ch[0], col.chars(), (size_t)col.chars_size(), hipMemcpyDeviceToHost));
      c.s.resize(n);
      for (size_t i = 0; i < n; i++)
        c.s[i] = ch.substr((size_t)off[i], (size_t)(off[i + 1] - off[i]));
    } else {
      const int w = width_of(c.type);
      std::vector<uint8_t> raw(n * (size_t)w);
      if (n) CHECK(hipMemcpy(raw.data(), col.head(), raw.size(), hipMemcpyDeviceToHost));
      c.v.assign(n, 0);
      for (size_t i = 0; i < n; i++) {
        int64_t v = 0;
        memcpy(&v, &raw[i * (size_t)w], (size_t)w);
        if (w < 8) v = (v << (64 - 8 * w)) >> (64 - 8 * w);  // sign-extend
        c.v[i] = v;
      }
    }
    out.push_back(std::move(c));
  }
  return out;
}

/* rows [row0, row0+rows) of a global table:
 *   left : key INT64, pay INT32, str STRING
 *   right: key INT64, pay INT64, pay2 INT16
 * every column nullable; keys only when null_keys. The value under a null key
 * is key id 1 or -1: both would match valid keys if they were compared. */
static HTable host_table(int64_t row0, int64_t rows, bool left, bool null_keys, int64_t distinct,
                         int key_null_every)
{
  HTable t(3);
  t[0].type = cudf::type_id::INT64;
  t[1].type = left ? cudf::type_id::INT32 : cudf::type_id::INT64;
  t[2].type = left ? cudf::type_id::STRING : cudf::type_id::INT16;
  for (auto& c : t) c.mask = true;
  t[0].mask = null_keys;
  for (int64_t r = 0; r < rows; r++) {
    const uint64_t g = (uint64_t)(row0 + r) + (left ? 0ull : 1000003ull);
    const bool knull = null_keys && dj_mix64(g ^ 0xabcdef) % (uint64_t)key_null_every == 0;
    int64_t key = (int64_t)(dj_mix64(g) % (uint64_t)distinct);
    if (dj_mix64(g) % 11 == 0) key = -1;  // the engine's sentinel, as a valid key
    if (knull) key = (g & 1) ? 1 : -1;
    t[0].v.push_back(key);
    t[0].valid.push_back(!knull);
    t[1].v.push_back(left ? (int64_t)(int32_t)(g * 7) : (int64_t)g * 3);
    t[1].valid.push_back(dj_mix64(g ^ 0x1111) % 4 != 0);
    if (left) {
      t[2].s.push_back(str_of(g));
    } else {
      t[2].v.push_back((int64_t)(int16_t)(g * 5));
    }
    t[2].valid.push_back(dj_mix64(g ^ 0x2222) % 3 != 0);
  }
  return t;
}

static std::string key_code(const HTable& t, size_t i)
{
  if (!t[0].valid[i]) return "n";
  return "v" + std::to_string(t[0].v[i]);
}

/* host inner join on column 0, null == null: (rows, order-insensitive sum) */
static void host_join(const HTable& l, const HTable& r, long long* rows, uint64_t* sum)
{
  std::map<std::string, std::vector<size_t>> idx;
  for (size_t i = 0; i < rows_of(l); i++) idx[key_code(l, i)].push_back(i);
  long long n = 0;
  uint64_t s = 0;
  for (size_t j = 0; j < rows_of(r); j++) {
    auto it = idx.find(key_code(r, j));
    if (it == idx.end()) continue;
    const uint64_t rh = row_hash(r, 0, r.size(), j);
    for (size_t i : it->second) {
      s += dj_mix64(row_hash(l, 0, l.size(), i) ^ dj_mix64(rh));
      n++;
    }
  }
  *rows = n;
  *sum = s;
}

static void join_output_sum(const HTable& out, size_t nl, long long* rows, uint64_t* sum)
{
  uint64_t s = 0;
  for (size_t i = 0; i < rows_of(out); i++) {
    if (key_code(out, i) != (out[nl].valid[i] ? "v" + std::to_string(out[nl].v[i]) : "n"))
      FAIL("JOIN ROW WITH UNEQUAL KEYS");
    s += dj_mix64(row_hash(out, 0, nl, i) ^ dj_mix64(row_hash(out, nl, out.size(), i)));
  }
  *rows = (long long)rows_of(out);
  *sum = s;
}

/* the rank that passes its column 1 without a mask (all rows valid there) */
constexpr int kMasklessRank = 1;

static HTable rank_table(int r, int64_t R, bool left, bool null_keys, int64_t distinct, int every)
{
  HTable t = host_table(r * R, R, left, null_keys, distinct, every);
  if (!left && r == kMasklessRank) {
    t[1].mask = false;
    t[1].valid.assign(t[1].valid.size(), 1);
  }
  return t;
}

static HTable global_table(int G, int64_t R, bool left, bool null_keys, int64_t distinct, int every)
{
  HTable all;
  for (int r = 0; r < G; r++) {
    HTable t = rank_table(r, R, left, null_keys, distinct, every);
    if (all.empty()) {
      all = t;
      continue;
    }
    for (size_t c = 0; c < t.size(); c++) {
      all[c].v.insert(all[c].v.end(), t[c].v.begin(), t[c].v.end());
      all[c].s.insert(all[c].s.end(), t[c].s.begin(), t[c].s.end());
      all[c].valid.insert(all[c].valid.end(), t[c].valid.begin(), t[c].valid.end());
    }
  }
  return all;
}

static void check_join(int G, int64_t R, bool null_keys, int od)
{
  const int64_t distinct = std::max<int64_t>(4, G * R / 3);
  const int every = G * R > 100 ? 16 : 3;
  long long want_rows = 0, got_rows = 0;
  uint64_t want_sum = 0, got_sum = 0;
  host_join(global_table(G, R, true, null_keys, distinct, every),
            global_table(G, R, false, null_keys, distinct, every), &want_rows, &want_sum);
  Mailbox mb;
  std::mutex m;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto left = to_device(rank_table(r, R, true, null_keys, distinct, every));
    auto right = to_device(rank_table(r, R, false, null_keys, distinct, every));
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, od,
                                      false, nullptr, G);
    if (res->num_columns() != 6) FAIL("JOIN OUTPUT SCHEMA WRONG");
    for (int c = 0; c < 6; c++) {
      const bool want_mask = (c != 0 && c != 3) || null_keys;
      if (res->get_column(c).nullable() != want_mask)
        FAIL("rank %d: output column %d nullable=%d, expected %d", r, c,
             (int)res->get_column(c).nullable(), (int)want_mask);
    }
    long long rows = 0;
    uint64_t sum = 0;
    join_output_sum(from_device(*res), 3, &rows, &sum);
    std::lock_guard<std::mutex> g(m);
    got_rows += rows;
    got_sum += sum;
  });
  printf("join G=%d R=%lld null_keys=%d od=%d: host rows=%lld sum=%llx; got rows=%lld sum=%llx\n",
         G, (long long)R, (int)null_keys, od, want_rows, (unsigned long long)want_sum, got_rows,
         (unsigned long long)got_sum);
  if (want_rows != got_rows || want_sum != got_sum) FAIL("NULL LOOPBACK JOIN MISMATCH");
}

static void check_shuffle(int G, int64_t R)
{
  const int64_t distinct = std::max<int64_t>(4, G * R / 3);
  const int every = G * R > 100 ? 16 : 3;
  const HTable all = global_table(G, R, false, true, distinct, every);
  uint64_t want_sum = 0, got_sum = 0;
  for (size_t i = 0; i < rows_of(all); i++) want_sum += dj_mix64(row_hash(all, 0, 3, i));
  Mailbox mb;
  std::mutex m;
  std::map<std::string, int> owner;
  long long got_rows = 0;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto t = to_device(rank_table(r, R, false, true, distinct, every));
    auto opts = generate_compression_options_distributed(t->view(), false);
    auto sh = shuffle_on(t->view(), {0}, comm, opts, cudf::hash_id::HASH_MURMUR3, 12345678u);
    for (int c = 0; c < 3; c++)
      if (!sh->get_column(c).nullable()) FAIL("rank %d: shuffled column %d lost its mask", r, c);
    HTable h = from_device(*sh);
    std::lock_guard<std::mutex> g(m);
    for (size_t i = 0; i < rows_of(h); i++) {
      got_sum += dj_mix64(row_hash(h, 0, 3, i));
      got_rows++;
      const std::string k = key_code(h, i);
      if (k == "n" && r != (int)(0xFFFFFFFFu % (unsigned)G))
        FAIL("NULL KEY ROW ON RANK %d, expected %u", r, 0xFFFFFFFFu % (unsigned)G);
      auto it = owner.emplace(k, r).first;
      if (it->second != r) FAIL("KEY ON TWO RANKS (%d and %d)", it->second, r);
    }
  });
  printf("shuffle G=%d R=%lld: rows=%lld sum=%llx (want %zu, %llx)\n", G, (long long)R, got_rows,
         (unsigned long long)got_sum, rows_of(all), (unsigned long long)want_sum);
  if (got_rows != (long long)rows_of(all) || got_sum != want_sum)
    FAIL("NULL LOOPBACK SHUFFLE MISMATCH");
}

/* the entry points that do not carry masks say so */
static void check_refusals()
{
  Mailbox mb;
  LoopbackComm comm(0, 1, &mb);
  auto t = to_device(host_table(0, 8, false, true, 4, 3));
  int refused = 0;
  try {
    distribute_table(t->view(), &comm);
  } catch (std::runtime_error const&) {
    refused++;
  }
  try {
    collect_tables(t->view(), &comm);
  } catch (std::runtime_error const&) {
    refused++;
  }
  try {
    std::vector<AllToAllCommBuffer> bufs;
    append_to_all_to_all_comm_buffers(t->view(), t->mutable_view(), {0, 8}, {0, 8}, bufs,
                                      generate_none_compression_options(t->view()));
  } catch (std::runtime_error const&) {
    refused++;
  }
  if (refused != 3 || mb.sends.load() != 0) FAIL("NULLABLE TABLE NOT REFUSED (%d of 3)", refused);
  printf("refusals OK\n");
}

#endif /* NULL_LOOPBACK_COUNTS_ONLY */

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int64_t R = argc > 2 ? atoll(argv[2]) : 5;
  if (G < 2 || G > 16 || R < 1) FAIL("usage: null_loopback G(2..16) rows_per_rank");
  CHECK(hipSetDevice(0));
  count_mask_free(G, R);
#ifndef NULL_LOOPBACK_COUNTS_ONLY
  check_refusals();
  check_shuffle(G, R);
  check_join(G, R, /*null_keys=*/true, /*od=*/1);
  check_join(G, R, /*null_keys=*/false, /*od=*/2);
  printf("NULL LOOPBACK OK\n");
#endif
  return 0;
}
