/*
 * joinkinds_loopback.cpp — left / left semi / left anti joins across G ranks
 * on ONE GPU. Ranks run as host threads over the counting loopback
 * Communicator of null_loopback.cpp.
 *
 * usage: joinkinds_loopback G rows_per_rank
 *
 * Checks (global tables of G * rows_per_rank rows, a formula of the row):
 *   1. each of LEFT, LEFT_SEMI, LEFT_ANTI against a host join of the global
 *      tables: row count and an order-insensitive checksum over every value
 *      and validity bit —
 *        a. on a nullable key: null-key rows all meet on one rank; run once
 *           with null keys on both sides and (LEFT, ANTI) once with none on
 *           the right, where every null left key appears exactly once;
 *        b. on a non-nullable key, where one rank passes a left payload
 *           column WITHOUT a mask: the output column still has a mask on
 *           every rank;
 *      a LEFT result masks every right-hand column on every rank;
 *   2. the same semi join with the right table as keys only and with three
 *      wide payload columns behind the key: the Communicator sees identical
 *      send and receive bytes — right-hand payloads stay home;
 *   3. (G = 8) one LEFT join with nvlink_domain_size 4, i.e. through the
 *      inter-domain stage.
 *
 * Build/run: tests/test_gpu_join_kinds_loopback.py.
 */
#include "communicator.hpp"
#include "compression.hpp"
#include "distributed_join.hpp"

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

static std::string str_of(uint64_t id)
{
  const int len = (int)(id % 9);
  std::string s((size_t)len, 'a');
  for (int k = 0; k < len; k++) s[(size_t)k] = (char)('a' + dj_mix64(id * 16 + (uint64_t)k) % 26);
  return s;
}

static uint64_t fold(const std::string& s)
{
  uint64_t h = 1469598103934665603ull ^ s.size();
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

constexpr uint64_t kNullCell = 0x6e756c6cull;

static uint64_t cell_hash(const HCol& c, size_t i)
{
  if (!c.valid[i]) return kNullCell;
  return c.type == cudf::type_id::STRING ? fold(c.s[i]) : dj_mix64((uint64_t)c.v[i]);
}

/* hash of row i over columns [c0, c1): values and validity */
static uint64_t row_hash(const HTable& t, size_t c0, size_t c1, size_t i)
{
  uint64_t h = 0x12345;
  for (size_t c = c0; c < c1; c++) h = dj_mix64(h ^ cell_hash(t[c], i)) + (c - c0);
  return h;
}

/* row_hash of a row of ncols null cells: the right side of an unmatched row */
static uint64_t null_row_hash(size_t ncols)
{
  uint64_t h = 0x12345;
  for (size_t c = 0; c < ncols; c++) h = dj_mix64(h ^ kNullCell) + c;
  return h;
}

static size_t rows_of(const HTable& t) { return t.empty() ? 0 : t[0].valid.size(); }

static std::unique_ptr<cudf::table> to_device(const HTable& t)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (const HCol& c : t) {
    const size_t n = c.valid.size();
    std::unique_ptr<cudf::column> col;
    if (c.type == cudf::type_id::STRING) {
      std::vector<int32_t> off(n + 1, 0);
      std::string chars;
      for (size_t i = 0; i < n; i++) {
        chars += c.s[i];
        off[i + 1] = (int32_t)chars.size();
      }
      col = std::make_unique<cudf::column>((cudf::size_type)n, (int64_t)chars.size());
      CHECK(hipMemcpy(col->head(), off.data(), off.size() * 4, hipMemcpyHostToDevice));
      if (!chars.empty())
        CHECK(hipMemcpy(col->chars(), chars.data(), chars.size(), hipMemcpyHostToDevice));
    } else {
      const int w = width_of(c.type);
      std::vector<uint8_t> raw(n * (size_t)w);
      for (size_t i = 0; i < n; i++) memcpy(&raw[i * (size_t)w], &c.v[i], (size_t)w);  // LE
      col = std::make_unique<cudf::column>(cudf::data_type(c.type), (cudf::size_type)n);
      if (n) CHECK(hipMemcpy(col->head(), raw.data(), raw.size(), hipMemcpyHostToDevice));
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
 *   right: key INT64, pay INT64, pay2 INT16 (+ two more INT64 when wide;
 *          the key alone when keys_only)
 * Left keys draw from `distinct` values, right keys from two thirds of them,
 * so about a third of the left keys have no partner. Payloads are nullable;
 * keys only when null_keys. The value under a null key is key id 1 or -1:
 * both would match valid keys if they were compared. */
enum RightShape { kRightPlain, kRightKeysOnly, kRightWide };

static HTable host_table(int64_t row0, int64_t rows, bool left, bool null_keys, int64_t distinct,
                         int key_null_every, RightShape shape = kRightPlain)
{
  HTable t(3);
  t[0].type = cudf::type_id::INT64;
  t[1].type = left ? cudf::type_id::INT32 : cudf::type_id::INT64;
  t[2].type = left ? cudf::type_id::STRING : cudf::type_id::INT16;
  for (auto& c : t) c.mask = true;
  t[0].mask = null_keys;
  const uint64_t range = left ? (uint64_t)distinct : (uint64_t)std::max<int64_t>(2, distinct * 2 / 3);
  for (int64_t r = 0; r < rows; r++) {
    const uint64_t g = (uint64_t)(row0 + r) + (left ? 0ull : 1000003ull);
    const bool knull = null_keys && dj_mix64(g ^ 0xabcdef) % (uint64_t)key_null_every == 0;
    int64_t key = (int64_t)(dj_mix64(g) % range);
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
  if (!left && shape == kRightKeysOnly) t.resize(1);
  if (!left && shape == kRightWide) {  // three 8-byte payloads behind the key
    t[2].type = cudf::type_id::INT64;
    HCol c = t[1];
    for (auto& x : c.v) x = x * 5;
    t.push_back(c);
  }
  return t;
}

static std::string key_code(const HTable& t, size_t i)
{
  if (!t[0].valid[i]) return "n";
  return "v" + std::to_string(t[0].v[i]);
}

/* host join of `kind` on column 0, null == null: (rows, order-insensitive sum) */
static void host_join(join_kind kind, const HTable& l, const HTable& r, long long* rows,
                      uint64_t* sum)
{
  std::map<std::string, std::vector<size_t>> idx;
  for (size_t j = 0; j < rows_of(r); j++) idx[key_code(r, j)].push_back(j);
  long long n = 0;
  uint64_t s = 0;
  const uint64_t pad = null_row_hash(r.size());
  for (size_t i = 0; i < rows_of(l); i++) {
    auto it = idx.find(key_code(l, i));
    const bool hit = it != idx.end();
    const uint64_t lh = row_hash(l, 0, l.size(), i);
    if (kind == join_kind::LEFT) {
      if (!hit) {
        s += dj_mix64(lh ^ dj_mix64(pad));
        n++;
        continue;
      }
      for (size_t j : it->second) {
        s += dj_mix64(lh ^ dj_mix64(row_hash(r, 0, r.size(), j)));
        n++;
      }
    } else if (hit == (kind == join_kind::LEFT_SEMI)) {
      s += dj_mix64(lh);
      n++;
    }
  }
  *rows = n;
  *sum = s;
}

static void output_sum(join_kind kind, const HTable& out, size_t nl, long long* rows,
                       uint64_t* sum)
{
  uint64_t s = 0;
  for (size_t i = 0; i < rows_of(out); i++) {
    const uint64_t lh = row_hash(out, 0, nl, i);
    s += kind == join_kind::LEFT ? dj_mix64(lh ^ dj_mix64(row_hash(out, nl, out.size(), i)))
                                 : dj_mix64(lh);
  }
  *rows = (long long)rows_of(out);
  *sum = s;
}

/* the rank that passes its LEFT column 1 without a mask (all rows valid there) */
constexpr int kMasklessRank = 1;

/* right_nulls = false: the right key keeps its mask but marks no row null
 * (the values that were under its nulls, 1 and -1, become ordinary keys), so
 * that a null left key has no partner anywhere */
static HTable rank_table(int r, int64_t R, bool left, bool null_keys, int64_t distinct, int every,
                         bool maskless_rank, RightShape shape = kRightPlain,
                         bool right_nulls = true)
{
  HTable t = host_table(r * R, R, left, null_keys, distinct, every, shape);
  if (!left && !right_nulls) t[0].valid.assign(t[0].valid.size(), 1);
  if (left && maskless_rank && r == kMasklessRank) {
    t[1].mask = false;
    t[1].valid.assign(t[1].valid.size(), 1);
  }
  return t;
}

static HTable global_table(int G, int64_t R, bool left, bool null_keys, int64_t distinct,
                           int every, bool maskless_rank, RightShape shape = kRightPlain,
                           bool right_nulls = true)
{
  HTable all;
  for (int r = 0; r < G; r++) {
    HTable t = rank_table(r, R, left, null_keys, distinct, every, maskless_rank, shape,
                          right_nulls);
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

static const char* kind_name(join_kind k)
{
  return k == join_kind::LEFT ? "left" : k == join_kind::LEFT_SEMI ? "semi" : "anti";
}

struct RunResult {
  long long rows, send_bytes, recv_bytes;
  uint64_t sum;
};

/* one distributed join of `kind` over G ranks, checked against the host join */
static RunResult check_join(join_kind kind, int G, int64_t R, bool null_keys, int domain,
                            RightShape shape = kRightPlain, bool right_nulls = true)
{
  const int64_t distinct = std::max<int64_t>(4, G * R / 3);
  const int every = G * R > 100 ? 16 : 3;
  const bool maskless = !null_keys;
  long long want_rows = 0, got_rows = 0;
  uint64_t want_sum = 0, got_sum = 0;
  host_join(kind, global_table(G, R, true, null_keys, distinct, every, maskless),
            global_table(G, R, false, null_keys, distinct, every, maskless, shape, right_nulls),
            &want_rows, &want_sum);
  Mailbox mb;
  std::mutex m;
  run_ranks(G, &mb, [&](int r, Communicator* comm) {
    auto left = to_device(rank_table(r, R, true, null_keys, distinct, every, maskless));
    auto right = to_device(
      rank_table(r, R, false, null_keys, distinct, every, maskless, shape, right_nulls));
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    std::unique_ptr<cudf::table> res;
    if (kind == join_kind::LEFT)
      res = distributed_left_join(left->view(), right->view(), {0}, {0}, comm, lo, ro, 2, false,
                                  nullptr, domain);
    else
      res = distributed_join(kind, left->view(), right->view(), {0}, {0}, comm, lo, ro, 1, false,
                             nullptr, domain);
    const int nl = left->num_columns();
    const int want_cols = nl + (kind == join_kind::LEFT ? right->num_columns() : 0);
    if (res->num_columns() != want_cols) FAIL("JOIN OUTPUT SCHEMA WRONG");
    for (int c = 0; c < want_cols; c++) {
      /* left side: a mask where any rank passed one; right side of LEFT: always */
      const bool want_mask = c >= nl || c != 0 || null_keys;
      if (res->get_column(c).nullable() != want_mask)
        FAIL("rank %d: output column %d nullable=%d, expected %d", r, c,
             (int)res->get_column(c).nullable(), (int)want_mask);
    }
    long long rows = 0;
    uint64_t sum = 0;
    output_sum(kind, from_device(*res), (size_t)nl, &rows, &sum);
    std::lock_guard<std::mutex> g(m);
    got_rows += rows;
    got_sum += sum;
  });
  printf("%s G=%d R=%lld null_keys=%d right_nulls=%d domain=%d shape=%d: host rows=%lld sum=%llx; got rows=%lld "
         "sum=%llx; send_bytes=%lld recv_bytes=%lld\n",
         kind_name(kind), G, (long long)R, (int)null_keys, (int)right_nulls, domain, (int)shape,
         want_rows,
         (unsigned long long)want_sum, got_rows, (unsigned long long)got_sum,
         mb.send_bytes.load(), mb.recv_bytes.load());
  if (want_rows != got_rows || want_sum != got_sum) FAIL("JOIN KINDS LOOPBACK MISMATCH");
  if (want_rows == 0) FAIL("JOIN KINDS LOOPBACK: empty reference result checks nothing");
  return RunResult{got_rows, mb.send_bytes.load(), mb.recv_bytes.load(), got_sum};
}

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int64_t R = argc > 2 ? atoll(argv[2]) : 1000;
  if (G < 2 || G > 16 || R < 1) FAIL("usage: joinkinds_loopback G(2..16) rows_per_rank");
  CHECK(hipSetDevice(0));
  for (join_kind kind : {join_kind::LEFT, join_kind::LEFT_SEMI, join_kind::LEFT_ANTI}) {
    check_join(kind, G, R, /*null_keys=*/true, /*domain=*/G);
    check_join(kind, G, R, /*null_keys=*/false, /*domain=*/G);
  }
  /* null left keys without a partner: each appears once, padded (LEFT) or
   * kept (ANTI), although all of them meet on one rank */
  check_join(join_kind::LEFT, G, R, true, G, kRightPlain, /*right_nulls=*/false);
  check_join(join_kind::LEFT_ANTI, G, R, true, G, kRightPlain, /*right_nulls=*/false);
  /* payloads stay home: the wire sees the same bytes whatever rides behind
   * the right table's key */
  const RunResult keys = check_join(join_kind::LEFT_SEMI, G, R, true, G, kRightKeysOnly);
  const RunResult wide = check_join(join_kind::LEFT_SEMI, G, R, true, G, kRightWide);
  if (keys.send_bytes != wide.send_bytes || keys.recv_bytes != wide.recv_bytes)
    FAIL("SEMI JOIN SHIPPED RIGHT-HAND PAYLOAD BYTES (%lld/%lld vs %lld/%lld)", wide.send_bytes,
         wide.recv_bytes, keys.send_bytes, keys.recv_bytes);
  if (keys.rows != wide.rows || keys.sum != wide.sum) FAIL("SEMI JOIN DEPENDS ON RIGHT PAYLOADS");
  if (keys.send_bytes == 0) FAIL("SEMI JOIN SENT NOTHING");
  if (G == 8) check_join(join_kind::LEFT, G, R, true, /*domain=*/4);
  printf("JOIN KINDS LOOPBACK OK\n");
  return 0;
}
