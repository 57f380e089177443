/*
 * lds_join_prefetch_check.cpp — lds_join_kernel's row prefetch, through
 * dj::lds_join and dj::lds_join_slack on bucket tables laid out by hand.
 *
 * The kernel loads each lane's first build row and first probe row of a
 * bucket into registers before it clears the table, under the predicate
 * lane < length of that side; rows past the block size come from the strided
 * loops; the rows of a bucket that is then skipped (empty side, skew-routed)
 * are dropped. What can go wrong is a row past a bucket's length (in another
 * bucket's segment, or past the buffer's end), a length or offset read past B,
 * a stale row kept over a skipped bucket, and the first row and the strided
 * rows of a long bucket overlapping or leaving a gap. The cases also cover
 * what a prefetch of the NEXT bucket would have to get right (the next bucket
 * is b+1 inside a flush group, the first bucket of group bb/4 + grid_groups at
 * a group's end, none after the block's last group): that variant was built
 * and measured against these cases, and whoever tries it again has them. So
 * every populated bucket here draws its keys from ONE pool, in the same order,
 * with payloads of its own: a row taken from another bucket gives a pair with
 * a key that matches and a payload that does not.
 *
 * Reference, on the host, per bucket: a std::unordered_multimap join of that
 * bucket's build and probe rows (build rows with key -1 are skipped and set
 * the error word; buckets with both sides non-empty and more than
 * slots * 3 / 4 build rows are flagged and skipped). All checks are exact: the
 * counter, the sorted (out0..out3) tuples, the per-bucket flags, the
 * any-overflow word, the error word, and the fill pattern past the output.
 *
 * Every case runs with both table sizes and in both layouts. Nothing is
 * padded: the offset arrays hold B + 1 entries and the row buffers the rows
 * alone; the length arrays hold B entries and the slack buffers B * cap rows,
 * with cap the longest bucket of that side unless the case sets it — the rows
 * between a length and cap hold poison with keys of the bucket's other side.
 *
 * Cases (T = bucket_partition_shape().bucket_threads, cap = slots * 3 / 4,
 * G = lds_join_shape().grid_groups, groups of lds_join_shape().flush_group):
 *   block-size edges    (build, probe) rows of (T-1, T+1), (T, T-1), (T+1, T),
 *                       (min(2T+1, cap), 2T+1), (cap, cap+T+1), (1, 2T+1),
 *                       (T, 1), (cap, T)
 *   -1 sentinel         T+5 build rows with -1 at row 3 and at row T+2
 *   neighbours, group   populated -> X -> populated inside one group, X an
 *                       empty build side, an empty probe side, a skew-routed
 *                       bucket
 *   neighbours, trip    the same three X as the first and as the last bucket
 *                       of a group, the populated neighbour in the block's
 *                       other trip (group g and group g + G)
 *   three trips         block 4: groups 4 and 2G+4 populated, G+4 empty;
 *                       block 5: groups 5 and G+5 populated, and group 6 (what
 *                       a plain b+1 names after group 5) populated too; the
 *                       last bucket of B populated (B = 4 * (2G + 5))
 *   short slack         caps of 8 and 6 rows, lengths 0..cap, last bucket full
 *
 * usage: lds_join_prefetch_check [--inputs-only]
 *   --inputs-only: cases, reference and the structural checks on the cases
 *   (which trip a group falls in, which buckets are flagged); no GPU.
 * Build/run: tests/test_gpu_lds_join_prefetch.py.
 */
#include "bucket_model.hpp" /* kGuardRows, kPoison */
#include "check.hpp"

#include "dj_kernels.hpp"

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

struct Row {
  int64_t k, v;
};
static_assert(sizeof(Row) == sizeof(longlong2), "Row must lay out as longlong2");
using Tuple = std::array<int64_t, 4>;

struct Bucket {
  std::vector<Row> L, R;
};

struct Case {
  std::string name;
  int slots = 2048;
  std::vector<Bucket> bk;
  int64_t capL = 0, capR = 0;  // slack capacities; 0: the side's longest bucket
  int want_flagged = 0, want_error = 0;
};

static dj::LdsJoinShape g_shape;
static int g_T;
constexpr int64_t kFill = (int64_t)0xEEEEEEEEEEEEEEEEULL;

#define BAD_INPUTS(...)            \
  do {                             \
    printf("BAD TEST INPUTS: ");   \
    printf(__VA_ARGS__);           \
    printf("\n");                  \
    exit(2);                       \
  } while (0)

/* ------------------------------------------------------------ row makers */

static uint64_t g_rng = 777;
static int64_t g_pay_ctr = 0;
static std::vector<int64_t> g_pool, g_absent;

static int64_t lpay() { return 1000000000LL + g_pay_ctr++; }
static int64_t rpay() { return 2000000000LL + g_pay_ctr++; }
static int64_t poison_pay() { return 7000000000LL + g_pay_ctr++; }

static int row_cap(int slots) { return slots * 3 / 4; }

/* dj_mix64 is a bijection, so the keys are distinct from each other */
static void make_pools(size_t n)
{
  uint64_t ctr = 1;
  auto fresh = [&]() {
    for (;;) {
      const int64_t k = (int64_t)dj_mix64(ctr++ | (1ULL << 41));
      if (k != -1 && k != 0) return k;
    }
  };
  for (size_t i = 0; i < n; i++) g_pool.push_back(fresh());
  for (size_t i = 0; i < n; i++) g_absent.push_back(fresh());
}

static void shuffle(std::vector<Row>& v)
{
  for (size_t i = v.size(); i > 1; i--) {
    g_rng = dj_mix64(g_rng);
    std::swap(v[i - 1], v[(size_t)(g_rng % i)]);
  }
}

/* nL build rows on the pool's first nL keys; probe rows alternate between the
 * pool's keys (a match when the key is among the first nL) and absent keys */
static Bucket pool_bucket(int nL, int nR)
{
  if ((size_t)nL > g_pool.size() || (size_t)nR / 2 + 1 > g_pool.size())
    BAD_INPUTS("key pool too small for %d x %d", nL, nR);
  Bucket b;
  for (int i = 0; i < nL; i++) b.L.push_back({g_pool[(size_t)i], lpay()});
  for (int i = 0; i < nR; i++)
    b.R.push_back({i % 2 == 0 ? g_pool[(size_t)i / 2] : g_absent[(size_t)i / 2], rpay()});
  shuffle(b.L);
  shuffle(b.R);
  return b;
}

enum Kind { POP, EMPTY_BUILD, EMPTY_PROBE, SKEW };
/* populated buckets differ in size, so a neighbour's length on this bucket's
 * rows (or the other way round) reads past one of the two */
static Bucket make_kind(Kind kind, int slots, int salt)
{
  switch (kind) {
    case POP: return pool_bucket(20 + salt % 17, 30 + salt % 23);
    case EMPTY_BUILD: return pool_bucket(0, 25 + salt % 7);
    case EMPTY_PROBE: return pool_bucket(22 + salt % 5, 0);
    case SKEW: return pool_bucket(row_cap(slots) + 1, 40);
  }
  return {};
}

static void put_group(Case& c, int group, const Kind (&kinds)[4])
{
  for (int k = 0; k < 4; k++) {
    c.bk[(size_t)group * 4 + k] = make_kind(kinds[k], c.slots, group * 4 + k);
    c.want_flagged += kinds[k] == SKEW;
  }
}

/* ----------------------------------------------------------------- cases */

static Case edge_case(int slots)
{
  const int T = g_T, cap = row_cap(slots);
  Case c;
  c.name = "block-size edges";
  c.slots = slots;
  const int sizes[8][2] = {{T - 1, T + 1}, {T, T - 1}, {T + 1, T}, {std::min(2 * T + 1, cap), 2 * T + 1},
                           {cap, cap + T + 1}, {1, 2 * T + 1}, {T, 1}, {cap, T}};
  for (const auto& s : sizes) {
    if (s[0] > cap) BAD_INPUTS("edge build length %d over the cap %d", s[0], cap);
    c.bk.push_back(pool_bucket(s[0], s[1]));
  }
  return c;
}

static Case sentinel_case(int slots)
{
  const int T = g_T;
  if (T + 5 > row_cap(slots)) BAD_INPUTS("T + 5 build rows exceed the cap");
  Case c;
  c.name = "-1 among a build bucket's first T rows and in its tail";
  c.slots = slots;
  c.bk.resize(4);
  c.bk[0] = pool_bucket(40, 50);
  c.bk[1] = pool_bucket(T + 5, T + 9);
  c.bk[1].L[3].k = -1;
  c.bk[1].L[(size_t)T + 2].k = -1;
  c.bk[2] = pool_bucket(33, 44);
  c.bk[3] = pool_bucket(T + 5, 60);
  c.want_error = 1;
  return c;
}

static Case group_neighbours_case(int slots)
{
  Case c;
  c.name = "populated -> X -> populated inside one group";
  c.slots = slots;
  c.bk.resize(16);
  put_group(c, 0, {POP, EMPTY_BUILD, POP, POP});
  put_group(c, 1, {POP, EMPTY_PROBE, POP, POP});
  put_group(c, 2, {POP, SKEW, POP, POP});
  put_group(c, 3, {POP, POP, EMPTY_PROBE, EMPTY_BUILD});
  return c;
}

/* block i takes groups i and G + i: X is the first bucket of the second trip
 * (after the populated last bucket of the first) or the last bucket of the
 * first trip (before the populated first bucket of the second) */
static Case trip_neighbours_case(int slots)
{
  const int G = g_shape.grid_groups;
  Case c;
  c.name = "populated -> X -> populated across the block's trips";
  c.slots = slots;
  c.bk.resize((size_t)4 * (G + 6));
  const Kind xs[3] = {EMPTY_BUILD, EMPTY_PROBE, SKEW};
  for (int i = 0; i < 3; i++) {
    put_group(c, 2 * i, {POP, POP, POP, POP});
    put_group(c, G + 2 * i, {xs[i], POP, POP, POP});
    put_group(c, 2 * i + 1, {POP, POP, POP, xs[i]});
    put_group(c, G + 2 * i + 1, {POP, POP, POP, POP});
  }
  return c;
}

static Case three_trips_case(int slots)
{
  const int G = g_shape.grid_groups;
  Case c;
  c.name = "empty group between trips, second trip beside b+1, last bucket of B";
  c.slots = slots;
  c.bk.resize((size_t)4 * (2 * G + 5));
  put_group(c, 4, {POP, POP, POP, POP});
  /* group G + 4 stays empty */
  put_group(c, 2 * G + 4, {POP, EMPTY_BUILD, POP, POP});  // its last bucket is B - 1
  put_group(c, 5, {POP, POP, POP, POP});
  put_group(c, 6, {POP, POP, POP, POP});  // bucket 4 * 5 + 4: what b + 1 names
  put_group(c, G + 5, {POP, POP, POP, POP});
  return c;
}

static Case short_slack_case(int slots)
{
  Case c;
  c.name = "slack capacities of 8 and 6 rows, lengths 0..cap, last bucket full";
  c.slots = slots;
  c.capL = 8;
  c.capR = 6;
  c.bk.resize(24);
  for (int b = 0; b < 24; b++)
    c.bk[(size_t)b] = pool_bucket(b == 23 ? 8 : (b * 5 + 1) % 9, b == 23 ? 6 : (b * 3 + 2) % 7);
  return c;
}

/* --------------------------------------------------------------- reference */

struct Ref {
  std::vector<Tuple> rows;  // sorted
  std::vector<uint32_t> flags;
  int any = 0, error = 0;
};

static Ref reference(const Case& c)
{
  Ref ref;
  ref.flags.assign(c.bk.size(), 0);
  for (size_t b = 0; b < c.bk.size(); b++) {
    const Bucket& bu = c.bk[b];
    if (bu.L.empty() || bu.R.empty()) continue;
    if ((int64_t)bu.L.size() > row_cap(c.slots)) {
      ref.flags[b] = 1;
      ref.any = 1;
      continue;
    }
    std::unordered_multimap<int64_t, int64_t> tbl;
    tbl.reserve(bu.L.size());
    for (const Row& r : bu.L) {
      if (r.k == -1) {
        ref.error = 1;
        continue;
      }
      tbl.emplace(r.k, r.v);
    }
    for (const Row& r : bu.R) {
      if (r.k == -1) continue;  // the empty-slot value ends the walk at once
      auto range = tbl.equal_range(r.k);
      for (auto it = range.first; it != range.second; ++it)
        ref.rows.push_back({r.k, it->second, r.k, r.v});
    }
  }
  std::sort(ref.rows.begin(), ref.rows.end());
  return ref;
}

static int64_t side_cap(const Case& c, bool left)
{
  if (left ? c.capL : c.capR) return left ? c.capL : c.capR;
  size_t m = 1;
  for (const Bucket& bu : c.bk) m = std::max(m, left ? bu.L.size() : bu.R.size());
  return (int64_t)m;
}

/* what a case claims about itself, checked before anything runs */
static void check_inputs(const Case& c, const Ref& ref)
{
  const int KB = g_shape.flush_group, G = g_shape.grid_groups;
  const size_t B = c.bk.size();
  if (KB != 4) BAD_INPUTS("the cases are written for groups of 4");
  if (B % (size_t)KB) BAD_INPUTS("'%s': B = %zu is no multiple of the group", c.name.c_str(), B);
  int flagged = 0;
  for (uint32_t f : ref.flags) flagged += (int)f;
  if (flagged != c.want_flagged)
    BAD_INPUTS("'%s': %d buckets flagged, the case wants %d", c.name.c_str(), flagged,
               c.want_flagged);
  if (ref.error != c.want_error) BAD_INPUTS("'%s': error word %d", c.name.c_str(), ref.error);
  if (ref.rows.empty()) BAD_INPUTS("'%s': no matches at all", c.name.c_str());
  const int64_t capL = side_cap(c, true), capR = side_cap(c, false);
  for (const Bucket& bu : c.bk)
    if ((int64_t)bu.L.size() > capL || (int64_t)bu.R.size() > capR)
      BAD_INPUTS("'%s': a bucket exceeds its slack capacity", c.name.c_str());
  auto populated = [&](size_t b) { return !c.bk[b].L.empty() && !c.bk[b].R.empty(); };
  if (B > (size_t)KB * G) {
    /* some block must join buckets in two trips, and B - 1 closes a trip */
    bool two = false;
    for (size_t g = 0; g + G < B / KB && !two; g++) {
      bool a = false, b2 = false;
      for (int k = 0; k < KB; k++) a |= populated(g * KB + k), b2 |= populated((g + G) * KB + k);
      two = a && b2;
    }
    if (!two) BAD_INPUTS("'%s': no block joins buckets in two trips", c.name.c_str());
  }
}

/* ------------------------------------------------------------- GPU runs */

struct Dev {
  std::vector<void*> ptrs;
  template <class T>
  T* alloc(size_t n)
  {
    void* p = nullptr;
    CHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    ptrs.push_back(p);
    return (T*)p;
  }
  void release()
  {
    for (void* p : ptrs) CHECK(hipFree(p));
    ptrs.clear();
  }
};

static void print_tuple(const char* what, const Tuple& t)
{
  printf("  %s (%lld, %lld, %lld, %lld)\n", what, (long long)t[0], (long long)t[1],
         (long long)t[2], (long long)t[3]);
}

/* rows of one slack segment: the bucket's own, then poison up to the capacity
 * with keys of the bucket's other side */
static std::vector<Row> slack_segment(const std::vector<Row>& own, const std::vector<Row>& other,
                                      int64_t cap)
{
  std::vector<Row> seg(own);
  for (size_t i = own.size(); i < (size_t)cap; i++) {
    const std::vector<Row>& src = !other.empty() ? other : own;
    seg.push_back({src.empty() ? g_pool[i % g_pool.size()] : src[i % src.size()].k, poison_pay()});
  }
  return seg;
}

static void run_case(const Case& c, const Ref& ref, bool slack)
{
  char head[64];
  snprintf(head, sizeof head, " [slots=%d B=%zu] %s", c.slots, c.bk.size(),
           slack ? "slack" : "compact");
  const std::string label = c.name + head;
  const int B = (int)c.bk.size();
  Dev dev;
  Row *d_l, *d_r;
  int64_t* d_loff = nullptr;
  int64_t* d_roff = nullptr;
  uint32_t* d_llen = nullptr;
  uint32_t* d_rlen = nullptr;
  int64_t capL = 0, capR = 0;
  if (slack) {
    capL = side_cap(c, true);
    capR = side_cap(c, false);
    std::vector<uint32_t> llen((size_t)B), rlen((size_t)B);
    d_l = dev.alloc<Row>((size_t)B * capL);
    d_r = dev.alloc<Row>((size_t)B * capR);
    /* segments of the many empty buckets of a large B stay -1 rows: read as
     * build rows they set the error word */
    CHECK(hipMemset(d_l, 0xFF, (size_t)B * capL * sizeof(Row)));
    CHECK(hipMemset(d_r, 0xFF, (size_t)B * capR * sizeof(Row)));
    const bool dense = B <= 256;
    for (int b = 0; b < B; b++) {
      const Bucket& bu = c.bk[(size_t)b];
      llen[(size_t)b] = (uint32_t)bu.L.size();
      rlen[(size_t)b] = (uint32_t)bu.R.size();
      if (!dense && bu.L.empty() && bu.R.empty()) continue;
      const std::vector<Row> ls = slack_segment(bu.L, bu.R, capL);
      const std::vector<Row> rs = slack_segment(bu.R, bu.L, capR);
      CHECK(hipMemcpy(d_l + (int64_t)b * capL, ls.data(), ls.size() * sizeof(Row),
                      hipMemcpyHostToDevice));
      CHECK(hipMemcpy(d_r + (int64_t)b * capR, rs.data(), rs.size() * sizeof(Row),
                      hipMemcpyHostToDevice));
    }
    d_llen = dev.alloc<uint32_t>((size_t)B);
    d_rlen = dev.alloc<uint32_t>((size_t)B);
    CHECK(hipMemcpy(d_llen, llen.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_rlen, rlen.data(), (size_t)B * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<Row> hl, hr;
    std::vector<int64_t> loff((size_t)B + 1), roff((size_t)B + 1);
    for (int b = 0; b < B; b++) {
      const Bucket& bu = c.bk[(size_t)b];
      loff[(size_t)b] = (int64_t)hl.size();
      roff[(size_t)b] = (int64_t)hr.size();
      hl.insert(hl.end(), bu.L.begin(), bu.L.end());
      hr.insert(hr.end(), bu.R.begin(), bu.R.end());
    }
    loff[(size_t)B] = (int64_t)hl.size();
    roff[(size_t)B] = (int64_t)hr.size();
    d_l = dev.alloc<Row>(hl.size());
    d_r = dev.alloc<Row>(hr.size());
    d_loff = dev.alloc<int64_t>((size_t)B + 1);
    d_roff = dev.alloc<int64_t>((size_t)B + 1);
    CHECK(hipMemcpy(d_l, hl.data(), hl.size() * sizeof(Row), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_r, hr.data(), hr.size() * sizeof(Row), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_loff, loff.data(), ((size_t)B + 1) * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_roff, roff.data(), ((size_t)B + 1) * 8, hipMemcpyHostToDevice));
  }

  const int64_t total = (int64_t)ref.rows.size();
  const int64_t cap = total + 8;
  const size_t alloc = (size_t)(cap + kGuardRows);
  int64_t* d_col[4];
  for (int i = 0; i < 4; i++) {
    d_col[i] = dev.alloc<int64_t>(alloc);
    CHECK(hipMemset(d_col[i], kPoison, alloc * 8));
  }
  int64_t* d_counter = dev.alloc<int64_t>(1);
  uint32_t* d_flags = dev.alloc<uint32_t>((size_t)B);
  int* d_any = dev.alloc<int>(1);
  int* d_error = dev.alloc<int>(1);
  CHECK(hipMemset(d_counter, 0, 8));
  CHECK(hipMemset(d_flags, 0, (size_t)B * 4));
  CHECK(hipMemset(d_any, 0, 4));
  CHECK(hipMemset(d_error, 0, 4));

  if (slack)
    dj::lds_join_slack((const longlong2*)d_l, d_llen, capL, (const longlong2*)d_r, d_rlen, capR,
                       B, c.slots, d_col[0], d_col[1], d_col[2], d_col[3], cap, d_counter,
                       d_flags, d_any, d_error, nullptr);
  else
    dj::lds_join((const longlong2*)d_l, d_loff, (const longlong2*)d_r, d_roff, B, c.slots,
                 d_col[0], d_col[1], d_col[2], d_col[3], cap, d_counter, d_flags, d_any, d_error,
                 nullptr);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());

  int64_t counter = -1;
  int any = -1, error = -1;
  std::vector<uint32_t> flags((size_t)B);
  CHECK(hipMemcpy(&counter, d_counter, 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&any, d_any, 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&error, d_error, 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(flags.data(), d_flags, (size_t)B * 4, hipMemcpyDeviceToHost));
  std::vector<int64_t> col[4];
  for (int i = 0; i < 4; i++) {
    col[i].resize(alloc);
    CHECK(hipMemcpy(col[i].data(), d_col[i], alloc * 8, hipMemcpyDeviceToHost));
  }
  dev.release();

  const char* l = label.c_str();
  if (counter != total)
    FAIL("%s: FAILED\n  counter %lld, reference %lld", l, (long long)counter, (long long)total);
  for (size_t b = 0; b < flags.size(); b++)
    if (flags[b] != ref.flags[b])
      FAIL("%s: FAILED\n  overflow_flags[%zu] = %u, reference %u", l, b, flags[b], ref.flags[b]);
  if (any != ref.any) FAIL("%s: FAILED\n  any_overflow %d, reference %d", l, any, ref.any);
  if (error != ref.error) FAIL("%s: FAILED\n  error word %d, reference %d", l, error, ref.error);
  for (int i = 0; i < 4; i++)
    for (size_t r = (size_t)total; r < alloc; r++)
      if (col[i][r] != kFill)
        FAIL("%s: FAILED\n  out%d[%zu] overwritten (%lld) past %lld rows", l, i, r,
             (long long)col[i][r], (long long)total);
  std::vector<Tuple> got((size_t)total);
  for (size_t r = 0; r < got.size(); r++) got[r] = {col[0][r], col[1][r], col[2][r], col[3][r]};
  std::sort(got.begin(), got.end());
  for (size_t r = 0; r < got.size(); r++)
    if (got[r] != ref.rows[r]) {
      printf("%s: FAILED\n  sorted row %zu differs\n", l, r);
      print_tuple("got ", got[r]);
      print_tuple("want", ref.rows[r]);
      exit(1);
    }
  printf("%s: ok\n", l);
}

/* ---------------------------------------------------------------- main */

int main(int argc, char** argv)
{
  const bool inputs_only = argc > 1 && strcmp(argv[1], "--inputs-only") == 0;
  if (argc > 1 && !inputs_only) {
    printf("usage: lds_join_prefetch_check [--inputs-only]\n");
    return 2;
  }
  g_shape = dj::lds_join_shape();
  g_T = dj::bucket_partition_shape().bucket_threads;
  if (g_T + 5 > row_cap(2048) || g_T < 16)
    BAD_INPUTS("block size %d does not fit the cases", g_T);
  make_pools((size_t)row_cap(4096) + (size_t)g_T + 64);

  std::vector<Case> cases;
  for (int slots : {2048, 4096}) {
    cases.push_back(edge_case(slots));
    cases.push_back(sentinel_case(slots));
    cases.push_back(group_neighbours_case(slots));
    cases.push_back(trip_neighbours_case(slots));
    cases.push_back(three_trips_case(slots));
    cases.push_back(short_slack_case(slots));
  }
  /* every input check comes before the first launch */
  std::vector<Ref> refs;
  for (const Case& c : cases) {
    refs.push_back(reference(c));
    check_inputs(c, refs.back());
    if (inputs_only) {
      size_t nl = 0, nr = 0;
      for (const Bucket& b : c.bk) nl += b.L.size(), nr += b.R.size();
      printf("inputs %s [slots=%d B=%zu]: %zu x %zu rows, %zu matches, %d flagged, caps %lld/%lld\n",
             c.name.c_str(), c.slots, c.bk.size(), nl, nr, refs.back().rows.size(),
             c.want_flagged, (long long)side_cap(c, true), (long long)side_cap(c, false));
    }
  }
  {
    /* the three-trips case: its claims about single buckets */
    const int G = g_shape.grid_groups;
    for (const Case& c : cases) {
      if (c.bk.size() != (size_t)4 * (2 * G + 5)) continue;
      auto pop = [&](size_t b) { return !c.bk[b].L.empty() && !c.bk[b].R.empty(); };
      if (!pop(c.bk.size() - 1)) BAD_INPUTS("the last bucket of B is not populated");
      if (!pop(4 * 5 + 3) || !pop(4 * 6) || !pop((size_t)4 * (G + 5)))
        BAD_INPUTS("second trip: group 5's last, group 6's first or group G+5's first is empty");
      for (int k = 0; k < 4; k++)
        if (!c.bk[(size_t)4 * (G + 4) + k].L.empty() || !c.bk[(size_t)4 * (G + 4) + k].R.empty())
          BAD_INPUTS("group G+4 is not empty");
      if (!pop(4 * 4 + 3) || !pop((size_t)4 * (2 * G + 4)))
        BAD_INPUTS("the groups around the empty group are not populated");
    }
  }
  if (inputs_only) {
    printf("LDS JOIN PREFETCH INPUTS OK (%zu cases)\n", cases.size());
    return 0;
  }
  int runs = 0;
  for (size_t i = 0; i < cases.size(); i++) {
    run_case(cases[i], refs[i], false);
    run_case(cases[i], refs[i], true);
    runs += 2;
  }
  printf("LDS JOIN PREFETCH OK (%d runs)\n", runs);
  return 0;
}
