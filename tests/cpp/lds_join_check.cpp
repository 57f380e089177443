/*
 * lds_join_check.cpp — lds_join_kernel (the fused per-bucket LDS build + probe
 * with its staged output) called directly through dj::lds_join and
 * dj::lds_join_slack, on bucket tables laid out by hand. The kernel does not
 * care which keys share a bucket, so a bucket here is an arbitrary row set:
 * exactly cap build rows, exactly watermark - 1 matches, one home slot for a
 * whole bucket, a populated group in the grid's second trip.
 *
 * Reference, on the host, per bucket: a std::unordered_multimap join of that
 * bucket's build and probe rows. Build rows with key -1 are skipped (and set
 * the error word when their bucket is joined); buckets with both sides
 * non-empty and more than slots * 3 / 4 build rows are flagged and skipped.
 *
 * Checks per run, all exact: the counter, the sorted (out0..out3) tuples, the
 * per-bucket flags, the any-overflow word (0 or 1, bit 2 never) and the error
 * word. Every output column has 64 rows past `cap` holding a fill pattern;
 * they and every row past the counter must read back untouched. With `cap`
 * below the total the counter is still the full total and rows [0, cap) hold
 * no tuple more often than the reference does.
 *
 * Every case runs in the compact layout (loff/roff) and in the slack layout
 * (capL != capR, llen/rlen, one trailing group of zero-length buckets). In
 * the slack layout the rows between a bucket's length and its capacity hold
 * poison rows whose keys occur on the bucket's other side, so a read past the
 * length shows as extra matches (or, for untouched -1 filler, as the error
 * word).
 *
 * Cases (sizes from dj::lds_join_shape(), never from copies):
 *   build-length edge   1, cap-1, cap, cap+1 and 3*cap build rows; the flagged
 *                       buckets then go through join_table_slots, a 0xFF
 *                       memset, join_build_pairs, join_probe_pairs as the
 *                       product's fallback does, and the union is compared
 *   table reset         each bucket probes for the previous bucket's build
 *                       keys, within a group and into the block's next trip
 *   stage arithmetic    groups of four buckets by match count around the
 *                       watermark and the stage size (see stage_patterns),
 *                       each in the first, a middle and the last group
 *   output capacity     the stage table again with cap 0, cap below one
 *                       flush, and cap cutting through a flush and a spill
 *   wrap-around         a bucket of cap keys that all hash to slot slots-1
 *   duplicates, sentinel, extreme keys
 *   second trip         B = flush_group * (grid_groups + 2), populated in
 *                       both trips of one block, in the first only, in the
 *                       second only
 *
 * usage: lds_join_check [--inputs-only | --bad-b]
 *   --inputs-only: all host-side work (cases, reference, wrap-around key
 *   search, stage-pattern coverage by plain arithmetic on the match counts);
 *   touches no GPU.
 *   --bad-b: dj::lds_join with B = 6 and nothing allocated; DJ_CHECK_ERROR
 *   must end the process with status 1 before any launch.
 * Build/run: tests/test_gpu_lds_join.py.
 */
#include "bucket_model.hpp" /* kGuardRows, kPoison */
#include "check.hpp"

#include "dj_kernels.hpp"

#include <algorithm>
#include <array>
#include <cstdarg>
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

enum CapMode { CAP_FULL, CAP_ZERO, CAP_SMALL, CAP_MID };

struct Case {
  std::string name;
  int slots = 2048;
  std::vector<Bucket> bk;
  CapMode cap_mode = CAP_FULL;
  bool fallback = false;  // join the flagged buckets the way the product does
  /* stage cases: staged and spilled rows predicted from the match counts */
  int64_t pred_staged = -1, pred_spilled = -1;
};

static dj::LdsJoinShape g_shape;
constexpr int64_t kFill = (int64_t)0xEEEEEEEEEEEEEEEEULL;

[[noreturn]] static void bad_inputs(const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  printf("BAD TEST INPUTS: ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
  exit(2);
}

/* ------------------------------------------------------------ row makers */

static uint64_t g_key_ctr = 1, g_rng = 12345;
static int64_t g_pay_ctr = 0;

/* dj_mix64 is a bijection, so fresh keys are distinct from each other */
static int64_t fresh_key()
{
  for (;;) {
    const int64_t k = (int64_t)dj_mix64(g_key_ctr++ | (1ULL << 40));
    if (k != -1 && k != -2 && k != 0 && k != INT64_MIN && k != INT64_MAX) return k;
  }
}
/* payloads are distinct across both sides, so a swapped payload shows */
static int64_t lpay() { return 1000000000LL + g_pay_ctr++; }
static int64_t rpay() { return 2000000000LL + g_pay_ctr++; }
static int64_t poison_pay() { return 7000000000LL + g_pay_ctr++; }

static void shuffle(std::vector<Row>& v)
{
  for (size_t i = v.size(); i > 1; i--) {
    g_rng = dj_mix64(g_rng);
    std::swap(v[i - 1], v[(size_t)(g_rng % i)]);
  }
}

/* m matches on unique build keys, plus rows that match nothing */
static Bucket match_bucket(int m, int extra_build = 2, int extra_probe = 3)
{
  Bucket b;
  for (int i = 0; i < m; i++) {
    const int64_t k = fresh_key();
    b.L.push_back({k, lpay()});
    b.R.push_back({k, rpay()});
  }
  for (int i = 0; i < extra_build; i++) b.L.push_back({fresh_key(), lpay()});
  for (int i = 0; i < extra_probe; i++) b.R.push_back({fresh_key(), rpay()});
  shuffle(b.L);
  shuffle(b.R);
  return b;
}

/* nbuild unique build keys, every one of them probed, plus absent probes */
static Bucket full_bucket(int nbuild, int absent)
{
  return match_bucket(nbuild, 0, absent);
}

/* nk keys, each dup times on either side: nk * dup * dup matches */
static Bucket dup_bucket(int nk, int dup)
{
  Bucket b;
  for (int i = 0; i < nk; i++) {
    const int64_t k = fresh_key();
    for (int d = 0; d < dup; d++) {
      b.L.push_back({k, lpay()});
      b.R.push_back({k, rpay()});
    }
  }
  shuffle(b.L);
  shuffle(b.R);
  return b;
}

static int row_cap(int slots) { return slots * 3 / 4; }

/* ------------------------------------------------- stage-arithmetic table */

enum Kind { JOIN, DUP, EMPTY_BOTH, EMPTY_L, EMPTY_R, SKEW };
struct Slot {
  Kind kind;
  int m;  // JOIN: matches; DUP: keys (each 64 x 64)
};
struct Pattern {
  const char* name;
  Slot s[4];
};
constexpr int kDup = 64;

static int slot_matches(const Slot& s)
{
  return s.kind == JOIN ? s.m : s.kind == DUP ? s.m * kDup * kDup : 0;
}

static std::vector<Pattern> stage_patterns()
{
  const int S = g_shape.stage_rows, W = g_shape.watermark;
  return {
    {"carry W-1 drained through an empty last slot",
     {{JOIN, W - 1}, {JOIN, 0}, {JOIN, 0}, {EMPTY_BOTH, 0}}},
    {"carry W-1 drained through a skew-flagged last slot",
     {{JOIN, W - 1}, {JOIN, 0}, {JOIN, 0}, {SKEW, 0}}},
    {"early flush at k=0 [W,1,1,1]", {{JOIN, W}, {JOIN, 1}, {JOIN, 1}, {JOIN, 1}}},
    {"early flush first at k=1 [W-1,1,1,1]", {{JOIN, W - 1}, {JOIN, 1}, {JOIN, 1}, {JOIN, 1}}},
    {"early flush first at k=2 [W-2,1,1,1]", {{JOIN, W - 2}, {JOIN, 1}, {JOIN, 1}, {JOIN, 1}}},
    {"stage filled to exactly S [W-1,S-W+1,1,1]",
     {{JOIN, W - 1}, {JOIN, S - W + 1}, {JOIN, 1}, {JOIN, 1}}},
    {"exactly one spilled row [W-1,S-W+2,1,1]",
     {{JOIN, W - 1}, {JOIN, S - W + 2}, {JOIN, 1}, {JOIN, 1}}},
    {"one bucket of 5 x 64 x 64 duplicate matches", {{JOIN, 3}, {DUP, 5}, {JOIN, 2}, {JOIN, 1}}},
    {"all-empty group",
     {{EMPTY_BOTH, 0}, {EMPTY_BOTH, 0}, {EMPTY_BOTH, 0}, {EMPTY_BOTH, 0}}},
    {"four buckets with one empty side each",
     {{EMPTY_L, 0}, {EMPTY_R, 0}, {EMPTY_L, 0}, {EMPTY_R, 0}}},
  };
}
static const Pattern kFiller = {"filler", {{JOIN, 5}, {JOIN, 0}, {EMPTY_BOTH, 0}, {JOIN, 7}}};

/* what the kernel's stage does with one group, by arithmetic on the match
 * counts alone: a joined bucket stages its matches while the stage has room
 * and spills the rest; a slot before the last flushes when the stage holds
 * watermark rows or more; the last slot always flushes, joined or not */
struct Coverage {
  bool drain_empty_last = false, drain_skew_last = false, early[3] = {false, false, false};
  bool carry_below_water = false, exact_full = false, one_spill = false, heavy_spill = false;
  bool all_empty = false, one_sided = false;
};
struct Pred {
  int64_t staged = 0, spilled = 0;
  std::string flushes;
};

static Pred predict(const Pattern& p, Coverage& cov)
{
  const int S = g_shape.stage_rows, W = g_shape.watermark, KB = g_shape.flush_group;
  Pred pr;
  int64_t cur = 0, group_spilled = 0;
  bool flushed = false;
  int n_empty_both = 0, n_el = 0, n_er = 0;
  for (int k = 0; k < KB; k++) {
    const Slot& s = p.s[k];
    const bool joined = s.kind == JOIN || s.kind == DUP;
    n_empty_both += s.kind == EMPTY_BOTH;
    n_el += s.kind == EMPTY_L;
    n_er += s.kind == EMPTY_R;
    if (joined) {
      const int64_t m = slot_matches(s);
      const int64_t st = std::min<int64_t>(m, std::max<int64_t>(0, S - cur));
      pr.staged += st;
      pr.spilled += m - st;
      group_spilled += m - st;
      cur += m;
      if (m >= 4 * (int64_t)S) cov.heavy_spill = true;
    } else if (k != KB - 1) {
      continue;
    }
    if (k < KB - 1 && cur < W) {
      if (cur == W - 1) cov.carry_below_water = true;
      continue;
    }
    const int64_t rows = std::min<int64_t>(cur, S);
    if (k < KB - 1 && !flushed) cov.early[k] = true;
    if (k == KB - 1 && rows > 0 && !joined) {
      if (s.kind == SKEW) cov.drain_skew_last = true;
      else cov.drain_empty_last = true;
    }
    if (cur == S && group_spilled == 0) cov.exact_full = true;
    char buf[64];
    snprintf(buf, sizeof buf, " k=%d:%lld", k, (long long)rows);
    pr.flushes += buf;
    flushed = true;
    cur = 0;
  }
  if (group_spilled == 1) cov.one_spill = true;
  if (n_empty_both == KB) cov.all_empty = true;
  if (n_el + n_er == KB && n_el && n_er) cov.one_sided = true;
  return pr;
}

static Bucket make_slot(const Slot& s, int slots)
{
  Bucket b;
  switch (s.kind) {
    case JOIN:
      if (s.m + 2 > row_cap(slots)) bad_inputs("a JOIN slot exceeds the build-row cap");
      return match_bucket(s.m);
    case DUP: return dup_bucket(s.m, kDup);
    case EMPTY_BOTH: return b;
    case EMPTY_L:
      for (int i = 0; i < 9; i++) b.R.push_back({fresh_key(), rpay()});
      return b;
    case EMPTY_R:
      for (int i = 0; i < 11; i++) b.L.push_back({fresh_key(), lpay()});
      return b;
    case SKEW:
      /* probed for its own build keys: none of them may reach the output */
      return full_bucket(row_cap(slots) + 1, 3);
  }
  return b;
}

static void put_group(Case& c, int group, const Pattern& p)
{
  for (int k = 0; k < 4; k++) c.bk[(size_t)group * 4 + k] = make_slot(p.s[k], c.slots);
}

/* the pattern in the first, a middle and the last of five groups */
static Case stage_case(const Pattern& p, int slots)
{
  Case c;
  c.name = std::string("stage: ") + p.name;
  c.slots = slots;
  c.bk.resize(5 * 4);
  Coverage unused;
  c.pred_staged = c.pred_spilled = 0;
  for (int g = 0; g < 5; g++) {
    const Pattern& q = (g % 2 == 0) ? p : kFiller;
    put_group(c, g, q);
    const Pred pr = predict(q, unused);
    c.pred_staged += pr.staged;
    c.pred_spilled += pr.spilled;
  }
  return c;
}

/* ----------------------------------------------------------- other cases */

static Case build_edge_case(int slots)
{
  const int cap = row_cap(slots);
  Case c;
  c.name = "build-length edge 1, cap-1, cap, cap+1, 3*cap";
  c.slots = slots;
  c.fallback = true;
  c.bk.resize(8);
  c.bk[0] = full_bucket(1, 4);
  c.bk[1] = full_bucket(cap + 1, 50);  // flagged, between joined neighbours
  c.bk[2] = full_bucket(cap - 1, 50);
  c.bk[3] = full_bucket(cap, 50);  // must join, in the group's flush slot
  c.bk[4] = full_bucket(cap, 50);
  c.bk[5] = full_bucket(3 * cap, 50);  // flagged
  c.bk[6] = full_bucket(1, 0);
  c.bk[7] = full_bucket(cap + 1, 7);  // flagged, in the group's flush slot
  return c;
}

/* chain of buckets one block joins back to back — a whole group, then the
 * group of the block's next trip; each probes for the previous one's build
 * keys, which a table that was not cleared would still hold */
static Case table_reset_case(int slots)
{
  const int G = g_shape.grid_groups;
  Case c;
  c.name = "table reset between buckets, within a group and into the next trip";
  c.slots = slots;
  c.bk.resize((size_t)4 * (G + 1));
  const int nbuild[8] = {60, 50, 40, 30, 25, 20, 12, 5};
  const Bucket* prev = nullptr;
  for (int i = 0; i < 8; i++) {
    const size_t b = i < 4 ? (size_t)i : (size_t)4 * G + (i - 4);
    Bucket bu = match_bucket(nbuild[i] / 2, nbuild[i] - nbuild[i] / 2, 2);
    if (prev)
      for (const Row& r : prev->L) bu.R.push_back({r.k, rpay()});
    shuffle(bu.R);
    c.bk[b] = bu;
    prev = &c.bk[b];
  }
  return c;
}

/* small integers by home slot, for homes slots-4 .. slots-1 */
struct HomeKeys {
  std::vector<int64_t> at[4];
  int64_t searched = 0;
};
static HomeKeys find_home_keys(int slots, size_t need_last, size_t need_others)
{
  HomeKeys h;
  const uint32_t smask = (uint32_t)slots - 1;
  for (int64_t x = 1; x < (int64_t)1 << 31; x++) {
    const uint32_t home = (uint32_t)dj_mix64((uint64_t)x) & smask;
    if (home + 4 >= (uint32_t)slots) {
      const int i = (int)(home + 4 - (uint32_t)slots);
      if (h.at[i].size() < (i == 3 ? need_last : need_others)) h.at[i].push_back(x);
    }
    if (h.at[3].size() == need_last && h.at[0].size() == need_others &&
        h.at[1].size() == need_others && h.at[2].size() == need_others) {
      h.searched = x;
      return h;
    }
  }
  bad_inputs("no keys found for the last home slots of a %d-slot table", slots);
}

static Case wrap_case(int slots, bool report)
{
  const int cap = row_cap(slots);
  const HomeKeys h = find_home_keys(slots, (size_t)2 * cap + 20, 20);
  const uint32_t smask = (uint32_t)slots - 1;
  for (int i = 0; i < 4; i++)
    for (int64_t k : h.at[i])
      if (((uint32_t)dj_mix64((uint64_t)k) & smask) != (uint32_t)(slots - 4 + i))
        bad_inputs("home-slot search returned a key with another home");
  if (report)
    printf("inputs wrap-around slots=%d: %zu keys with home %d among integers 1..%lld\n", slots,
           h.at[3].size(), slots - 1, (long long)h.searched);
  Case c;
  c.name = "probe chain wrapping the table end";
  c.slots = slots;
  c.bk.resize(4);
  /* one chain of cap rows from slot slots-1 round to slot cap-2; absent keys
   * with the same home walk all of it to the first empty slot */
  Bucket& b0 = c.bk[0];
  for (int i = 0; i < cap; i++) {
    b0.L.push_back({h.at[3][(size_t)i], lpay()});
    b0.R.push_back({h.at[3][(size_t)i], rpay()});
    b0.R.push_back({h.at[3][(size_t)(cap + i)], rpay()});
  }
  for (int i = 0; i < 200; i++) b0.R.push_back({fresh_key(), rpay()});
  shuffle(b0.L);
  shuffle(b0.R);
  /* homes spread over the last four slots: present and absent keys of each */
  Bucket& b1 = c.bk[1];
  for (int s = 0; s < 4; s++) {
    const size_t base = s == 3 ? (size_t)2 * cap : 0;
    for (int i = 0; i < 10; i++) {
      b1.L.push_back({h.at[s][base + i], lpay()});
      b1.R.push_back({h.at[s][base + i], rpay()});
      b1.R.push_back({h.at[s][base + 10 + i], rpay()});
    }
  }
  shuffle(b1.L);
  shuffle(b1.R);
  c.bk[2] = match_bucket(3);
  c.bk[3] = match_bucket(0);
  return c;
}

static Case duplicates_case()
{
  Case c;
  c.name = "duplicate build keys, extreme keys, -1 on the probe side only";
  c.bk.resize(4);
  Bucket& b0 = c.bk[0];
  const int64_t x = fresh_key(), y = fresh_key();
  for (int i = 0; i < 5; i++) b0.L.push_back({x, lpay()});
  for (int i = 0; i < 3; i++) b0.L.push_back({y, lpay()});
  for (int i = 0; i < 4; i++) b0.L.push_back({fresh_key(), lpay()});
  b0.R = {{x, rpay()}, {y, rpay()}, {x, rpay()}, {fresh_key(), rpay()}, {fresh_key(), rpay()}};
  shuffle(b0.L);
  Bucket& b1 = c.bk[1];
  for (int64_t k : {INT64_MIN, INT64_MAX, (int64_t)0, (int64_t)-2, (int64_t)0}) {
    b1.L.push_back({k, lpay()});
    b1.R.push_back({k, rpay()});
  }
  b1.R.push_back({-1, rpay()});
  b1.R.push_back({fresh_key(), rpay()});
  c.bk[2] = match_bucket(1, 4, 0);
  for (int i = 0; i < 3; i++) c.bk[2].R.push_back({-1, rpay()});
  c.bk[3] = match_bucket(4);
  return c;
}

static Case sentinel_build_case()
{
  Case c;
  c.name = "-1 on the build side of a joined bucket";
  c.bk.resize(4);
  c.bk[0] = match_bucket(4, 2, 2);
  c.bk[0].L.push_back({-1, lpay()});
  c.bk[0].L.push_back({-1, lpay()});
  c.bk[0].R.push_back({-1, rpay()});
  c.bk[0].R.push_back({-1, rpay()});
  shuffle(c.bk[0].L);
  shuffle(c.bk[0].R);
  c.bk[1] = match_bucket(3);
  c.bk[3] = match_bucket(2);
  return c;
}

static Case sentinel_unjoined_case()
{
  Case c;
  c.name = "-1 on the build side of a bucket with an empty probe side";
  c.bk.resize(4);
  c.bk[0] = match_bucket(4);
  for (int i = 0; i < 3; i++) c.bk[1].L.push_back({i == 1 ? -1 : fresh_key(), lpay()});
  c.bk[2] = match_bucket(3);
  return c;
}

/* groups: pairs of (group index, pattern index into stage_patterns()) */
static Case second_trip_case(const char* what, int slots,
                             const std::vector<std::pair<int, int>>& groups)
{
  const std::vector<Pattern> pats = stage_patterns();
  Case c;
  c.name = std::string("second trip: ") + what;
  c.slots = slots;
  c.bk.resize((size_t)g_shape.flush_group * (g_shape.grid_groups + 2));
  Coverage unused;
  c.pred_staged = c.pred_spilled = 0;
  for (const auto& gp : groups) {
    put_group(c, gp.first, pats[(size_t)gp.second]);
    const Pred pr = predict(pats[(size_t)gp.second], unused);
    c.pred_staged += pr.staged;
    c.pred_spilled += pr.spilled;
  }
  return c;
}

/* --------------------------------------------------------------- reference */

struct Ref {
  std::vector<Tuple> rows;       // what lds_join alone must emit, sorted
  std::vector<Tuple> rows_full;  // with the flagged buckets joined too, sorted
  std::vector<uint32_t> flags;
  int any = 0, error = 0, error_full = 0;
};

static bool join_bucket(const Bucket& b, std::vector<Tuple>& out)
{
  bool saw_sentinel = false;
  std::unordered_multimap<int64_t, int64_t> tbl;
  tbl.reserve(b.L.size());
  for (const Row& r : b.L) {
    if (r.k == -1) {
      saw_sentinel = true;
      continue;
    }
    tbl.emplace(r.k, r.v);
  }
  for (const Row& r : b.R) {
    if (r.k == -1) continue;  // the empty-slot value ends the walk at once
    auto range = tbl.equal_range(r.k);
    for (auto it = range.first; it != range.second; ++it)
      out.push_back({r.k, it->second, r.k, r.v});
  }
  return saw_sentinel;
}

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
      if (join_bucket(bu, ref.rows_full)) ref.error_full = 1;
      continue;
    }
    const size_t before = ref.rows.size();
    if (join_bucket(bu, ref.rows)) ref.error = ref.error_full = 1;
    ref.rows_full.insert(ref.rows_full.end(), ref.rows.begin() + (long)before, ref.rows.end());
  }
  std::sort(ref.rows.begin(), ref.rows.end());
  std::sort(ref.rows_full.begin(), ref.rows_full.end());
  return ref;
}

static int64_t out_cap_of(const Case& c, const Ref& ref)
{
  const int64_t total = (int64_t)(c.fallback ? ref.rows_full.size() : ref.rows.size());
  switch (c.cap_mode) {
    case CAP_ZERO: return 0;
    case CAP_SMALL: return g_shape.watermark / 8;  // below any early flush
    case CAP_MID: return total / 2 + 1;
    default: return total + 8;
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

[[noreturn]] static void fail(const std::string& label, const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  printf("%s: FAILED\n  ", label.c_str());
  vprintf(fmt, ap);
  printf("\nLDS JOIN FAILED\n");
  va_end(ap);
  exit(1);
}

static void print_tuple(const char* what, const Tuple& t)
{
  printf("  %s (%lld, %lld, %lld, %lld)\n", what, (long long)t[0], (long long)t[1],
         (long long)t[2], (long long)t[3]);
}

struct Outputs {
  int64_t* col[4];
  int64_t cap;
  int64_t* counter;
  uint32_t* flags;
  int* any;
  int* error;
  int nflags;
};

static void verify(const std::string& label, const Outputs& o, const std::vector<Tuple>& want,
                   const std::vector<uint32_t>& want_flags, int want_any, int want_error)
{
  int64_t counter = -1;
  int any = -1, error = -1;
  std::vector<uint32_t> flags((size_t)o.nflags);
  CHECK(hipMemcpy(&counter, o.counter, 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&any, o.any, 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&error, o.error, 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(flags.data(), o.flags, flags.size() * 4, hipMemcpyDeviceToHost));
  const size_t alloc = (size_t)(o.cap + kGuardRows);
  std::vector<int64_t> col[4];
  for (int i = 0; i < 4; i++) {
    col[i].resize(alloc);
    CHECK(hipMemcpy(col[i].data(), o.col[i], alloc * 8, hipMemcpyDeviceToHost));
  }
  const int64_t total = (int64_t)want.size();
  if (counter != total) fail(label, "counter %lld, reference %lld", (long long)counter, (long long)total);
  for (size_t b = 0; b < flags.size(); b++) {
    const uint32_t w = b < want_flags.size() ? want_flags[b] : 0;
    if (flags[b] != w) fail(label, "overflow_flags[%zu] = %u, reference %u", b, flags[b], w);
  }
  if (any != want_any) fail(label, "any_overflow %d, reference %d", any, want_any);
  if (error != want_error) fail(label, "error word %d, reference %d", error, want_error);
  const int64_t written = std::min(total, o.cap);
  for (int i = 0; i < 4; i++)
    for (size_t r = (size_t)written; r < alloc; r++)
      if (col[i][r] != kFill)
        fail(label, "out%d[%zu] overwritten (%lld) — %lld rows written, cap %lld", i, r,
             (long long)col[i][r], (long long)written, (long long)o.cap);
  std::vector<Tuple> got((size_t)written);
  for (size_t r = 0; r < got.size(); r++) got[r] = {col[0][r], col[1][r], col[2][r], col[3][r]};
  std::sort(got.begin(), got.end());
  if (written == total) {
    for (size_t r = 0; r < got.size(); r++)
      if (got[r] != want[r]) {
        printf("%s: FAILED\n  sorted row %zu differs\n", label.c_str(), r);
        print_tuple("got ", got[r]);
        print_tuple("want", want[r]);
        printf("LDS JOIN FAILED\n");
        exit(1);
      }
  } else {
    /* truncated: no tuple more often than the reference has it */
    size_t w = 0;
    for (size_t r = 0; r < got.size(); r++) {
      while (w < want.size() && want[w] < got[r]) w++;
      if (w == want.size() || want[w] != got[r]) {
        printf("%s: FAILED\n  truncated output holds a row more often than the reference\n",
               label.c_str());
        print_tuple("got ", got[r]);
        printf("LDS JOIN FAILED\n");
        exit(1);
      }
      w++;
    }
  }
}

/* rows of one slack segment: the bucket's own, then poison up to the capacity
 * with keys of the bucket's other side */
static std::vector<Row> slack_segment(const std::vector<Row>& own, const std::vector<Row>& other,
                                      int64_t cap)
{
  std::vector<Row> seg(own);
  for (size_t i = own.size(); i < (size_t)cap; i++) {
    int64_t k;
    if (!other.empty()) k = other[i % other.size()].k;
    else if (!own.empty()) k = own[i % own.size()].k;
    else k = 0x5000 + (int64_t)(i & 3);  // the same on both sides of an empty bucket
    seg.push_back({k, poison_pay()});
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
  const int Bk = slack ? B + g_shape.flush_group : B;
  const Bucket empty;
  Dev dev;
  Row *d_l, *d_r;
  std::vector<int64_t> lstart((size_t)B), rstart((size_t)B);
  int64_t* d_loff = nullptr;
  int64_t* d_roff = nullptr;
  uint32_t* d_llen = nullptr;
  uint32_t* d_rlen = nullptr;
  int64_t capL = 0, capR = 0;
  if (slack) {
    size_t maxL = 0, maxR = 0;
    for (const Bucket& bu : c.bk) {
      maxL = std::max(maxL, bu.L.size());
      maxR = std::max(maxR, bu.R.size());
    }
    capL = (int64_t)maxL + 3;
    capR = (int64_t)maxR + 9;
    if (capL == capR) capR++;
    std::vector<uint32_t> llen((size_t)Bk, 0), rlen((size_t)Bk, 0);
    d_l = dev.alloc<Row>((size_t)Bk * capL);
    d_r = dev.alloc<Row>((size_t)Bk * capR);
    /* segments of the many empty buckets of a large B stay -1 rows: read as
     * build rows they set the error word */
    CHECK(hipMemset(d_l, 0xFF, (size_t)Bk * capL * sizeof(Row)));
    CHECK(hipMemset(d_r, 0xFF, (size_t)Bk * capR * sizeof(Row)));
    const bool dense = Bk <= 256;
    for (int b = 0; b < Bk; b++) {
      const Bucket& bu = b < B ? c.bk[(size_t)b] : empty;
      if (b < B) {
        llen[(size_t)b] = (uint32_t)bu.L.size();
        rlen[(size_t)b] = (uint32_t)bu.R.size();
        lstart[(size_t)b] = (int64_t)b * capL;
        rstart[(size_t)b] = (int64_t)b * capR;
      }
      if (!dense && b < B && bu.L.empty() && bu.R.empty()) continue;
      const std::vector<Row> ls = slack_segment(bu.L, bu.R, capL);
      const std::vector<Row> rs = slack_segment(bu.R, bu.L, capR);
      CHECK(hipMemcpy(d_l + (int64_t)b * capL, ls.data(), ls.size() * sizeof(Row),
                      hipMemcpyHostToDevice));
      CHECK(hipMemcpy(d_r + (int64_t)b * capR, rs.data(), rs.size() * sizeof(Row),
                      hipMemcpyHostToDevice));
    }
    d_llen = dev.alloc<uint32_t>((size_t)Bk);
    d_rlen = dev.alloc<uint32_t>((size_t)Bk);
    CHECK(hipMemcpy(d_llen, llen.data(), (size_t)Bk * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_rlen, rlen.data(), (size_t)Bk * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<Row> hl, hr;
    std::vector<int64_t> loff((size_t)B + 1), roff((size_t)B + 1);
    for (int b = 0; b < B; b++) {
      const Bucket& bu = c.bk[(size_t)b];
      loff[(size_t)b] = lstart[(size_t)b] = (int64_t)hl.size();
      roff[(size_t)b] = rstart[(size_t)b] = (int64_t)hr.size();
      hl.insert(hl.end(), bu.L.begin(), bu.L.end());
      hr.insert(hr.end(), bu.R.begin(), bu.R.end());
    }
    loff[(size_t)B] = (int64_t)hl.size();
    roff[(size_t)B] = (int64_t)hr.size();
    d_l = dev.alloc<Row>(hl.size());
    d_r = dev.alloc<Row>(hr.size());
    d_loff = dev.alloc<int64_t>((size_t)B + 1);
    d_roff = dev.alloc<int64_t>((size_t)B + 1);
    if (!hl.empty())
      CHECK(hipMemcpy(d_l, hl.data(), hl.size() * sizeof(Row), hipMemcpyHostToDevice));
    if (!hr.empty())
      CHECK(hipMemcpy(d_r, hr.data(), hr.size() * sizeof(Row), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_loff, loff.data(), ((size_t)B + 1) * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_roff, roff.data(), ((size_t)B + 1) * 8, hipMemcpyHostToDevice));
  }

  Outputs o;
  o.cap = out_cap_of(c, ref);
  o.nflags = Bk;
  for (int i = 0; i < 4; i++) {
    o.col[i] = dev.alloc<int64_t>((size_t)(o.cap + kGuardRows));
    CHECK(hipMemset(o.col[i], kPoison, (size_t)(o.cap + kGuardRows) * 8));
  }
  o.counter = dev.alloc<int64_t>(1);
  o.flags = dev.alloc<uint32_t>((size_t)Bk);
  o.any = dev.alloc<int>(1);
  o.error = dev.alloc<int>(1);
  CHECK(hipMemset(o.counter, 0, 8));
  CHECK(hipMemset(o.flags, 0, (size_t)Bk * 4));
  CHECK(hipMemset(o.any, 0, 4));
  CHECK(hipMemset(o.error, 0, 4));

  if (slack)
    dj::lds_join_slack((const longlong2*)d_l, d_llen, capL, (const longlong2*)d_r, d_rlen, capR,
                       Bk, c.slots, o.col[0], o.col[1], o.col[2], o.col[3], o.cap, o.counter,
                       o.flags, o.any, o.error, nullptr);
  else
    dj::lds_join((const longlong2*)d_l, d_loff, (const longlong2*)d_r, d_roff, B, c.slots,
                 o.col[0], o.col[1], o.col[2], o.col[3], o.cap, o.counter, o.flags, o.any,
                 o.error, nullptr);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  verify(label + (c.fallback ? " (before the fallback)" : ""), o, ref.rows, ref.flags, ref.any,
         ref.error);

  if (c.fallback) {
    /* the flagged buckets, joined the way the product's fallback joins them */
    for (int b = 0; b < B; b++) {
      if (!ref.flags[(size_t)b]) continue;
      const Bucket& bu = c.bk[(size_t)b];
      const int64_t nslots = dj::join_table_slots((int64_t)bu.L.size());
      int64_t* d_table = nullptr;
      CHECK(hipMalloc(&d_table, (size_t)nslots * 2 * sizeof(int64_t)));
      CHECK(hipMemset(d_table, 0xFF, (size_t)nslots * 2 * sizeof(int64_t)));
      dj::join_build_pairs((const longlong2*)d_l + lstart[(size_t)b], (int64_t)bu.L.size(),
                           d_table, nslots, o.error, nullptr);
      dj::join_probe_pairs((const longlong2*)d_r + rstart[(size_t)b], (int64_t)bu.R.size(),
                           d_table, nslots, o.col[0], o.col[1], o.col[2], o.col[3], o.cap,
                           o.counter, nullptr);
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
      CHECK(hipFree(d_table));
    }
    verify(label + " (after the fallback)", o, ref.rows_full, ref.flags, ref.any,
           ref.error_full);
  }
  dev.release();
  printf("%s: ok\n", label.c_str());
}

/* ---------------------------------------------------------------- main */

static std::vector<Case> build_cases(bool report)
{
  const int S = g_shape.stage_rows, W = g_shape.watermark;
  if (g_shape.flush_group != 4) bad_inputs("the stage patterns are written for groups of 4");
  if (!(W >= 16 && W < S && S - W + 2 + 2 <= row_cap(2048)))
    bad_inputs("stage %d / watermark %d do not fit the patterns", S, W);

  const std::vector<Pattern> pats = stage_patterns();
  Coverage cov;
  for (const Pattern& p : pats) {
    const Pred pr = predict(p, cov);
    if (report)
      printf("inputs pattern '%s': flushes%s, staged %lld, spilled %lld\n", p.name,
             pr.flushes.empty() ? " none" : pr.flushes.c_str(), (long long)pr.staged,
             (long long)pr.spilled);
  }
  const struct {
    bool have;
    const char* what;
  } needed[] = {
    {cov.drain_empty_last, "carry drained through an empty last slot"},
    {cov.drain_skew_last, "carry drained through a skew-flagged last slot"},
    {cov.early[0], "early flush at k=0"},
    {cov.early[1], "early flush first at k=1"},
    {cov.early[2], "early flush first at k=2"},
    {cov.carry_below_water, "carry of W-1 rows that does not flush"},
    {cov.exact_full, "stage filled to exactly S without a spill"},
    {cov.one_spill, "exactly one spilled row"},
    {cov.heavy_spill, "one bucket with many times S matches"},
    {cov.all_empty, "all-empty group"},
    {cov.one_sided, "group of four buckets with one empty side each"},
  };
  for (const auto& n : needed)
    if (!n.have) bad_inputs("no stage pattern gives: %s", n.what);

  std::vector<Case> cases;
  for (int slots : {2048, 4096}) cases.push_back(build_edge_case(slots));
  for (int slots : {2048, 4096}) cases.push_back(table_reset_case(slots));
  for (int slots : {2048, 4096})
    for (const Pattern& p : pats) cases.push_back(stage_case(p, slots));
  const struct {
    CapMode mode;
    const char* tag;
  } caps[] = {{CAP_ZERO, " (cap 0)"},
              {CAP_SMALL, " (cap below one flush)"},
              {CAP_MID, " (cap mid-output)"}};
  for (const auto& cm : caps)
    for (const Pattern& p : pats) {
      Case c = stage_case(p, 2048);
      c.cap_mode = cm.mode;
      c.name += cm.tag;
      cases.push_back(c);
    }
  for (int slots : {2048, 4096}) cases.push_back(wrap_case(slots, report));
  cases.push_back(duplicates_case());
  cases.push_back(sentinel_build_case());
  cases.push_back(sentinel_unjoined_case());
  const int G = g_shape.grid_groups;
  /* pattern indices: 6 one spill, 3 flush at k=1, 2 flush at k=0, 0 drain */
  cases.push_back(second_trip_case("groups 0 and grid_groups (one block, both trips)", 2048,
                                   {{0, 6}, {G, 3}}));
  cases.push_back(second_trip_case("group 1 only (first trip)", 4096, {{1, 2}}));
  cases.push_back(second_trip_case("group grid_groups+1 only (second trip)", 2048,
                                   {{G + 1, 0}}));
  return cases;
}

int main(int argc, char** argv)
{
  const bool inputs_only = argc > 1 && strcmp(argv[1], "--inputs-only") == 0;
  const bool bad_b = argc > 1 && strcmp(argv[1], "--bad-b") == 0;
  if (argc > 1 && !inputs_only && !bad_b) {
    printf("usage: lds_join_check [--inputs-only | --bad-b]\n");
    return 2;
  }
  if (bad_b) {
    dj::lds_join(nullptr, nullptr, nullptr, nullptr, 6, 2048, nullptr, nullptr, nullptr,
                 nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    printf("B = 6 WAS NOT REJECTED\n");
    return 3;
  }
  g_shape = dj::lds_join_shape();
  const std::vector<Case> cases = build_cases(inputs_only);
  /* every input check comes before the first launch */
  std::vector<Ref> refs;
  bool mid_staged = false, mid_spill = false;
  for (const Case& c : cases) {
    refs.push_back(reference(c));
    const Ref& ref = refs.back();
    const int64_t total = (int64_t)ref.rows.size();
    if (c.pred_staged >= 0 && c.pred_staged + c.pred_spilled != total)
      bad_inputs("'%s': predicted %lld staged + %lld spilled rows, reference %lld",
                 c.name.c_str(), (long long)c.pred_staged, (long long)c.pred_spilled,
                 (long long)total);
    if (c.cap_mode == CAP_MID && total > 1) {
      const int64_t cap = out_cap_of(c, ref);
      /* all rows staged: the cut falls inside the staged flushes; far more
       * spilled than staged rows on either side of the cut: inside a spill */
      if (c.pred_spilled == 0 && cap < total) mid_staged = true;
      if (cap > c.pred_staged && total - cap > c.pred_staged) mid_spill = true;
    }
    if (inputs_only) {
      size_t nl = 0, nr = 0, flagged = 0;
      for (const Bucket& b : c.bk) nl += b.L.size(), nr += b.R.size();
      for (uint32_t f : ref.flags) flagged += f;
      printf("inputs %s [slots=%d B=%zu]: %zu x %zu rows, %lld matches, %zu flagged, cap %lld\n",
             c.name.c_str(), c.slots, c.bk.size(), nl, nr,
             (long long)(c.fallback ? ref.rows_full.size() : ref.rows.size()), flagged,
             (long long)out_cap_of(c, ref));
    }
  }
  if (!mid_staged || !mid_spill)
    bad_inputs("no capacity cuts through a %s", mid_staged ? "spill" : "staged flush");
  if (inputs_only) {
    printf("LDS JOIN INPUTS OK (%zu cases)\n", cases.size());
    return 0;
  }
  int runs = 0;
  for (size_t i = 0; i < cases.size(); i++) {
    run_case(cases[i], refs[i], false);
    run_case(cases[i], refs[i], true);
    runs += 2;
  }
  printf("LDS JOIN OK (%d runs)\n", runs);
  return 0;
}
