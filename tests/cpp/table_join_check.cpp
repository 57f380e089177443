/*
 * table_join_check.cpp — the global-table join (dj::join_build / join_probe,
 * join_build_pairs / join_probe_pairs: the last-resort path after two slack
 * overflows, the per-bucket skew fallback and the engine of
 * dj_local_inner_join_global) and dj::neg1_cross_join, called directly and
 * compared, exactly, with a host prediction.
 *
 * Host reference: a multimap join. Build payloads are 7*i+3 and probe payloads
 * 11*j+5 (the row numbers i and j when the payload pointers are null), so an
 * output row names the pair of input rows it joins: "the multiset of output
 * rows equals the reference's" is checked as "every written row (out0, out1,
 * out2, out3) has out0 == out2 == the key of build row i and of probe row j,
 * that key is not -1, no pair (i, j) is written twice, and the count equals
 * the multimap's".
 *
 * Every join case builds three times — columns with payloads (error word
 * preset 0), columns with null payloads (preset 1), pairs (preset 0; the pair
 * pointers are base + 1, aligned to 16 bytes only) — and after each build
 * reads the table back:
 *   - every build row with key != -1 appears exactly once as {key, payload},
 *     every other slot is {-1, -1};
 *   - walking from dj_mix64(key) & mask, each entry is reached before any
 *     empty slot;
 *   - the error word is preset | (some build key is -1).
 * Then it probes with start counter 0 and 1000 and cap 0, start + 37,
 * start + total - 1 and start + total:
 *   - the counter reads start + total;
 *   - rows [start, min(cap, start + total)) are written and belong to the
 *     reference, each pair once; every other row of the outputs, before start
 *     and from cap on, keeps its poison.
 * neg1_cross_join runs with payloads and without, with the same start counters
 * and caps: the appended rows are the cross product of the two sides' -1
 * rows, each pair once, -1 in both key columns; an empty side appends nothing
 * and leaves the counter alone. Its int64 overflow guard of the product needs
 * billions of rows and is not tested.
 *
 * The table, the four outputs, the counter and the error word each sit between
 * two guards of kGuard poisoned elements, checked after every run. A table
 * smaller than join_table_slots(ln) is never passed: a full table makes the
 * build spin forever.
 *
 * Every size derives from dj::table_join_shape().
 *
 * usage: table_join_check [--inputs-only] [--set sizes|edges|neg1]
 *   --inputs-only: the join_table_slots checks, every case's inputs and host
 *   reference; fails if a case misses the situation it is named for (needs no
 *   GPU).
 * Build/run: tests/test_gpu_table_join.py.
 */
#include "bucket_model.hpp"
#include "check.hpp"

#include "dj_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

static dj::TableJoinShape g_sh;
constexpr size_t kGuard = 128; /* poisoned elements on either side of a written buffer */
constexpr int64_t kStarts[] = {0, 1000};
constexpr int64_t kCut = 37; /* cap = start + kCut falls inside a wave's append */
constexpr int64_t kTail = 64; /* output rows allocated past start + total */

static size_t g_bytes = 0, g_largest = 0; /* device bytes of the running case */

/* a device buffer of n elements between two poisoned guards */
template <class T>
struct Guarded {
  T* base = nullptr;
  size_t n = 0;
  void alloc(size_t n_)
  {
    n = n_;
    CHECK(hipMalloc(&base, (n + 2 * kGuard) * sizeof(T)));
    g_bytes += (n + 2 * kGuard) * sizeof(T);
  }
  T* p() { return base + kGuard; }
  void poison() { CHECK(hipMemset(base, kPoison, (n + 2 * kGuard) * sizeof(T))); }
  /* the payload alone; guards_ok() reads the guards */
  std::vector<T> read()
  {
    std::vector<T> v(n);
    CHECK(hipMemcpy(v.data(), p(), n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
  }
  bool guards_ok()
  {
    std::vector<T> g(2 * kGuard);
    CHECK(hipMemcpy(g.data(), base, kGuard * sizeof(T), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g.data() + kGuard, base + kGuard + n, kGuard * sizeof(T),
                    hipMemcpyDeviceToHost));
    return all_poison(g.data(), 2 * kGuard * sizeof(T));
  }
  void release()
  {
    CHECK(hipFree(base));
    g_bytes -= (n + 2 * kGuard) * sizeof(T);
    base = nullptr;
  }
};

/* an input on the device, `lead` elements after the allocation's start */
template <class T>
static T* upload(const std::vector<T>& v, size_t lead, T** base)
{
  CHECK(hipMalloc(base, (v.size() + lead + 1) * sizeof(T)));
  g_bytes += (v.size() + lead + 1) * sizeof(T);
  CHECK(hipMemcpy(*base + lead, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return *base + lead;
}
template <class T>
static void drop(T* base, size_t elems)
{
  CHECK(hipFree(base));
  g_bytes -= (elems + 1) * sizeof(T);
}

static int64_t lpay_of(bool null_pay, int64_t i) { return null_pay ? i : 7 * i + 3; }
static int64_t rpay_of(bool null_pay, int64_t j) { return null_pay ? j : 11 * j + 5; }
/* the row a payload names, or -1 */
static int64_t row_of(bool null_pay, int64_t pay, int64_t mul, int64_t add, int64_t n)
{
  int64_t r = pay;
  if (!null_pay) {
    if (pay < add || (pay - add) % mul) return -1;
    r = (pay - add) / mul;
  }
  return r >= 0 && r < n ? r : -1;
}

static uint64_t home_of(int64_t key, uint64_t mask) { return dj_mix64((uint64_t)key) & mask; }

/* ---------------- join cases ---------------- */

struct JoinCase {
  std::string name;
  std::vector<int64_t> lk, rk;
  /* the situation the case is named for, checked by inputs_ok() */
  bool want_wrap = false, want_hot = false, want_trip = false, want_neg1_build = false;
  int64_t hot_key = 0, second_key = 0;
};
struct Ref {
  int64_t total = 0;
  bool neg1_build = false;
  std::vector<int64_t> per_probe; /* matches of probe row j */
};
static Ref reference(const JoinCase& c)
{
  std::unordered_multimap<int64_t, int64_t> mm;
  Ref r;
  for (size_t i = 0; i < c.lk.size(); i++) {
    if (c.lk[i] == -1)
      r.neg1_build = true;
    else
      mm.emplace(c.lk[i], (int64_t)i);
  }
  r.per_probe.resize(c.rk.size());
  for (size_t j = 0; j < c.rk.size(); j++) {
    r.per_probe[j] = c.rk[j] == -1 ? 0 : (int64_t)mm.count(c.rk[j]);
    r.total += r.per_probe[j];
  }
  return r;
}

/* sizes of the append groups of a probe of at most one wave, in order: round r
 * appends one row for every lane with more than r matches */
static std::vector<int64_t> one_wave_groups(const Ref& r)
{
  std::vector<int64_t> g;
  for (int64_t round = 0;; round++) {
    int64_t lanes = 0;
    for (int64_t m : r.per_probe) lanes += m > round;
    if (!lanes) break;
    g.push_back(lanes);
  }
  return g;
}
static bool cut_inside_group(const Ref& r, int64_t cut)
{
  int64_t pre = 0;
  for (int64_t g : one_wave_groups(r)) {
    if (pre < cut && cut < pre + g) return true;
    pre += g;
  }
  return false;
}

struct JoinSituations {
  int cut_inside = 0, last_cut_inside = 0;
};

static bool inputs_ok(const JoinCase& c, const Ref& r, JoinSituations& sit)
{
  const int64_t ln = (int64_t)c.lk.size(), rn = (int64_t)c.rk.size();
  const int64_t nslots = dj::join_table_slots(ln);
  const uint64_t mask = (uint64_t)nslots - 1;
  const int64_t T = (int64_t)g_sh.block * g_sh.grid_cap;
  printf("inputs %s: ln=%lld rn=%lld nslots=%lld total=%lld%s\n", c.name.c_str(), (long long)ln,
         (long long)rn, (long long)nslots, (long long)r.total,
         r.neg1_build ? ", -1 on the build side" : "");
  auto bad = [&](const char* what) {
    printf("BAD TEST INPUTS: %s: %s\n", c.name.c_str(), what);
    return false;
  };
  if (nslots < 2 * ln + 1) return bad("table too small");
  if (c.want_neg1_build != r.neg1_build) return bad("-1 on the build side, or not, against the name");
  if (rn <= 64) { /* one wave: the order of its appends is fixed */
    if (cut_inside_group(r, kCut)) sit.cut_inside++;
    if (r.total >= 2 && cut_inside_group(r, r.total - 1)) sit.last_cut_inside++;
  }
  if (c.want_wrap) {
    /* the occupied slots of a linear-probing table do not depend on the
     * insertion order: fill one on the host */
    std::vector<char> occ((size_t)nslots, 0);
    int64_t at_end = 0, probed = 0;
    for (int64_t k : c.lk) {
      uint64_t s = home_of(k, mask);
      if (s >= mask - 1) at_end++;
      while (occ[s]) s = (s + 1) & mask;
      occ[s] = 1;
    }
    for (int64_t j = 0; j < rn; j++)
      if (home_of(c.rk[(size_t)j], mask) >= mask - 1 && r.per_probe[(size_t)j] >= 2) probed++;
    /* more rows homed in the last two slots than those hold: the rest sit in
     * slots 0, 1, ... and every slot of the chain up to there is taken */
    if (at_end < 8 || probed < 4) return bad("too few rows or probes homed at the table's end");
    for (uint64_t s : {mask - 1, mask, (uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3})
      if (!occ[s]) return bad("the chain does not cross the table's end");
  }
  if (c.want_hot) {
    const uint64_t h = home_of(c.hot_key, mask), h2 = home_of(c.second_key, mask);
    int64_t hot_rows = 0;
    for (int64_t k : c.lk) hot_rows += k == c.hot_key;
    if (hot_rows != 3000) return bad("the hot key is not there 3000 times");
    const uint64_t dist = (h2 - h) & mask;
    if (dist == 0 || dist >= 3000) return bad("the second key's home slot is outside the run");
    if (rn > 64) return bad("the probe side is more than one wave");
    bool m0 = false, m1 = false, m3000 = false;
    for (int64_t m : r.per_probe) {
      m0 |= m == 0;
      m1 |= m == 1;
      m3000 |= m == 3000;
    }
    if (!m0 || !m1 || !m3000) return bad("the wave lacks a lane with 0, 1 or 3000 matches");
    if (!cut_inside_group(r, kCut) || !cut_inside_group(r, r.total - 1))
      return bad("a cut cap falls on a group boundary");
  }
  if (c.want_trip) {
    if (ln != T + 300 || rn != 2 * T + 77) return bad("not the trip sizes");
    std::unordered_map<int64_t, int> probe_keys;
    for (int64_t k : c.rk) probe_keys[k] = 1;
    for (int64_t i = 0; i < T; i++)
      if (probe_keys.count(c.lk[(size_t)i])) return bad("a build row of the first trip matches");
    int64_t later = 0, third = 0;
    for (int64_t j = 0; j < rn; j++) {
      if (j < T && r.per_probe[(size_t)j]) return bad("a probe row of the first trip matches");
      if (j >= T && r.per_probe[(size_t)j]) later++;
      if (j >= 2 * T && r.per_probe[(size_t)j]) third++;
    }
    if (!later || !third) return bad("no match in the second or the third trip");
  }
  return true;
}

static JoinCase sized(int64_t ln, int64_t rn)
{
  JoinCase c;
  c.name = "sizes ln=" + std::to_string(ln) + " rn=" + std::to_string(rn);
  for (int64_t i = 0; i < ln; i++) c.lk.push_back(hkey(1, (uint64_t)(i % 4 == 3 ? i - 1 : i)));
  for (int64_t j = 0; j < rn; j++)
    c.rk.push_back(j % 5 == 4 ? hkey(2, (uint64_t)j) : hkey(1, (uint64_t)((j * 7) % ln)));
  return c;
}

static JoinCase wrap_case()
{
  JoinCase c;
  c.name = "chain across the table's end";
  c.want_wrap = true;
  const int64_t ln = 200;
  const uint64_t mask = (uint64_t)dj::join_table_slots(ln) - 1;
  std::vector<int64_t> enders;
  for (uint64_t i = 0; enders.size() < 6; i++)
    if (home_of(hkey(7, i), mask) >= mask - 1) enders.push_back(hkey(7, i));
  /* each of them three times, spread among fillers */
  for (int64_t i = 0, e = 0; i < ln; i++) {
    if (i % 11 == 5 && e < 18)
      c.lk.push_back(enders[(size_t)(e++ % 6)]);
    else
      c.lk.push_back(hkey(8, (uint64_t)i));
  }
  for (int64_t j = 0; j < 40; j++) {
    if (j % 3 == 0)
      c.rk.push_back(enders[(size_t)((j / 3) % 6)]);
    else if (j % 3 == 1)
      c.rk.push_back(hkey(8, (uint64_t)j)); /* a filler, or absent where an ender took its row */
    else
      c.rk.push_back(hkey(2, (uint64_t)j)); /* absent */
  }
  return c;
}

static JoinCase hot_case()
{
  JoinCase c;
  c.name = "one key 3000 times, a second key inside its run";
  c.want_hot = true;
  const int64_t fillers = 150, ln = 3000 + 1 + fillers;
  const uint64_t mask = (uint64_t)dj::join_table_slots(ln) - 1;
  c.hot_key = hkey(9, 0);
  const uint64_t h = home_of(c.hot_key, mask);
  for (uint64_t i = 0;; i++) {
    const uint64_t dist = (home_of(hkey(10, i), mask) - h) & mask;
    if (dist >= 500 && dist < 2500) {
      c.second_key = hkey(10, i);
      break;
    }
  }
  for (int64_t i = 0; i < ln; i++) {
    if (i == 1700)
      c.lk.push_back(c.second_key);
    else if (i % 21 == 0 && i / 21 < fillers)
      c.lk.push_back(hkey(11, (uint64_t)(i / 21)));
    else
      c.lk.push_back(c.hot_key);
  }
  for (int64_t j = 0; j < 64; j++) {
    switch (j % 8) {
      case 0: c.rk.push_back(c.hot_key); break;
      case 1: c.rk.push_back(c.second_key); break;
      case 2: c.rk.push_back(hkey(2, (uint64_t)j)); break; /* absent */
      default: c.rk.push_back(hkey(11, (uint64_t)j)); break; /* a filler */
    }
  }
  return c;
}

static JoinCase special_case()
{
  JoinCase c;
  c.name = "special keys";
  const int64_t sp[] = {INT64_MIN, INT64_MAX, 0, -2, 4294967295LL};
  for (int rep = 0; rep < 2; rep++)
    for (int64_t k : sp) {
      c.lk.push_back(k);
      c.lk.push_back(hkey(12, (uint64_t)c.lk.size()));
    }
  c.lk.push_back(0);
  for (int rep = 0; rep < 3; rep++)
    for (int64_t k : sp) {
      c.rk.push_back(k);
      c.rk.push_back(hkey(2, (uint64_t)c.rk.size()));
    }
  c.rk.push_back(1);
  c.rk.push_back(-3);
  return c;
}

static JoinCase neg1_probe_case(bool build_too)
{
  JoinCase c;
  c.name = build_too ? "-1 on both sides matches nothing" : "-1 probe rows match nothing";
  c.want_neg1_build = build_too;
  for (int64_t i = 0; i < 300; i++)
    c.lk.push_back(build_too && i % 97 == 13 ? -1 : hkey(13, (uint64_t)(i / 2)));
  for (int64_t j = 0; j < 200; j++)
    c.rk.push_back(j % 9 == 2 ? -1 : j % 9 == 5 ? hkey(2, (uint64_t)j) : hkey(13, (uint64_t)j));
  return c;
}

static JoinCase trip_case()
{
  JoinCase c;
  c.name = "matches past the first trip only";
  c.want_trip = true;
  const int64_t T = (int64_t)g_sh.block * g_sh.grid_cap, ln = T + 300, rn = 2 * T + 77;
  c.lk.resize((size_t)ln);
  c.rk.resize((size_t)rn);
  for (int64_t i = 0; i < ln; i++)
    c.lk[(size_t)i] = i < T ? hkey(14, (uint64_t)i) : hkey(15, (uint64_t)((i - T) / 2));
  for (int64_t j = 0; j < rn; j++) {
    const bool hit = (j >= T && j < T + 40) || (j >= 2 * T - 20 && j % 3 == 0);
    c.rk[(size_t)j] = hit ? hkey(15, (uint64_t)(j % 150)) : hkey(16, (uint64_t)j);
  }
  return c;
}

/* ---------------- a join case on the device ---------------- */

struct Form {
  const char* name;
  bool pairs, null_pay;
  int preset;
};
static const Form kForms[] = {{"columns", false, false, 0},
                              {"columns, null payloads", false, true, 1},
                              {"pairs", true, false, 0}};

static int check_table(const JoinCase& c, const Form& f, const std::vector<longlong2>& tab,
                       int64_t nslots)
{
  int bad = 0;
  auto fail = [&](const char* what, long long a, long long b) {
    if (bad++ < 6) printf("  FAIL %s, table: %s (%lld, %lld)\n", f.name, what, a, b);
  };
  const int64_t ln = (int64_t)c.lk.size();
  const uint64_t mask = (uint64_t)nslots - 1;
  std::vector<char> seen((size_t)ln, 0);
  int64_t stored = 0, expected = 0;
  for (int64_t k : c.lk) expected += k != -1;
  for (int64_t s = 0; s < nslots; s++) {
    const longlong2 e = tab[(size_t)s];
    if (e.x == -1) {
      if (e.y != -1) fail("an empty slot holds a payload (slot, payload)", s, e.y);
      continue;
    }
    const int64_t i = row_of(f.null_pay, e.y, 7, 3, ln);
    if (i < 0 || c.lk[(size_t)i] != e.x) {
      fail("an entry is no build row (slot, payload)", s, e.y);
    } else if (seen[(size_t)i]) {
      fail("a build row is stored twice (slot, row)", s, i);
    } else {
      seen[(size_t)i] = 1;
      stored++;
    }
    for (uint64_t t = home_of(e.x, mask); t != (uint64_t)s; t = (t + 1) & mask)
      if (tab[t].x == -1) {
        fail("an empty slot lies between an entry and its home (slot, empty slot)", s,
             (long long)t);
        break;
      }
  }
  if (stored != expected) fail("stored rows != build rows with a key (stored, expected)", stored, expected);
  return bad;
}

static int run_join_case(const JoinCase& c, const Ref& ref, int* runs)
{
  const int64_t ln = (int64_t)c.lk.size(), rn = (int64_t)c.rk.size();
  const int64_t nslots = dj::join_table_slots(ln);
  const size_t out_rows = (size_t)(kStarts[1] + ref.total + kTail);
  int bad = 0;
  auto fail = [&](const Form& f, int64_t start, int64_t cap, const char* what, long long a,
                  long long b) {
    if (bad++ < 8)
      printf("  FAIL %s, start %lld cap %lld: %s (%lld, %lld)\n", f.name, (long long)start,
             (long long)cap, what, a, b);
  };

  Guarded<longlong2> table;
  Guarded<int64_t> out[4], counter;
  Guarded<int> err;
  table.alloc((size_t)nslots);
  for (auto& o : out) o.alloc(out_rows);
  counter.alloc(1);
  err.alloc(1);

  for (const Form& f : kForms) {
    /* inputs */
    std::vector<int64_t> lp((size_t)ln), rp((size_t)rn);
    std::vector<longlong2> lrows((size_t)ln), rrows((size_t)rn);
    for (int64_t i = 0; i < ln; i++) {
      lp[(size_t)i] = lpay_of(f.null_pay, i);
      lrows[(size_t)i] = {c.lk[(size_t)i], lp[(size_t)i]};
    }
    for (int64_t j = 0; j < rn; j++) {
      rp[(size_t)j] = rpay_of(f.null_pay, j);
      rrows[(size_t)j] = {c.rk[(size_t)j], rp[(size_t)j]};
    }
    int64_t *b_lk = nullptr, *b_lp = nullptr, *b_rk = nullptr, *b_rp = nullptr;
    longlong2 *b_lrows = nullptr, *b_rrows = nullptr;
    const int64_t *d_lk = nullptr, *d_lp = nullptr, *d_rk = nullptr, *d_rp = nullptr;
    const longlong2 *d_lrows = nullptr, *d_rrows = nullptr;
    if (f.pairs) {
      /* base + 1: aligned to 16 bytes and no more */
      d_lrows = upload(lrows, 1, &b_lrows);
      d_rrows = upload(rrows, 1, &b_rrows);
    } else {
      d_lk = upload(c.lk, 0, &b_lk);
      d_rk = upload(c.rk, 0, &b_rk);
      if (!f.null_pay) {
        d_lp = upload(lp, 0, &b_lp);
        d_rp = upload(rp, 0, &b_rp);
      }
    }
    g_largest = std::max(g_largest, g_bytes);

    /* build */
    table.poison();
    err.poison();
    CHECK(hipMemcpy(err.p(), &f.preset, 4, hipMemcpyHostToDevice));
    dj::join_table_init((int64_t*)table.p(), nslots, nullptr);
    if (f.pairs)
      dj::join_build_pairs(d_lrows, ln, (int64_t*)table.p(), nslots, err.p(), nullptr);
    else
      dj::join_build(d_lk, d_lp, ln, (int64_t*)table.p(), nslots, err.p(), nullptr);
    CHECK(hipDeviceSynchronize());
    (*runs)++;
    bad += check_table(c, f, table.read(), nslots);
    const int word = err.read()[0], want_word = f.preset | (ref.neg1_build ? 1 : 0);
    if (word != want_word) fail(f, 0, 0, "error word after the build (got, expected)", word, want_word);
    if (!table.guards_ok()) fail(f, 0, 0, "guard around the table written by the build", 0, 0);
    if (!err.guards_ok()) fail(f, 0, 0, "guard around the error word written", 0, 0);

    /* probes */
    for (int64_t start : kStarts) {
      std::vector<int64_t> caps = {0, start + kCut, start + ref.total - 1, start + ref.total};
      std::sort(caps.begin(), caps.end());
      caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
      for (int64_t cap : caps) {
        if (cap < 0) continue;
        for (auto& o : out) o.poison();
        counter.poison();
        CHECK(hipMemcpy(counter.p(), &start, 8, hipMemcpyHostToDevice));
        if (f.pairs)
          dj::join_probe_pairs(d_rrows, rn, (const int64_t*)table.p(), nslots, out[0].p(),
                               out[1].p(), out[2].p(), out[3].p(), cap, counter.p(), nullptr);
        else
          dj::join_probe(d_rk, d_rp, rn, (const int64_t*)table.p(), nslots, out[0].p(),
                         out[1].p(), out[2].p(), out[3].p(), cap, counter.p(), nullptr);
        CHECK(hipDeviceSynchronize());
        (*runs)++;

        const int64_t got = counter.read()[0];
        if (got != start + ref.total)
          fail(f, start, cap, "counter (got, expected)", got, start + ref.total);
        const int64_t end = std::max(start, std::min(cap, start + ref.total));
        std::vector<int64_t> o[4];
        for (int k = 0; k < 4; k++) {
          o[k] = out[k].read();
          if (!all_poison(o[k].data(), (size_t)start * 8))
            fail(f, start, cap, "an output row before the start counter written (column)", k, 0);
          if (!all_poison(o[k].data() + end, (out_rows - (size_t)end) * 8))
            fail(f, start, cap, "an output row at or past cap, or past the matches, written (column)", k, 0);
          if (!out[k].guards_ok()) fail(f, start, cap, "guard around an output written (column)", k, 0);
        }
        if (!counter.guards_ok()) fail(f, start, cap, "guard around the counter written", 0, 0);
        std::vector<int64_t> pairs;
        pairs.reserve((size_t)(end - start));
        for (int64_t x = start; x < end; x++) {
          const int64_t i = row_of(f.null_pay, o[1][(size_t)x], 7, 3, ln);
          const int64_t j = row_of(f.null_pay, o[3][(size_t)x], 11, 5, rn);
          if (i < 0 || j < 0 || o[0][(size_t)x] != o[2][(size_t)x] ||
              c.lk[(size_t)i] != o[0][(size_t)x] || c.rk[(size_t)j] != o[0][(size_t)x] ||
              o[0][(size_t)x] == -1)
            fail(f, start, cap, "a written row is not in the reference (output row, out0)", x,
                 o[0][(size_t)x]);
          else
            pairs.push_back(i * rn + j);
        }
        std::sort(pairs.begin(), pairs.end());
        if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end())
          fail(f, start, cap, "a pair of rows written twice", 0, 0);
        if ((int64_t)pairs.size() != end - start)
          fail(f, start, cap, "reference rows written (got, expected)", (long long)pairs.size(),
               end - start);
      }
    }
    /* the probes leave the table and its guards alone */
    if (!table.guards_ok()) fail(f, 0, 0, "guard around the table written by a probe", 0, 0);
    if (f.pairs) {
      drop(b_lrows, lrows.size() + 1);
      drop(b_rrows, rrows.size() + 1);
    } else {
      drop(b_lk, c.lk.size());
      drop(b_rk, c.rk.size());
      if (!f.null_pay) {
        drop(b_lp, lp.size());
        drop(b_rp, rp.size());
      }
    }
  }
  table.release();
  for (auto& o : out) o.release();
  counter.release();
  err.release();
  return bad;
}

/* ---------------- neg1_cross_join cases ---------------- */

struct CrossCase {
  std::string name;
  std::vector<int64_t> lk, rk;
  int64_t n1 = 0, n2 = 0;
  bool want_trip = false, want_two_emit_trips = false;
};
/* n rows: `neg` of them -1, evenly spread from row `from` on, the rest the
 * keys the collect kernel must pass over */
static std::vector<int64_t> side(int64_t n, int64_t neg, int64_t from, uint64_t stream)
{
  const int64_t sp[] = {-2, 0, 4294967295LL, INT64_MIN};
  std::vector<int64_t> v((size_t)n);
  const int64_t room = n - from;
  for (int64_t i = 0, m = 0; i < n; i++) {
    if (i >= from && (i - from + 1) * neg / room > (i - from) * neg / room) {
      v[(size_t)i] = -1;
    } else {
      v[(size_t)i] = m % 13 < 4 ? sp[m % 13] : hkey(stream, (uint64_t)m);
      m++;
    }
  }
  return v;
}
static CrossCase cross(int64_t n1, int64_t n2)
{
  CrossCase c;
  c.name = "cross " + std::to_string(n1) + " x " + std::to_string(n2);
  c.n1 = n1;
  c.n2 = n2;
  c.want_two_emit_trips = n1 == 700;
  c.lk = side(n1 + 54, n1, 0, 17);
  c.rk = side(n2 + 71, n2, 0, 18);
  return c;
}

static bool cross_inputs_ok(const CrossCase& c)
{
  const int64_t T = (int64_t)g_sh.block * g_sh.grid_cap;
  int64_t n1 = 0, n2 = 0, first1 = -1, first2 = -1;
  bool others = true;
  for (const std::vector<int64_t>* v : {&c.lk, &c.rk}) {
    bool have[4] = {false, false, false, false};
    for (int64_t k : *v) {
      have[0] |= k == -2;
      have[1] |= k == 0;
      have[2] |= k == 4294967295LL;
      have[3] |= k == INT64_MIN;
    }
    others &= have[0] && have[1] && have[2] && have[3];
  }
  for (size_t i = 0; i < c.lk.size(); i++)
    if (c.lk[i] == -1 && n1++ == 0) first1 = (int64_t)i;
  for (size_t j = 0; j < c.rk.size(); j++)
    if (c.rk[j] == -1 && n2++ == 0) first2 = (int64_t)j;
  printf("inputs %s: ln=%zu rn=%zu, -1 rows %lld x %lld = %lld appended rows, one emit trip "
         "covers %lld\n",
         c.name.c_str(), c.lk.size(), c.rk.size(), (long long)n1, (long long)n2,
         (long long)(n1 * n2), (long long)T);
  if (n1 != c.n1 || n2 != c.n2 || !others) {
    printf("BAD TEST INPUTS: %s: wrong number of -1 rows, or a key to pass over is missing\n",
           c.name.c_str());
    return false;
  }
  if (c.want_two_emit_trips && n1 * n2 <= T) {
    printf("BAD TEST INPUTS: %s: the cross product fits one trip of the emit kernel\n",
           c.name.c_str());
    return false;
  }
  if (c.want_trip && (first1 < T || first2 < T)) {
    printf("BAD TEST INPUTS: %s: a -1 row lies in the collect kernel's first trip\n",
           c.name.c_str());
    return false;
  }
  return true;
}

static int run_cross_case(const CrossCase& c, int* runs)
{
  const int64_t ln = (int64_t)c.lk.size(), rn = (int64_t)c.rk.size();
  const int64_t total = c.n1 * c.n2;
  const size_t out_rows = (size_t)(kStarts[1] + total + kTail);
  int bad = 0;
  Guarded<int64_t> out[4], counter;
  for (auto& o : out) o.alloc(out_rows);
  counter.alloc(1);
  int64_t *b_lk, *b_rk, *b_lp, *b_rp;
  const int64_t* d_lk = upload(c.lk, 0, &b_lk);
  const int64_t* d_rk = upload(c.rk, 0, &b_rk);
  for (int null_pay = 0; null_pay < 2; null_pay++) {
    std::vector<int64_t> lp((size_t)ln), rp((size_t)rn);
    for (int64_t i = 0; i < ln; i++) lp[(size_t)i] = lpay_of(false, i);
    for (int64_t j = 0; j < rn; j++) rp[(size_t)j] = rpay_of(false, j);
    const int64_t* d_lp = upload(lp, 0, &b_lp);
    const int64_t* d_rp = upload(rp, 0, &b_rp);
    g_largest = std::max(g_largest, g_bytes);
    for (int64_t start : kStarts) {
      std::vector<int64_t> caps = {0, start + kCut, start + total - 1, start + total};
      std::sort(caps.begin(), caps.end());
      caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
      for (int64_t cap : caps) {
        if (cap < 0) continue;
        auto fail = [&](const char* what, long long a, long long b) {
          if (bad++ < 8)
            printf("  FAIL %s, start %lld cap %lld: %s (%lld, %lld)\n",
                   null_pay ? "null payloads" : "payloads", (long long)start, (long long)cap, what,
                   a, b);
        };
        for (auto& o : out) o.poison();
        counter.poison();
        CHECK(hipMemcpy(counter.p(), &start, 8, hipMemcpyHostToDevice));
        dj::neg1_cross_join(d_lk, null_pay ? nullptr : d_lp, ln, d_rk, null_pay ? nullptr : d_rp,
                            rn, out[0].p(), out[1].p(), out[2].p(), out[3].p(), cap, counter.p(),
                            nullptr);
        CHECK(hipDeviceSynchronize());
        (*runs)++;
        const int64_t got = counter.read()[0];
        if (got != start + total) fail("counter (got, expected)", got, start + total);
        const int64_t end = std::max(start, std::min(cap, start + total));
        std::vector<int64_t> o[4];
        for (int k = 0; k < 4; k++) {
          o[k] = out[k].read();
          if (!all_poison(o[k].data(), (size_t)start * 8))
            fail("an output row before the start counter written (column)", k, 0);
          if (!all_poison(o[k].data() + end, (out_rows - (size_t)end) * 8))
            fail("an output row at or past cap, or past the product, written (column)", k, 0);
          if (!out[k].guards_ok()) fail("guard around an output written (column)", k, 0);
        }
        if (!counter.guards_ok()) fail("guard around the counter written", 0, 0);
        std::vector<int64_t> pairs;
        pairs.reserve((size_t)(end - start));
        for (int64_t x = start; x < end; x++) {
          const int64_t i = row_of(null_pay, o[1][(size_t)x], 7, 3, ln);
          const int64_t j = row_of(null_pay, o[3][(size_t)x], 11, 5, rn);
          if (i < 0 || j < 0 || o[0][(size_t)x] != -1 || o[2][(size_t)x] != -1 ||
              c.lk[(size_t)i] != -1 || c.rk[(size_t)j] != -1)
            fail("a written row is not in the cross product (output row, out1)", x,
                 o[1][(size_t)x]);
          else
            pairs.push_back(i * rn + j);
        }
        std::sort(pairs.begin(), pairs.end());
        if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end())
          fail("a pair of -1 rows written twice", 0, 0);
        if ((int64_t)pairs.size() != end - start)
          fail("rows of the cross product written (got, expected)", (long long)pairs.size(),
               end - start);
      }
    }
    drop(b_lp, lp.size());
    drop(b_rp, rp.size());
  }
  drop(b_lk, c.lk.size());
  drop(b_rk, c.rk.size());
  for (auto& o : out) o.release();
  counter.release();
  return bad;
}

/* ---------------- join_table_slots ---------------- */

static bool table_slots_ok()
{
  std::vector<int64_t> lns = {0, 1, 2, 3, 4};
  for (int k = 1; k <= 21; k++)
    for (int64_t d = -1; d <= 1; d++) lns.push_back(((int64_t)1 << k) + d);
  for (int64_t ln : lns) {
    const int64_t s = dj::join_table_slots(ln);
    const bool pow2 = s > 0 && (s & (s - 1)) == 0;
    if (!pow2 || s < 2 * ln + 1 || (s > 1 && s / 2 >= 2 * ln + 1)) {
      printf("FAIL join_table_slots(%lld) = %lld: not the smallest power of two >= 2 ln + 1\n",
             (long long)ln, (long long)s);
      return false;
    }
  }
  printf("join_table_slots: ok\n");
  return true;
}

/* ---------------- main ---------------- */

struct Entry {
  const char* set;
  std::function<JoinCase()> join;
  std::function<CrossCase()> cross;
};

static std::vector<Entry> entries()
{
  std::vector<Entry> e;
  const int64_t sizes[] = {1, 63, 64, 65, 255, 256, 257};
  for (int64_t ln : sizes)
    for (int64_t rn : sizes) e.push_back({"sizes", [=] { return sized(ln, rn); }, nullptr});
  e.push_back({"edges", wrap_case, nullptr});
  e.push_back({"edges", hot_case, nullptr});
  e.push_back({"edges", special_case, nullptr});
  e.push_back({"edges", [] { return neg1_probe_case(false); }, nullptr});
  e.push_back({"edges", [] { return neg1_probe_case(true); }, nullptr});
  e.push_back({"edges", trip_case, nullptr});
  const int64_t crosses[][2] = {{0, 5}, {5, 0}, {1, 1}, {40, 25}, {700, 800}};
  for (auto& x : crosses) {
    const int64_t n1 = x[0], n2 = x[1];
    e.push_back({"neg1", nullptr, [=] { return cross(n1, n2); }});
  }
  e.push_back({"neg1", nullptr, [] {
                 const int64_t T = (int64_t)g_sh.block * g_sh.grid_cap;
                 CrossCase c;
                 c.name = "cross 3 x 4 past the collect kernel's first trip";
                 c.n1 = 3;
                 c.n2 = 4;
                 c.want_trip = true;
                 c.lk = side(T + 50, 3, T + 2, 17);
                 c.rk = side(T + 30, 4, T + 1, 18);
                 return c;
               }});
  return e;
}

int main(int argc, char** argv)
{
  bool inputs_only = false;
  std::string set;
  for (int i = 1; i < argc; i++) {
    if (strcmp(argv[i], "--inputs-only") == 0) {
      inputs_only = true;
    } else if (strcmp(argv[i], "--set") == 0 && i + 1 < argc) {
      set = argv[++i];
    } else {
      printf("usage: table_join_check [--inputs-only] [--set sizes|edges|neg1]\n");
      return 2;
    }
  }
  g_sh = dj::table_join_shape();
  printf("shape: block %d, grid cap %d, one trip covers %lld rows\n", g_sh.block, g_sh.grid_cap,
         (long long)g_sh.block * g_sh.grid_cap);
  if (!table_slots_ok()) return 1;

  JoinSituations sit;
  int bad = 0, ncases = 0, runs = 0;
  double slowest_ms = 0;
  std::string slowest;
  for (const Entry& e : entries()) {
    if (!set.empty() && set != e.set) continue;
    const auto t0 = std::chrono::steady_clock::now();
    std::string name;
    int b = 0;
    /* every input check comes before the case's launches */
    if (e.join) {
      const JoinCase c = e.join();
      const Ref r = reference(c);
      name = c.name;
      if (!inputs_ok(c, r, sit)) return 2;
      if (!inputs_only) b = run_join_case(c, r, &runs);
    } else {
      const CrossCase c = e.cross();
      name = c.name;
      if (!cross_inputs_ok(c)) return 2;
      if (!inputs_only) b = run_cross_case(c, &runs);
    }
    ncases++;
    if (!inputs_only) {
      const double ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (ms > slowest_ms) {
        slowest_ms = ms;
        slowest = name;
      }
      printf("%s: %.0f ms: %s\n", name.c_str(), ms, b ? "FAILED" : "ok");
      bad += b;
    }
  }
  if (ncases == 0) {
    printf("no such set: %s\n", set.c_str());
    return 2;
  }
  if (set.empty() && (sit.cut_inside < 2 || sit.last_cut_inside < 2)) {
    printf("BAD TEST INPUTS: fewer than two one-wave cases whose cut caps fall inside a group\n");
    return 2;
  }
  if (bad) {
    printf("TABLE JOIN FAILED: %d checks\n", bad);
    return 1;
  }
  if (inputs_only) {
    printf("TABLE JOIN INPUTS OK (%d cases)\n", ncases);
  } else {
    printf("%d launcher calls; slowest case %.0f ms (%s, inputs and host checks included), "
           "largest device footprint %.1f MB\n",
           runs, slowest_ms, slowest.c_str(), (double)g_largest / 1e6);
    printf("TABLE JOIN OK (%d cases)\n", ncases);
  }
  return 0;
}
