/*
 * host_table.hpp — the host side of the *_loopback programs: tables as plain
 * vectors with validity, their upload and read-back, an order-insensitive row
 * hash over every value and validity bit, the generator of the global test
 * tables and a host join of every kind to compare against.
 *
 * With HOST_TABLE_NO_MASKS defined only the mask-free upload helpers remain
 * (str_of, device_fixed, device_strings), which need nothing newer than the
 * mask-free dj_cudf_types.hpp.
 */
#pragma once

#include "check.hpp"
#include "dj_cudf_types.hpp"

#include "../../distributed_join_amd/csrc/dj_rng.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

/* string of a row id: 0-8 lowercase bytes */
static inline std::string str_of(uint64_t id)
{
  const int len = (int)(id % 9);
  std::string s((size_t)len, 'a');
  for (int k = 0; k < len; k++) s[(size_t)k] = (char)('a' + dj_mix64(id * 16 + (uint64_t)k) % 26);
  return s;
}

static inline std::unique_ptr<cudf::column> device_fixed(cudf::type_id type, const void* data,
                                                         int64_t rows, int width)
{
  auto col = std::make_unique<cudf::column>(cudf::data_type(type), (cudf::size_type)rows);
  if (rows) CHECK(hipMemcpy(col->head(), data, (size_t)rows * width, hipMemcpyHostToDevice));
  return col;
}

static inline std::unique_ptr<cudf::column> device_strings(const std::vector<std::string>& s)
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

#ifndef HOST_TABLE_NO_MASKS

#include "distributed_join.hpp" /* join_kind */

/* ---------------- host tables with validity ---------------- */

struct HCol {
  cudf::type_id type;
  std::vector<int64_t> v;      // fixed-width values, sign-extended (garbage under a null)
  std::vector<std::string> s;  // STRING values (garbage under a null)
  std::vector<uint8_t> valid;
  bool mask;  // carries a mask on the device
};
using HTable = std::vector<HCol>;

static inline int width_of(cudf::type_id t) { return cudf::size_of(cudf::data_type(t)); }

static inline uint64_t fold(const std::string& s)
{
  uint64_t h = 1469598103934665603ull ^ s.size();
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

constexpr uint64_t kNullCell = 0x6e756c6cull;

static inline uint64_t cell_hash(const HCol& c, size_t i)
{
  if (!c.valid[i]) return kNullCell;
  return c.type == cudf::type_id::STRING ? fold(c.s[i]) : dj_mix64((uint64_t)c.v[i]);
}

/* hash of row i over columns [c0, c1): values and validity */
static inline uint64_t row_hash(const HTable& t, size_t c0, size_t c1, size_t i)
{
  uint64_t h = 0x12345;
  for (size_t c = c0; c < c1; c++) h = dj_mix64(h ^ cell_hash(t[c], i)) + (c - c0);
  return h;
}

/* row_hash of a row of ncols null cells: the right side of an unmatched row */
static inline uint64_t null_row_hash(size_t ncols)
{
  uint64_t h = 0x12345;
  for (size_t c = 0; c < ncols; c++) h = dj_mix64(h ^ kNullCell) + c;
  return h;
}

static inline size_t rows_of(const HTable& t) { return t.empty() ? 0 : t[0].valid.size(); }

static inline std::unique_ptr<cudf::column> to_device(const HCol& c)
{
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
  return col;
}

static inline std::unique_ptr<cudf::table> to_device(const HTable& t)
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (const HCol& c : t) cols.push_back(to_device(c));
  return std::make_unique<cudf::table>(std::move(cols));
}

/* `ci` only names the column in a failure message */
static inline HCol from_device(const cudf::column& col, int ci = 0)
{
  const size_t n = (size_t)col.size();
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
  return c;
}

static inline HTable from_device(const cudf::table& t)
{
  HTable out;
  for (cudf::size_type ci = 0; ci < t.num_columns(); ci++)
    out.push_back(from_device(t.get_column(ci), ci));
  return out;
}

/* ---------------- the global test tables ---------------- */

enum RightShape { kRightPlain, kRightKeysOnly, kRightWide };

/* rows [row0, row0+rows) of a global table:
 *   left : key INT64, pay INT32, str STRING
 *   right: key INT64, pay INT64, pay2 INT16 (+ two more INT64 when wide;
 *          the key alone when keys_only)
 * Keys draw from `distinct` values. Payloads are nullable; keys only when
 * null_keys. The value under a null key is key id 1 or -1: both would match
 * valid keys if they were compared. */
static inline HTable host_table(int64_t row0, int64_t rows, bool left, bool null_keys,
                                int64_t distinct, int key_null_every,
                                RightShape shape = kRightPlain)
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
  if (!left && shape == kRightKeysOnly) t.resize(1);
  if (!left && shape == kRightWide) {  // three 8-byte payloads behind the key
    t[2].type = cudf::type_id::INT64;
    HCol c = t[1];
    for (auto& x : c.v) x = x * 5;
    t.push_back(c);
  }
  return t;
}

/* the rank that may pass its column 1 without a mask (all rows valid there) */
constexpr int kMasklessRank = 1;
enum Maskless { kMasklessNone, kMasklessLeft, kMasklessRight };

/* one pair of global tables over G ranks of R rows each */
struct TablePair {
  int G;
  int64_t R;
  bool null_keys;
  int64_t distinct, right_distinct;  // key values on the left, on the right
  int every;                         // one key in `every` is null (when null_keys)
  Maskless maskless = kMasklessNone;  // the side whose column 1 kMasklessRank passes maskless
  RightShape shape = kRightPlain;
  /* false: the right key keeps its mask but marks no row null (the values
   * that were under its nulls, 1 and -1, become ordinary keys), so that a
   * null left key has no partner anywhere */
  bool right_nulls = true;

  TablePair(int G_, int64_t R_, bool null_keys_)
    : G(G_), R(R_), null_keys(null_keys_), distinct(std::max<int64_t>(4, G_ * R_ / 3)),
      right_distinct(distinct), every(G_ * R_ > 100 ? 16 : 3)
  {
  }
};

static inline HTable rank_table(const TablePair& p, int r, bool left)
{
  HTable t = host_table(r * p.R, p.R, left, p.null_keys, left ? p.distinct : p.right_distinct,
                        p.every, p.shape);
  if (!left && !p.right_nulls) t[0].valid.assign(t[0].valid.size(), 1);
  if (r == kMasklessRank && p.maskless == (left ? kMasklessLeft : kMasklessRight)) {
    t[1].mask = false;
    t[1].valid.assign(t[1].valid.size(), 1);
  }
  return t;
}

static inline HTable global_table(const TablePair& p, bool left)
{
  HTable all;
  for (int r = 0; r < p.G; r++) {
    HTable t = rank_table(p, r, left);
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

/* ---------------- host join ---------------- */

static inline std::string key_code(const HTable& t, size_t i, size_t col = 0)
{
  if (!t[col].valid[i]) return "n";
  return "v" + std::to_string(t[col].v[i]);
}

/* host join of `kind` on column 0, null == null: (rows, order-insensitive sum) */
static inline void host_join(join_kind kind, const HTable& l, const HTable& r, long long* rows,
                             uint64_t* sum)
{
  std::map<std::string, std::vector<size_t>> idx;
  for (size_t j = 0; j < rows_of(r); j++) idx[key_code(r, j)].push_back(j);
  const bool pairs = kind == join_kind::INNER || kind == join_kind::LEFT;
  long long n = 0;
  uint64_t s = 0;
  const uint64_t pad = null_row_hash(r.size());
  for (size_t i = 0; i < rows_of(l); i++) {
    auto it = idx.find(key_code(l, i));
    const bool hit = it != idx.end();
    const uint64_t lh = row_hash(l, 0, l.size(), i);
    if (pairs) {
      if (!hit) {
        if (kind == join_kind::INNER) continue;
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

/* the same (rows, sum) of a join's output, whose first nl columns are the
 * left table's; an INNER row must carry equal keys */
static inline void output_sum(join_kind kind, const HTable& out, size_t nl, long long* rows,
                              uint64_t* sum)
{
  const bool pairs = kind == join_kind::INNER || kind == join_kind::LEFT;
  uint64_t s = 0;
  for (size_t i = 0; i < rows_of(out); i++) {
    if (kind == join_kind::INNER && key_code(out, i) != key_code(out, i, nl))
      FAIL("JOIN ROW WITH UNEQUAL KEYS");
    const uint64_t lh = row_hash(out, 0, nl, i);
    s += pairs ? dj_mix64(lh ^ dj_mix64(row_hash(out, nl, out.size(), i))) : dj_mix64(lh);
  }
  *rows = (long long)rows_of(out);
  *sum = s;
}

#endif /* HOST_TABLE_NO_MASKS */
