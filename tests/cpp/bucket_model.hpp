/*
 * bucket_model.hpp — the host's own statement of the engine's bucket bit
 * fields, shared by the *_check programs. It restates the comment at
 * groupA_of / subF_of in dj_kernels.hip and deliberately takes nothing from
 * the product but the two hashes: a check that read the layout from the
 * kernels' header would agree with whatever they do.
 *
 *   m       = dj_mix64(key)
 *   groupA  = (m >> 40) & (PA - 1)                       pass-A group
 *   subF    = (m >> 32) & (F - 1)                        F <= 256
 *           = (m >> 32) & 255 | ((m >> 50) & (F/256 - 1)) << 8   F > 256
 *   bucket  = groupA * F + subF
 *
 * Host only: nothing here touches the device.
 */
#pragma once

#include "dj_hash.h"
#include "dj_rng.h"

#include <cstddef>
#include <cstdint>

static inline uint32_t group_of(int64_t key, int PA)
{
  return (uint32_t)(dj_mix64((uint64_t)key) >> 40) & (uint32_t)(PA - 1);
}
static inline uint32_t sub_of(int64_t key, int F)
{
  const uint64_t m = dj_mix64((uint64_t)key);
  if (F <= 256) return (uint32_t)(m >> 32) & (uint32_t)(F - 1);
  return ((uint32_t)(m >> 32) & 255u) | (((uint32_t)(m >> 50) & (uint32_t)((F >> 8) - 1)) << 8);
}
static inline uint32_t bucket_of(int64_t key, int PA, int F)
{
  return group_of(key, PA) * (uint32_t)F + sub_of(key, F);
}
/* slice of the fused wire partition: (rank/batch partition) * PA + groupA */
static inline uint32_t slice_of_key(int64_t key, int npr, uint32_t seed, int PA)
{
  return (dj_murmur3_int64(key, seed) % (uint32_t)npr) * (uint32_t)PA + group_of(key, PA);
}

/* distinct keys: an odd multiplier is a bijection of the index */
static inline int64_t hkey(uint64_t stream, uint64_t i)
{
  return (int64_t)(((stream << 40) + i + 1) * 0x9E3779B97F4A7C15ULL);
}

/* every output is filled with kPoison before a run and allocated with a guard
 * behind it: kGuardRows rows (or column elements), kGuardWords words */
constexpr int kPoison = 0xEE;
constexpr int kGuardRows = 64, kGuardWords = 16;

static inline bool all_poison(const void* p, size_t bytes)
{
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < bytes; i++)
    if (b[i] != kPoison) return false;
  return true;
}
