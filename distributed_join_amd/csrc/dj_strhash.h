/*
 * dj_strhash.h — hash spec for STRING key columns, shared by host and device.
 *
 * The reference forwards STRING key columns to cudf::hash_partition and
 * cudf::inner_join; here a STRING key row is reduced to a 64-bit value that
 * enters the fused key chain of composite keys (dj_hash.h "STRING and
 * composite keys"), and a byte-exact compare after the join drops the
 * collisions. The spec:
 *
 *   dj_murmur3_bytes(p, len, seed) = MurmurHash3_x86_32 over p[0..len):
 *       little-endian 4-byte blocks, the 1-3 byte tail, h ^= len, fmix32
 *   dj_string_key64(p, len)        = murmur3(p, len, 0)
 *                                  | (uint64)murmur3(p, len, 0x9747B28C) << 32
 *
 * Both seeds appear in tests/golden/murmur3_public_vectors.json, so each half
 * is pinned to published vectors (tests/test_strhash_cpu.py), not to this
 * code. Only p[0..len) is touched; len == 0 is safe with any p.
 *
 * Plain C99; compiles under gcc/g++/hipcc.
 */
#ifndef DJ_STRHASH_H
#define DJ_STRHASH_H

#include <stdint.h>

#include "dj_hash.h"

#define DJ_STRKEY_SEED_LO 0u
#define DJ_STRKEY_SEED_HI 0x9747B28Cu

/* one 4-byte block into the running state */
DJ_HASH_HD uint32_t dj_murmur3_block(uint32_t h1, uint32_t k1)
{
  k1 *= 0xCC9E2D51u;
  k1 = dj_rotl32(k1, 15);
  k1 *= 0x1B873593u;
  h1 ^= k1;
  h1 = dj_rotl32(h1, 13);
  return h1 * 5 + 0xE6546B64u;
}

/* the 1-3 byte tail (already packed little-endian into k1) */
DJ_HASH_HD uint32_t dj_murmur3_tail(uint32_t h1, uint32_t k1)
{
  k1 *= 0xCC9E2D51u;
  k1 = dj_rotl32(k1, 15);
  k1 *= 0x1B873593u;
  return h1 ^ k1;
}

DJ_HASH_HD uint32_t dj_murmur3_bytes(const uint8_t* p, int32_t len, uint32_t seed)
{
  uint32_t h1           = seed;
  const int32_t nblocks = len / 4;
  for (int32_t i = 0; i < nblocks; i++) {
    const uint8_t* b = p + 4 * i;
    uint32_t k1 = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) |
                  ((uint32_t)b[3] << 24);
    h1 = dj_murmur3_block(h1, k1);
  }
  const int32_t rem = len & 3;
  if (rem) {
    const uint8_t* t = p + 4 * nblocks;
    uint32_t k1      = t[0];
    if (rem >= 2) k1 |= (uint32_t)t[1] << 8;
    if (rem >= 3) k1 |= (uint32_t)t[2] << 16;
    h1 = dj_murmur3_tail(h1, k1);
  }
  h1 ^= (uint32_t)len;
  return dj_fmix32(h1);
}

DJ_HASH_HD uint64_t dj_string_key64(const uint8_t* p, int32_t len)
{
  return (uint64_t)dj_murmur3_bytes(p, len, DJ_STRKEY_SEED_LO) |
         ((uint64_t)dj_murmur3_bytes(p, len, DJ_STRKEY_SEED_HI) << 32);
}

#endif /* DJ_STRHASH_H */
