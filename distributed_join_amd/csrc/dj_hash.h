/*
 * dj_hash.h — row-hash spec for partition placement.
 *
 * The reference delegates partition hashing to cudf::hash_partition with
 * cudf::hash_id::HASH_MURMUR3 (seed 12345678 intra-node, 87654321 for the
 * inter-node stage — /root/reference/src/distributed_join.cpp:160,211-226;
 * shuffle_on.cpp:59-60). No reference test pins MurmurHash3 placement
 * (placement is parity-unpinned; the only placement test,
 * test_shuffle_on.cpp:78-83, uses HASH_IDENTITY). Our spec therefore is:
 *
 *   hash(int64 key) = MurmurHash3_32(little-endian 8 bytes of key, seed)
 *   partition(key)  = hash % nparts
 *   HASH_IDENTITY   : hash = (uint32_t)key  (cudf IdentityHash truncates),
 *                     partition = hash % nparts
 *
 * The global join result is partition-invariant (every placement that sends
 * equal keys to the same rank yields the same join), so end-to-end parity
 * with the oracle does not depend on this choice; shuffle placement parity is
 * pinned to THIS spec by our own tests.
 *
 * STRING and composite keys (our spec, parity-unpinned like the above): the
 * key tuple is fused into one 64-bit value by the chain
 *
 *   h = 0x9e3779b97f4a7c15;  for each key column c:  h = dj_mix64(h ^ v_c)
 *
 * where v_c is the integer value of an integer-rep column as int64 (signed
 * reps sign-extended, UINT8/UINT16/UINT32/BOOL8 zero-extended, UINT64
 * reinterpreted — the same widening a single narrow key gets before
 * dj_row_hash) and dj_string_key64(row bytes) of a STRING column (dj_strhash.h: two
 * MurmurHash3_x86_32 halves, seeds 0 and 0x9747B28C). Placement is then
 * dj_murmur3_int64(fused, seed) % nparts, exactly as for an int64 key. A
 * single STRING key takes the same chain. The join matches on the fused
 * value and drops collisions by comparing the real columns (strings: length,
 * then bytes). HASH_IDENTITY has no STRING form (cuDF has none either).
 *
 * Null keys: a valid row of a nullable key column places exactly as it would
 * without the mask (so a mask that marks no row null changes nothing). A null
 * key element contributes the element hash 0xFFFFFFFF (cuDF's row-hasher
 * convention for a null element), whatever is stored under it:
 *   - single integer key, HASH_MURMUR3 and HASH_IDENTITY alike:
 *       hash = 0xFFFFFFFF, partition = 0xFFFFFFFF % nparts;
 *   - in the fused chain above: v_c = 0xFFFFFFFF for a null element of
 *     column c (integer-rep or STRING), the other columns as usual.
 * The join treats null as equal to null (cudf::inner_join's default
 * null_equality::EQUAL, which the reference call relies on): the tuple
 * filter compares validity first and values only where both are valid.
 *
 * Plain C99; compiles under gcc/g++/hipcc.
 */
#ifndef DJ_HASH_H
#define DJ_HASH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define DJ_HASH_HD __host__ __device__ static inline
#else
#define DJ_HASH_HD static inline
#endif

#define DJ_HASH_MURMUR3 0
#define DJ_HASH_IDENTITY 1

/* default seed matches cudf::DEFAULT_HASH_SEED = 0 */
#define DJ_DEFAULT_HASH_SEED 0u
/* seeds the reference passes on the hot path (distributed_join.cpp:160,211) */
#define DJ_SEED_INTRA 12345678u
#define DJ_SEED_INTER 87654321u

DJ_HASH_HD uint32_t dj_rotl32(uint32_t x, int8_t r) { return (x << r) | (x >> (32 - r)); }

DJ_HASH_HD uint32_t dj_fmix32(uint32_t h)
{
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

/* MurmurHash3_32 (x86_32) of one int64 key, treated as 8 little-endian bytes */
DJ_HASH_HD uint32_t dj_murmur3_int64(int64_t key, uint32_t seed)
{
  const uint32_t c1 = 0xCC9E2D51u;
  const uint32_t c2 = 0x1B873593u;
  uint32_t h1       = seed;
  uint64_t u        = (uint64_t)key;
  uint32_t blocks[2];
  blocks[0] = (uint32_t)(u & 0xFFFFFFFFu);
  blocks[1] = (uint32_t)(u >> 32);
  for (int i = 0; i < 2; i++) {
    uint32_t k1 = blocks[i];
    k1 *= c1;
    k1 = dj_rotl32(k1, 15);
    k1 *= c2;
    h1 ^= k1;
    h1 = dj_rotl32(h1, 13);
    h1 = h1 * 5 + 0xE6546B64u;
  }
  /* len = 8, no tail */
  h1 ^= 8u;
  return dj_fmix32(h1);
}

DJ_HASH_HD uint32_t dj_identity_int64(int64_t key, uint32_t seed)
{
  (void)seed;
  return (uint32_t)((uint64_t)key & 0xFFFFFFFFu);
}

DJ_HASH_HD uint32_t dj_row_hash(int64_t key, int hash_fn, uint32_t seed)
{
  return hash_fn == DJ_HASH_IDENTITY ? dj_identity_int64(key, seed)
                                     : dj_murmur3_int64(key, seed);
}

#endif /* DJ_HASH_H */
