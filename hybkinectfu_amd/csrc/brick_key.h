// brick_key.h -- the brick store's key: a world brick coordinate packed into one 64-bit word (brickstore.hip; no reference counterpart).
// A world brick coordinate is origin_vox / 8 + brick index: where a brick of the window lies in the bricks of the first cube.  Each component is a
// signed 21-bit field, [-2^20, 2^20): x at bits 0-20, y at bits 21-41, z at bits 42-62.  Bit 63 is never set, so no key equals KF_BRICK_KEY_EMPTY,
// the word of a free entry of the hash table.  Host and device: the CPU test compiles this header too (tests/brick_key_main.cpp).
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

#define KF_BRICK_KEY_BITS 21
#define KF_BRICK_KEY_MIN (-(1 << (KF_BRICK_KEY_BITS - 1)))        // -2^20, inclusive
#define KF_BRICK_KEY_MAX (1 << (KF_BRICK_KEY_BITS - 1))           //  2^20, exclusive
#define KF_BRICK_KEY_EMPTY 0xFFFFFFFFFFFFFFFFull

__host__ __device__ static inline bool kf_brick_key_in_range(int64_t c) { return c >= KF_BRICK_KEY_MIN && c < KF_BRICK_KEY_MAX; }

// does every brick of a window of nb bricks per axis that stands at origin_vox (voxels, multiples of 8) have a key?
__host__ __device__ static inline bool kf_window_in_key_range(const int32_t origin_vox[3], int nb) {
  for (int k = 0; k < 3; ++k) {
    const int64_t b = origin_vox[k] / 8;
    if (!kf_brick_key_in_range(b) || !kf_brick_key_in_range(b + nb - 1)) return false;
  }
  return true;
}

__host__ __device__ static inline unsigned long long kf_brick_key_pack(int32_t x, int32_t y, int32_t z) {
  const unsigned long long m = (1ull << KF_BRICK_KEY_BITS) - 1ull;
  return ((unsigned long long)(uint32_t)x & m) | (((unsigned long long)(uint32_t)y & m) << KF_BRICK_KEY_BITS) |
         (((unsigned long long)(uint32_t)z & m) << (2 * KF_BRICK_KEY_BITS));
}

// the sign comes back by subtracting 2^21 from a field whose top bit is set (no shift of a negative value)
__host__ __device__ static inline void kf_brick_key_unpack(unsigned long long key, int32_t out[3]) {
  const unsigned long long m = (1ull << KF_BRICK_KEY_BITS) - 1ull;
  for (int k = 0; k < 3; ++k) {
    const int32_t f = (int32_t)((key >> (k * KF_BRICK_KEY_BITS)) & m);
    out[k] = f >= KF_BRICK_KEY_MAX ? f - (1 << KF_BRICK_KEY_BITS) : f;
  }
}

// where a key's probe sequence starts in a table of `mask + 1` entries (a power of two): the 64-bit finaliser of MurmurHash3 (public domain)
__host__ __device__ static inline uint32_t kf_brick_key_hash(unsigned long long key, uint32_t mask) {
  key ^= key >> 33; key *= 0xFF51AFD7ED558CCDull; key ^= key >> 33; key *= 0xC4CEB9FE1A85EC53ull; key ^= key >> 33;
  return (uint32_t)key & mask;
}
