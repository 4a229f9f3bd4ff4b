// rigid_keys.h -- the host side of merging a map under a rigid transform (resample.hip, kf_merge_brick_store_rigid; no reference counterpart): is the
// transform one, which destination bricks can a source map reach, and where does a destination brick's corner voxel lie in the source; and what every entry
// point that reads a source map through a table of its own (resample.hip, halve.hip, align.hip) asks of the map's keys: kf_source_keys_table.  Plain host C++,
// fp64: the library and the stand-alone test program (tests/map_resample_main.cpp) both include it.
//
// xf is a row-major 3x4 [R | t]: source world -> destination world, in voxels.  World voxel g has its centre at g + 1/2, so a source position s (voxel
// index units) lies at d = R (s + 1/2) + t - 1/2 in the destination, and a destination voxel d at s = R^T (d + 1/2 - t) - 1/2 in the source.
#pragma once
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "brick_key.h"
#include "brick_keys_unique.h"

#define KF_RIGID_ORTHO_TOL 1e-5      // max |R^T R - I|: a rotation stored in fp32 is orthonormal to a few 1e-7; the rest is room for an accumulated pose

// all 12 values finite, max |R^T R - I| <= KF_RIGID_ORTHO_TOL, det R > 0 (a reflection is no rigid motion)
static inline bool kf_rigid_valid(const double* xf) {
  if (!xf) return false;
  for (int i = 0; i < 12; ++i) if (!isfinite(xf[i])) return false;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double g = xf[a] * xf[b] + xf[4 + a] * xf[4 + b] + xf[8 + a] * xf[8 + b];   // (R^T R)[a][b]: columns a and b
      if (!(fabs(g - (a == b ? 1.0 : 0.0)) <= KF_RIGID_ORTHO_TOL)) return false;
    }
  const double det = xf[0] * (xf[5] * xf[10] - xf[6] * xf[9]) - xf[1] * (xf[4] * xf[10] - xf[6] * xf[8]) + xf[2] * (xf[4] * xf[9] - xf[5] * xf[8]);
  return det > 0.0;
}

// The source position of destination brick K's voxel (0, 0, 0), split into an integer and a fraction in [0, 1):
//   a = 8 K + 0.5 - t;  c_j = ((R[0][j] a_0 + R[1][j] a_1) + R[2][j] a_2) - 0.5;  ib = floor(c);  fb = (float)(c - ib), and a fraction that rounds to 1.0f
// moves into the integer (ib + 1, 0.f).  False when an ib does not fit 31 bits: such a brick lies nowhere near any key.
static inline bool kf_rigid_brick_base(const double* xf, const int32_t K[3], int32_t ib[3], float fb[3]) {
  const double a0 = 8.0 * K[0] + 0.5 - xf[3], a1 = 8.0 * K[1] + 0.5 - xf[7], a2 = 8.0 * K[2] + 0.5 - xf[11];
  for (int j = 0; j < 3; ++j) {
    const double c = ((xf[j] * a0 + xf[4 + j] * a1) + xf[8 + j] * a2) - 0.5;
    const double fl = floor(c);
    if (!(fl >= -1073741824.0 && fl < 1073741824.0)) return false;
    ib[j] = (int32_t)fl;
    fb[j] = (float)(c - fl);
    if (fb[j] == 1.0f) { ib[j] += 1; fb[j] = 0.f; }
  }
  return true;
}

// a key as one word that sorts by (z, y, x): each component biased by 2^20 into 21 bits
static inline uint64_t kf_rigid_order_word(int64_t x, int64_t y, int64_t z) {
  return ((uint64_t)(z - KF_BRICK_KEY_MIN) << (2 * KF_BRICK_KEY_BITS)) | ((uint64_t)(y - KF_BRICK_KEY_MIN) << KF_BRICK_KEY_BITS) | (uint64_t)(x - KF_BRICK_KEY_MIN);
}

// The destination bricks a source map can reach.  A destination voxel draws on the source voxels floor(s) and floor(s) + 1 per axis, so it can draw on
// source brick k only when s lies in [8k - 1, 8k + 8)^3.  The 8 corners p of that box map to d_i = (((R[i][0] p_0 + R[i][1] p_1) + R[i][2] p_2) + t_i) - 0.5
// with p = s + 0.5; every destination brick (>> 3) the box floor(min d) .. ceil(max d) touches is a candidate.  Unique, sorted by (z, y, x); the first
// `cap` are written (out_keys may be NULL with cap 0).  Returns the number of candidates, or -1: a NULL pointer (keys with count > 0, xf), no valid
// transform, a candidate outside the key range [-2^20, 2^20).  Over-inclusion is harmless -- such a brick resamples to nothing --, under-inclusion a bug.
static inline int64_t kf_rigid_candidates(uint32_t count, const int32_t* keys, const double* xf, std::vector<uint64_t>& words) {
  words.clear();
  if ((count && !keys) || !kf_rigid_valid(xf)) return -1;
  for (uint32_t e = 0; e < count; ++e) {
    double lo[3], hi[3];
    for (int corner = 0; corner < 8; ++corner) {
      double p[3];
      for (int j = 0; j < 3; ++j) p[j] = 8.0 * keys[3 * (size_t)e + j] + (((corner >> j) & 1) ? 8.0 : -1.0) + 0.5;
      for (int i = 0; i < 3; ++i) {
        const double d = (((xf[4 * i] * p[0] + xf[4 * i + 1] * p[1]) + xf[4 * i + 2] * p[2]) + xf[4 * i + 3]) - 0.5;
        if (corner == 0 || d < lo[i]) lo[i] = d;
        if (corner == 0 || d > hi[i]) hi[i] = d;
      }
    }
    int64_t b0[3], b1[3];                                     // bricks, inclusive
    for (int i = 0; i < 3; ++i) {
      const double f = floor(lo[i]), c = ceil(hi[i]);
      if (!(f >= 8.0 * KF_BRICK_KEY_MIN && c < 8.0 * KF_BRICK_KEY_MAX)) return -1;   // (also what is not a number)
      b0[i] = (int64_t)f >> 3; b1[i] = (int64_t)c >> 3;
    }
    for (int64_t z = b0[2]; z <= b1[2]; ++z)
      for (int64_t y = b0[1]; y <= b1[1]; ++y)
        for (int64_t x = b0[0]; x <= b1[0]; ++x) words.push_back(kf_rigid_order_word(x, y, z));
  }
  std::sort(words.begin(), words.end());
  words.erase(std::unique(words.begin(), words.end()), words.end());
  return (int64_t)words.size();
}
// The open-addressing table over the source keys (in range, unique: the caller has checked) that the resampling kernel probes with store_find: a power of
// two >= 2 * count entries (at least 2), a key at the first free entry from kf_brick_key_hash on, its entry's index beside it.  Returns the mask.
static inline uint32_t kf_rigid_source_table(uint32_t count, const int32_t* keys, std::vector<unsigned long long>& tkey, std::vector<unsigned>& tslot) {
  uint64_t cap = 2;
  while (cap < 2ull * count) cap <<= 1;
  const uint32_t mask = (uint32_t)(cap - 1);
  tkey.assign((size_t)cap, KF_BRICK_KEY_EMPTY);
  tslot.assign((size_t)cap, 0u);
  for (uint32_t e = 0; e < count; ++e) {
    const unsigned long long key = kf_brick_key_pack(keys[3 * (size_t)e], keys[3 * (size_t)e + 1], keys[3 * (size_t)e + 2]);
    uint32_t h = kf_brick_key_hash(key, mask);
    while (tkey[h] != KF_BRICK_KEY_EMPTY) h = (h + 1u) & mask;   // at most half the entries are taken: a free one exists
    tkey[h] = key; tslot[h] = e;
  }
  return mask;
}
// What every entry point that takes a source map asks of its keys before anything is touched (kf_merge_brick_store_rigid, kf_merge_brick_store_halved,
// kf_align_brick_store): every component in the key range, every brick named once; then the table above.  False -- the callers' KF_ERR_ARG, which this plain
// header does not see -- leaves tkey, tslot and mask as they were.  (A std::bad_alloc reaches the caller's try.)
static inline bool kf_source_keys_table(uint32_t count, const int32_t* keys, std::vector<unsigned long long>& tkey, std::vector<unsigned>& tslot, uint32_t& mask) {
  std::vector<unsigned long long> packed(count);
  for (uint32_t i = 0; i < count; ++i) {
    const int32_t* k = keys + 3 * (size_t)i;
    for (int j = 0; j < 3; ++j) if (!kf_brick_key_in_range(k[j])) return false;
    packed[i] = kf_brick_key_pack(k[0], k[1], k[2]);
  }
  if (!kf_brick_keys_unique(packed.data(), packed.size())) return false;
  mask = kf_rigid_source_table(count, keys, tkey, tslot);
  return true;
}

static inline void kf_rigid_word_key(uint64_t w, int32_t out[3]) {
  const uint64_t m = (1ull << KF_BRICK_KEY_BITS) - 1ull;
  for (int k = 0; k < 3; ++k) out[k] = (int32_t)((w >> (k * KF_BRICK_KEY_BITS)) & m) + KF_BRICK_KEY_MIN;
}
static inline int64_t kf_rigid_keys(uint32_t count, const int32_t* keys, const double* xf, int32_t* out_keys, int64_t cap) {
  if (cap > 0 && !out_keys) return -1;
  std::vector<uint64_t> words;
  const int64_t n = kf_rigid_candidates(count, keys, xf, words);
  for (int64_t i = 0; i < n && i < cap; ++i) kf_rigid_word_key(words[(size_t)i], out_keys + 3 * i);
  return n;
}
