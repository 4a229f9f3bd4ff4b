// map_lookup.h -- the map as a function of a world voxel (device): the window's copy, else the brick store's, else nothing -- the rule of map_resolve_brick
// (vwindow.h) without a resolve table, for callers that read a few voxels at arbitrary places (query.hip: kf_map_sample, kf_map_cast_rays).  No reference
// counterpart.  Include after kf_internal.h, brick_key.h and brick_find.h.  The definition is written out above kf_map_sample in include/hybkf.h.
#pragma once

namespace mapq {

// where the map lies: the window's planes, its origin in world bricks, the store
struct MapRef { KfVolume vol; KfBrickStore st; int ob[3]; };
// (host) the map of a whole-volume context (kf_whole_volume)
static inline MapRef query_map(const kf_ctx* c) {
  MapRef m;
  m.vol = c->vol; m.st = c->bstore;
  for (int k = 0; k < 3; ++k) m.ob[k] = c->origin_vox[k] >> 3;      // (a multiple of 8; the shift floors)
  return m;
}

// the last brick a lane resolved: its key, its base pointers (tw == nullptr: nobody holds it) and its four deferred-weight words
struct MapBrick {
  unsigned long long key;
  const float2* tw;
  const uchar4* color;
  unsigned long long pend;
};
__device__ __forceinline__ MapBrick map_brick_none() { MapBrick b; b.key = KF_BRICK_KEY_EMPTY; b.tw = nullptr; b.color = nullptr; b.pend = 0ull; return b; }

// world brick (bx, by, bz), each in the key range: the window's copy where the brick is inside the window (the newer one), else the store's, else absent
__device__ __forceinline__ void map_brick_resolve(const MapRef& m, int bx, int by, int bz, unsigned long long key, MapBrick& b) {
  b.key = key; b.tw = nullptr; b.color = nullptr; b.pend = 0ull;
  const int nb = m.vol.nb;
  const int lx = bx - m.ob[0], ly = by - m.ob[1], lz = bz - m.ob[2];
  if ((unsigned)lx < (unsigned)nb && (unsigned)ly < (unsigned)nb && (unsigned)lz < (unsigned)nb) {
    const size_t s = ((size_t)lz * nb + (size_t)ly) * nb + (size_t)lx;
    b.tw = m.vol.tw + s * KF_BRICK_VOX;
    if (m.vol.color) b.color = m.vol.color + s * KF_BRICK_VOX;
    b.pend = m.vol.pend[s];
  } else if (m.st.max_bricks) {
    const unsigned s = store_find(m.st, key);
    if (s != KF_BRICK_NO_SLOT) {
      b.tw = m.st.tw + (size_t)s * KF_BRICK_VOX;
      if (m.st.color) b.color = m.st.color + (size_t)s * KF_BRICK_VOX;
      b.pend = m.st.pend[s];
    }
  }
}

// the lane's cached brick made the one of world voxel (gx, gy, gz); false: the voxel lies outside the key range
__device__ __forceinline__ bool map_brick_at(const MapRef& m, int gx, int gy, int gz, MapBrick& b) {
  const int bx = gx >> 3, by = gy >> 3, bz = gz >> 3;
  if (!kf_brick_key_in_range(bx) || !kf_brick_key_in_range(by) || !kf_brick_key_in_range(bz)) return false;
  const unsigned long long key = kf_brick_key_pack(bx, by, bz);
  if (key != b.key) map_brick_resolve(m, bx, by, bz, key, b);
  return true;
}

// World voxel (gx, gy, gz) as (tsdf, TRUE weight); a voxel whose true weight is not > 0, or that nobody holds, reads (0, 0).  off: its place in the brick.
__device__ __forceinline__ float2 map_voxel(const MapRef& m, int gx, int gy, int gz, MapBrick& b, unsigned& off) {
  off = (unsigned)(((gz & 7) << 6) | ((gy & 7) << 3) | (gx & 7));
  if (!map_brick_at(m, gx, gy, gz, b) || !b.tw) return make_float2(0.f, 0.f);
  const float2 q = b.tw[off];
  const unsigned pq = (unsigned)(b.pend >> (16u * (off >> 7))) & 0xFFFFu;
  const float w = kf_pend_weight(q.y, pq, m.vol.max_weight);
  return w > 0.f ? make_float2(q.x, w) : make_float2(0.f, 0.f);
}

// the colour of a voxel map_voxel has just read as observed (b is its brick); 0 on a map without a colour plane
__device__ __forceinline__ uchar4 map_voxel_color(const MapBrick& b, unsigned off) {
  return b.color ? b.color[off] : make_uchar4(0, 0, 0, 0);
}

}  // namespace mapq
