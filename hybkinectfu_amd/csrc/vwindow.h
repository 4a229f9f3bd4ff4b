// vwindow.h -- the VIRTUAL window: the window as kf_shift_volume would have assembled it at another origin, the brick store's bricks restored, without
// moving anything.  Shared by the map mesh (mapmesh.hip: kf_marching_cubes_at) and the map's viewer frames (viewat.hip: kf_render_view_at): one entry of 16
// bytes per brick slot of the window's shape says where that brick's voxels and colours are read from, and every read downstream is an unconditional load
// through one table entry.  Include after kf_internal.h, brick_key.h and brick_find.h.
#pragma once

namespace mapmesh {

struct McVBrick { const float2* tw; const uchar4* color; };        // one virtual brick slot: its 512 (tsdf, weight) pairs, its 512 colours

// voxel (x, y, z) of the virtual window
__device__ __forceinline__ float2 v_voxel(const McVBrick* __restrict__ tab, const KfVolume& v, int x, int y, int z) {
  return tab[kf_brick_slot(v, x >> 3, y >> 3, z >> 3)].tw[((z & 7) << 6) | ((y & 7) << 3) | (x & 7)];
}
// the eight gathers of a lookup (kf_interp_load) through the table
__device__ __forceinline__ void v_interp_load(const McVBrick* __restrict__ tab, const KfVolume& v, const KfInterp& it, float2 q[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = make_float2(0.f, 0.f);
  if (it.ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int x = it.g.x + (k >> 2), y = it.g.y + ((k >> 1) & 1), z = it.g.z + (k & 1);
      q[k] = tab[kf_brick_slot(v, x >> 3, y >> 3, z >> 3)].tw[((z & 7) << 6) | ((y & 7) << 3) | (x & 7)];
    }
  }
}
// kf_interp_load_nb through the table: no branch around the loads; a lookup that fails its range test reads voxel 0 of slot 0 -- a resolved entry, value unused
__device__ __forceinline__ void v_interp_load_nb(const McVBrick* __restrict__ tab, const KfVolume& v, const KfInterp& it, float2 q[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = it.g.x + (k >> 2), y = it.g.y + ((k >> 1) & 1), z = it.g.z + (k & 1);
    q[k] = it.ok ? v_voxel(tab, v, x, y, z) : tab[0].tw[0];
  }
}
// kf_interpolate_sdf_pair through the table: two lookups, 16 gathers in flight
__device__ __forceinline__ void v_interpolate_sdf_pair(const McVBrick* __restrict__ tab, const KfVolume& v, float3 p1, float3 p2, const KfRecip& rS, const KfRecip& rcell,
                                                       bool& ok1, float& d1, bool& ok2, float& d2) {
  const KfInterp i1 = kf_interp_prepare(v, p1, rS, rcell), i2 = kf_interp_prepare(v, p2, rS, rcell);
  float2 q1[8], q2[8];
  v_interp_load(tab, v, i1, q1); v_interp_load(tab, v, i2, q2);
  d1 = 0.f; d2 = 0.f;
  ok1 = kf_interp_finish(i1, q1, d1); ok2 = kf_interp_finish(i2, q2, d2);
}
// kf_interpolate_color through the table: the same arithmetic in the same order
__device__ __forceinline__ bool v_interp_color(const McVBrick* __restrict__ tab, const KfVolume& v, float3 pos, uchar4& out) {
  int3 g; float a, b, c;
  if (!kf_interp_params(v, pos, g, a, b, c)) return false;
  if (!kf_z_stored(v, g.z) || !kf_z_stored(v, g.z + 1)) return false;
  float ia = 1 - a, ib = 1 - b, ic = 1 - c;
  float wgt[8]; uchar4 col[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = g.x + (k >> 2), y = g.y + ((k >> 1) & 1), z = g.z + (k & 1);
    const McVBrick e = tab[kf_brick_slot(v, x >> 3, y >> 3, z >> 3)];
    const int o = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
    wgt[k] = e.tw[o].y; col[k] = e.color[o];
  }
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (wgt[k] == 0.f) return false;
    float wa = (k >> 2) ? a : ia, wb = ((k >> 1) & 1) ? b : ib, wc = (k & 1) ? c : ic;
    float t0 = (float)col[k].x * wa * wb * wc, t1 = (float)col[k].y * wa * wb * wc, t2 = (float)col[k].z * wa * wb * wc;
    acc[0] = (k == 0) ? t0 : acc[0] + t0; acc[1] = (k == 0) ? t1 : acc[1] + t1; acc[2] = (k == 0) ? t2 : acc[2] + t2;
  }
  out = make_uchar4((unsigned char)acc[0], (unsigned char)acc[1], (unsigned char)acc[2], 0);
  return true;
}

// ---- resolve -------------------------------------------------------------------------------------------------------------------------------
// wlo, wn: the brick range of the virtual window that is resolved; fb: the frame's origin in world bricks; ob: the window's
struct McResolve { int wlo[3], wn[3], fb[3], ob[3]; };
// One wave resolves virtual brick (bx, by, bz): world brick fb + b lies in the current window -> the window's copy (the newer one: a restored brick stays
// in the store as a stale copy) and the window's own has-negative bit; else the store's slot if the key is found, with the OR over its voxels reduced here
// (what k_store_restore would compute; the store keeps no flags); else the shared all-zero brick.  Wave-uniform up to the reduction.
__device__ __forceinline__ McVBrick map_resolve_brick(const KfVolume& v, const KfBrickStore& st, const McResolve& g, int bx, int by, int bz,
                                                      const float2* __restrict__ zero, unsigned lane, bool& neg) {
  const int nb = v.nb;
  const int wx = g.fb[0] + bx, wy = g.fb[1] + by, wz = g.fb[2] + bz;                             // the world brick
  const int lx = wx - g.ob[0], ly = wy - g.ob[1], lz = wz - g.ob[2];                             // ... in the window's bricks
  McVBrick e; e.tw = zero; e.color = reinterpret_cast<const uchar4*>(zero);
  neg = false;
  if ((unsigned)lx < (unsigned)nb && (unsigned)ly < (unsigned)nb && (unsigned)lz < (unsigned)nb) {
    const size_t s = ((size_t)lz * nb + (size_t)ly) * nb + (size_t)lx;
    e.tw = v.tw + s * KF_BRICK_VOX;
    if (v.color) e.color = v.color + s * KF_BRICK_VOX;
    neg = (v.negbits[s >> 5] >> (s & 31u)) & 1u;
  } else if (st.max_bricks) {
    const unsigned s = store_find(st, kf_brick_key_pack(wx, wy, wz));
    if (s != KF_BRICK_NO_SLOT) {
      e.tw = st.tw + (size_t)s * KF_BRICK_VOX;
      if (st.color) e.color = st.color + (size_t)s * KF_BRICK_VOX;
      const float4* p = reinterpret_cast<const float4*>(e.tw);
      bool mine = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float4 q = p[lane + 64u * (unsigned)k]; mine = mine || q.x < 0.f || q.z < 0.f; }
      neg = __ballot(mine) != 0ull;
    }
  }
  return e;
}

}  // namespace mapmesh
