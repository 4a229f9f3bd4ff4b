// raycast_tile.h -- the march of one 32x16 pixel tile (raycast_tile) with everything it is made of, and the host side that places its LDS tables
// (raycast_args).  Compiled twice, like mc_kernels.h: by raycast.hip over the window's own voxels, and by viewat.hip (kf_render_view_at) over a VIRTUAL
// window whose bricks are reached through an indirection table.  What differs is only where a voxel, a colour and a brick's has-negative flag are read:
// the hooks below, which a translation unit defines before the #include to replace them.  The defaults are the expressions raycast.hip has always had.
// No #include here: viewat.hip includes the file inside a namespace.
#ifndef RC_VOL
#define RC_VOL KfVolume                                    /* the type of RaycastArgs::vol: KfVolume or a struct derived from it */
#define RC_VOL_ASSIGN(dst, src) ((dst) = (src))            /* the KfVolume part of RaycastArgs::vol from the context's */
#define RC_TSDF_IN_SLOT(v, slot, off) ((v).tw[(size_t)(slot) * KF_BRICK_VOX + (size_t)(off)].x)     /* voxel `off` of stored brick `slot` */
#define RC_TSDF_AT(v, gx_, gy_, gz_) ((v).tw[kf_vox_index(v, gx_, gy_, gz_)].x)                    /* voxel (gx_, gy_, gz_), in a stored layer */
#define RC_BRICK_HASNEG(v, slot) (((v).flags[slot] & KF_FLAG_HASNEG) != 0)                          /* asked only when the per-brick bits are not in LDS */
#define RC_INTERP_LOAD(v, it, q) kf_interp_load(v, it, q)
#define RC_INTERP_LOAD_NB(v, it, q) kf_interp_load_nb(v, it, q)
#define RC_INTERP_SDF_PAIR(v, p1, p2, rS, rcell, ok1, d1, ok2, d2) kf_interpolate_sdf_pair(v, p1, p2, rS, rcell, ok1, d1, ok2, d2)
#define RC_INTERP_COLOR(v, pos, out) kf_interpolate_color(v, pos, out)
#define RC_SHARED_GRAD(shared) (shared)                    /* grad_shared.h reads v.tw through a buffer descriptor: 0 where there is no such plane */
#endif

// KF_RAYCAST_SHARED_GRAD (0 / 1 / 2, see RaycastArgs::shared_grad) in bits 0-7, KF_RAYCAST_VIEW_HALF (tests: brick layers of the gathers' view on either side, 0 = most) above.
// Read at every launch (uncached in kf_switches.h), unlike the other switches: a test can then compare the forms on ONE context -- the only way at 2048^3, where a second process
// would have to fuse 69 GB again.
static int rc_shared_grad_env() {
  const int mode = kf_switch(KF_SW_RAYCAST_SHARED_GRAD), half = kf_switch(KF_SW_RAYCAST_VIEW_HALF);
  return mode <= 0 ? 0 : ((mode & 255) | ((half > 0 && half < 4096 ? half : 0) << 8));
}
// the gathers' view spans at least two brick layers: they must fit 32-bit offsets (they do up to 724 bricks per axis; beyond: six separate lookups)
static int rc_shared_grad_for(const KfVolume& v) { return (unsigned long long)v.nb * v.nb * KF_BRICK_VOX * sizeof(float2) <= (1ull << 31) ? rc_shared_grad_env() : 0; }

struct RaycastArgs {
  RC_VOL vol;
  KfCam cam;
  const float* pose;             // device pointer or null -> pose_val
  KfMat pose_val;
  float4* out_v; float4* out_n; uchar4* out_rgb;
  float* out_t;                  // optional: ray parameter of the first crossing this context detected (+inf: none) -- z-slab merge
  unsigned long long* own_ta;    // z-slab merge, speculative normals (kf_raycast_volume_slab_cross_spec): a second copy of this context's words (the caller all-reduces out_ta in place) ...
  float* out_spec;               // ... and, three floats per pixel, the gradient at this context's own crossing's vertex when that vertex lies in the layers it OWNS (else zeros):
                                 // what kf_slab_ray_normals would compute for the pixel if this crossing wins the MIN all-reduce -- evaluated here, in the shadow of the march
  unsigned long long* out_ta;    // z-slab merge (what SlabPipeline runs): per pixel (bits of the crossing's ray parameter) << 32 | bits of the VERTEX's ray parameter
                                 // alpha -- +inf / 0 without a crossing, alpha 0 where the reference gives up at the crossing (raycastingVolume.cu:87-88).  Only the two
                                 // interpolations at the crossing are evaluated here; the gradient around the vertex is the job of whoever owns the vertex (k_slab_ray_normals)
  KfPyrOut pyr;                  // v1 non-null: the workgroups also leave levels 1 and 2 of the two maps' pyramids (bilateral_tile.h: kf_tile_pyramid)
  float inc, near_plane, far_plane;
  int has_color;
  int neg_words;                 // words of vol.negbits to keep in LDS (0: the table does not fit -> brick flags are read from global memory)
  int meso_words;                // words of the meso table (16^3-voxel cells) to keep in LDS behind the macro / super tables (0: it does not fit)
  int shared_grad;               // 1: a crossing's six gradient taps come from one 32-voxel neighbourhood (grad_shared.h; KF_RAYCAST_SHARED_GRAD=0: six separate lookups; 2: shared, with every other wave forced down the fallback -- tests)
  int bounds_meso;               // 1: where the volume has at most 8192 meso cells (up to 256^3), the tile bounds come from the meso table (KF_RAYCAST_BOUNDS_MESO=0: from the macro table)
  int tile_bounds;               // 1: every workgroup first bounds its tile's rays by the non-empty macro cells its frustum meets (rc_tile_bounds; KF_RAYCAST_BOUNDS=0: off,
                                 // 2: tests -- always through the super-cell list, whatever the volume's size)
  int exp_mode;                  // timing experiments only (KF_RAYCAST_EXP): 1 = stop at the crossing without evaluating it
  KfCounters* work;              // measurement passes only (kf_stage_timers bit 16): count the reference march's samples and the hits
};

// gradientForPoint raycastingVolume.cu:16-42: bounds tested on the LAST sample's voxel, taps taken around the vertex.
// The six taps (+x, -x, +y, -y, +z, -z) are looked up BATCH at a time (BATCH x 8 gathers in flight: 2 = the +/- pair of an axis, 3 = two round trips for the
// six, 6 = one); the reference's early-outs are pure, so loading a batch and then testing the verdicts in its order (+ then -, x then y then z) is equivalent.
// The interpolation itself is the reference's, operation for operation (kf_interp_prepare / kf_interp_finish).
template <int BATCH>
__device__ __forceinline__ bool gradient_for_point(const RC_VOL& v, float3 samplepos, float3 vtx, const KfRecip& rS, const KfRecip& rcell, float3& grad) {
  static_assert(BATCH == 2 || BATCH == 3 || BATCH == 6, "six taps in whole batches");
  const float rf = (float)v.res;
  const int3 g = make_int3(kf_f2i(kf_div(samplepos.x * rf, rS)), kf_f2i(kf_div(samplepos.y * rf, rS)), kf_f2i(kf_div(samplepos.z * rf, rS)));
  const int R = v.res;
  if (g.x <= 1 || g.x >= R - 2) return false;
  if (g.y <= 1 || g.y >= R - 2) return false;
  if (g.z <= 1 || g.z >= R - 2) return false;
  const float cell = v.cell;
  float f[6]; bool o[6];
#pragma unroll
  for (int k0 = 0; k0 < 6; k0 += BATCH) {
    KfInterp it[BATCH]; float2 q[BATCH][8];
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
      const int t = k0 + k; const float d = (t & 1) ? -cell : cell;
      const float3 p = kf3(vtx.x + ((t >> 1) == 0 ? d : 0.f), vtx.y + ((t >> 1) == 1 ? d : 0.f), vtx.z + ((t >> 1) == 2 ? d : 0.f));
      it[k] = BATCH == 2 ? kf_interp_prepare(v, p, rS, rcell) : kf_interp_prepare_nb(v, p, rS, rcell);
    }
#pragma unroll
    for (int k = 0; k < BATCH; ++k) { if (BATCH == 2) RC_INTERP_LOAD(v, it[k], q[k]); else RC_INTERP_LOAD_NB(v, it[k], q[k]); }     // (larger batches: no branch around the loads, so that they travel together)
#pragma unroll
    for (int k = 0; k < BATCH; ++k) { f[k0 + k] = 0.f; o[k0 + k] = kf_interp_finish(it[k], q[k], f[k0 + k]); }
    // (:22-37: the reference returns at the first failing tap; every tap of this batch and the earlier ones must have succeeded to go on)
#pragma unroll
    for (int k = 0; k < BATCH; ++k) if (!o[k0 + k]) return false;
  }
  float3 n;
  n.x = f[0] - f[1]; n.y = f[2] - f[3]; n.z = f[4] - f[5];
  float len = kf_norm(n);
  if ((double)len < 1e-8) return false;
  grad = kf_scale(n, 1 / len);                               // fp32 reciprocal (:40), unlike normalize()
  return true;
}

// The same verdict and gradient from the shared neighbourhood (grad_shared.h): nine cell computations and 32 gathers instead of 18 and 48.  A wave in which
// some lane's tap cell is not "vtx's cell moved by one" -- and whose verdict is not false already -- evaluates the generic way, all lanes together.
template <int BATCH, int ROUNDS>
__device__ __forceinline__ bool gradient_for_point_either(int shared, bool odd_wave, const RC_VOL& v, float3 samplepos, float3 vtx, const KfRecip& rS, const KfRecip& rcell, float3& grad) {
  int verdict = 2;
  if (RC_SHARED_GRAD(shared)) verdict = rc_gradient_shared<ROUNDS>(v, samplepos, vtx, rS, rcell, (shared & 255) == 2 && odd_wave, shared >> 8, grad);       // (`shared` is a launch argument: uniform; 2: every other wave is sent down the generic path)
  if (verdict == 2) verdict = gradient_for_point<BATCH>(v, samplepos, vtx, rS, rcell, grad) ? 1 : 0;
  return verdict == 1;
}

// the walk of the ray parameter: the chain of additions itself.  Its closed form (kf_ray_advance: exact, self-tested) is 3-4 % SLOWER here --
// a walk is 1-12 additions at the stock increment (4.5 voxels) and the chain costs three instructions per step (-DKF_RAY_ADVANCE_CLOSED for the A/B)
#ifdef KF_RAY_ADVANCE_CLOSED
#define RC_ADVANCE kf_ray_advance
#elif defined(RC_TRIP_OFF) && (RC_TRIP_OFF & 16)
#define RC_ADVANCE kf_ray_advance_plain
#else
#define RC_ADVANCE kf_ray_advance_plain2                   /* the same chain, two additions per loop round (kf_internal.h) */
#endif
#define RAYCAST_THREADS 512
#ifndef RC_GRAD_BATCH
#define RC_GRAD_BATCH 2           // taps of the crossing's gradient looked up together (2 / 3 / 6); 3 (two round trips) measured slower under the launch's 80-register cap: 46.0 vs 45.1 us at C2, 85.0 vs 83.6 at C4
#endif
#ifndef RC_GRAD_ROUNDS
#define RC_GRAD_ROUNDS 4          // the shared-neighbourhood form of those taps (grad_shared.h): gathers in 1 / 2 / 4 dependent rounds of 32 / 16 / 8
#endif
#ifndef RC_SLAB_GRAD_ROUNDS
#define RC_SLAB_GRAD_ROUNDS 1     // the same in k_slab_ray_normals (no register cap there)
#endif
#define RAYCAST_LDS_BYTES 49152   // budget for the two bit tables: 3 workgroups x 8 waves stay resident per CU (160 KiB LDS)

// bit `i` of a packed table
__device__ __forceinline__ bool rc_bit(const unsigned* words, unsigned i) { return (words[i >> 5] >> (i & 31u)) & 1u; }

// The march of one ray over the samples t_k in [t, t_end): the reference's loop (raySample :65-119) with the two empty-space levels.
// `t`, `t_prev`, `have_last`, `last_sdf` carry the reference's per-ray state in; on return t_cross < +inf names the first crossing of
// the range (with t_cross_prev the sample before it).  Whether sample k is a crossing depends on samples k-1 and k only (the previous
// sample's tsdf is fetched on demand), so a ray's range may be marched in pieces by different lanes: the first crossing of the ray
// is the first piece's that has one.
struct RcRay { float3 org, dir, inv_dir; };
// The loop is compiled once per way of forming a voxel coordinate -- a wave-uniform fact -- and chosen by rc_march with one branch outside it (tested
// inside the loop, the size's power-of-two test was two taken scalar branches per axis and trip, and again in the lazy previous-sample fetch):
// SCALE   how `worldPos * resolution / size` (tsdfVolume.h:50-56) is formed.  RC_SCALE_DIV: the quotient (kf_div).  RC_SCALE_MUL2: the size is a power of
//         two, so the quotient is an exact scaling -- the same bits from the product (pos * res) * (1 / size).  RC_SCALE_MUL1: the resolution is a power of two
//         as well and res >= size: pos * (res / size), one multiplication.  Same bits again: with res = 2^a, size = 2^b, a >= b, the first product of the
//         two-step form is pos * 2^a EXACTLY (scaling up never drops a bit, of a subnormal pos neither, and |pos| * 2^a is far from overflow), and its second
//         product rounds the real number pos * 2^(a - b) -- which is representable, being pos scaled up by 2^(a - b) >= 1 -- hence to itself: what the one
//         multiplication gives.  With res < size the net scaling is DOWN and a tiny pos may round: that case keeps the two products, whatever they give.
//         RC_SCALE_ANY: decided inside the loop, as before the loop was instantiated (A/B builds only).
// RC_SCALE_DIV and RC_SCALE_MUL2 are the arithmetic the march has always had, statement for statement.
enum { RC_SCALE_ANY = -1, RC_SCALE_DIV = 0, RC_SCALE_MUL2 = 1, RC_SCALE_MUL1 = 2 };
// A/B builds (tools/build_variant.sh <name> -DRC_TRIP_OFF=<bits>) take single steps back to the earlier instruction stream: 1 the one-multiplication scaling,
// 2 the median-of-three clamps, 16 the two-step walk, 32 the instantiation itself (which the first needs).  Every combination computes the same bits.
// (profiles/raycast_march_trip.txt: what each step measured, and the steps that were measured and taken out again.)
#ifndef RC_TRIP_OFF
#define RC_TRIP_OFF 0
#endif
__device__ __forceinline__ int rc_clamp_voxel(int g, int R) { return (RC_TRIP_OFF & 2) ? max(0, min(g, R - 1)) : kf_clamp0(g, R - 1); }
template <int SCALE>
__device__ __forceinline__ void rc_march_loop(const RaycastArgs& a, const RC_VOL& v, const unsigned* s_macro, const unsigned* s_super, const unsigned* s_meso, const unsigned* s_neg, bool neg_in_lds, const RcRay& ray,
                                              const KfRecip& rS, float t_end, float& t, float& t_prev, bool& have_last, float& last_sdf,
                                              float& t_cross, float& t_cross_prev, int& n_iter, int& n_samp, int& n_macro) {
  const float3 org = ray.org, dir = ray.dir;
  const int R = v.res;
  const float rf = (float)R;
  const int zs0 = v.bz0 * KF_BRICK, zs1 = v.bz1 * KF_BRICK;
  const int nm = v.nm, ns = v.ns, nq = v.nq;
  const bool meso_in_lds = a.meso_words != 0;
  // the empty-space walk measures in VOXEL units along each axis: with q the sample's (unrounded) voxel coordinate and `base` the first voxel
  // of its cell (32 voxels wide for a macro cell, 8 for a brick), the cell's far face lies E - (q - base) voxels ahead for a ray going up
  // the axis and q - base voxels for one going down: one fused multiply-add per axis with the ray's constants sgn / up, times cell / |dir|
  const float3 sgn = kf3(dir.x > 0.f ? -1.f : 1.f, dir.y > 0.f ? -1.f : 1.f, dir.z > 0.f ? -1.f : 1.f);
  const float3 up = kf3(dir.x > 0.f ? 1.f : 0.f, dir.y > 0.f ? 1.f : 0.f, dir.z > 0.f ? 1.f : 0.f);
  const float3 per_vox = kf3(v.cell * fabsf(ray.inv_dir.x), v.cell * fabsf(ray.inv_dir.y), v.cell * fabsf(ray.inv_dir.z));
  // `worldPos * resolution / size` (tsdfVolume.h:50-56): for a power-of-two size the quotient is an exact scaling -- the same bits from a product
  const float inv_size = 1.0f / v.size;
  const float res_by_size = rf * inv_size;                                  // RC_SCALE_MUL1: a power of two >= 1, exact
  const bool pow2 = (__float_as_uint(v.size) & 0x007FFFFFu) == 0u;          // RC_SCALE_ANY
  // one coordinate's voxel number, unrounded; the lazy previous-sample fetch below forms it the same way
  auto to_voxels = [&](float p) -> float {
    if (SCALE == RC_SCALE_MUL1) return p * res_by_size;
    if (SCALE == RC_SCALE_MUL2) return (p * rf) * inv_size;
    if (SCALE == RC_SCALE_DIV) return kf_div(p * rf, rS);
    return pow2 ? (p * rf) * inv_size : kf_div(p * rf, rS);
  };
  while (t < t_end) {
    ++n_iter;
    const float3 pos = kf_add(org, kf_scale(dir, t));
    // the sample's own voxel -- tsdfvolume::getVoxel(world) tsdfVolume.h:81-97: nearest voxel, index clamped
    const float qx = to_voxels(pos.x), qy = to_voxels(pos.y), qz = to_voxels(pos.z);
    const int gx = rc_clamp_voxel(kf_f2i(qx), R), gy = rc_clamp_voxel(kf_f2i(qy), R), gz = rc_clamp_voxel(kf_f2i(qz), R);
    // level 1: a 32^3-voxel macro cell without any negative voxel -> none of the samples inside it can be the negative
    // side of a crossing: walk to its far side.  The cell is the VOXEL's macro cell (g >> 5), like the brick level below:
    // picking it from the position with a different rounding could disagree with the voxel index at a cell face and skip
    // a sample whose voxel lies in the neighbouring (non-empty) cell.
    // level 2: only samples whose voxel this context OWNS can be its crossing candidates (the whole volume on one GPU; with
    // z-slabs the neighbour's layers are stored as halo and serve the previous-sample / trilinear / gradient reads only); a brick
    // that never held a negative tsdf cannot hold the negative sample of a crossing either.
    // Both levels take ONE code path with selected parameters: the lanes of
    // a wave sit in different states, and a wave executes the union of the paths its lanes take on every trip.
    const int mx = gx >> 5, my = gy >> 5, mz = gz >> 5;
    const bool macro_empty = !rc_bit(s_macro, __umul24(__umul24((unsigned)mz, (unsigned)nm) + (unsigned)my, (unsigned)nm) + (unsigned)mx);
    // level 0: the 128^3-voxel super cell (4 x 4 x 4 macro cells) the same way -- two thirds of a ray's trips were macro cells of open space
    const bool super_empty = !rc_bit(s_super, __umul24(__umul24((unsigned)(mz >> KF_SUPER_SHIFT), (unsigned)ns) + (unsigned)(my >> KF_SUPER_SHIFT), (unsigned)ns) + (unsigned)(mx >> KF_SUPER_SHIFT));
    const bool owned = gz >= v.own_z0 && gz < v.own_z1;
    // level 1.5 (round 5): the 16^3-voxel meso cell (2 x 2 x 2 bricks) -- inside a non-empty macro cell most bricks are still empty, and at 1024^3 the per-brick bits do
    // not fit into LDS (every brick-level trip then reads the flag byte from global memory): the meso bits do (32 KiB), and an empty meso cell is walked in one trip
    const bool meso_empty = meso_in_lds && !macro_empty &&
                            !rc_bit(s_meso, __umul24(__umul24((unsigned)(gz >> 4), (unsigned)nq) + (unsigned)(gy >> 4), (unsigned)nq) + (unsigned)(gx >> 4));
    size_t slot = 0; bool has_neg = false;
    if (!macro_empty && !meso_empty && owned) {
      slot = kf_brick_slot(v, gx >> 3, gy >> 3, gz >> 3);
      has_neg = neg_in_lds ? rc_bit(s_neg, (unsigned)slot) : RC_BRICK_HASNEG(v, slot);
    }
    if (!has_neg) {
      n_macro += macro_empty ? (super_empty ? 0x10000 : 1) : 0;
      // macro cell: walk to its far side; owned brick with the table an LDS read away: brick by brick is cheaper than sample by
      // sample (the cell is the VOXEL's brick: if rounding put pos a hair outside it, the walk is merely shorter, never past the
      // far face); otherwise one sample
      const bool walk = macro_empty || meso_empty || (owned && neg_in_lds);
      if (walk) {
        const int sup = (KF_MACRO << KF_SUPER_SHIFT);
        const int mask = super_empty ? ~(sup - 1) : macro_empty ? ~31 : meso_empty ? ~15 : ~7;
        const float edge = super_empty ? (float)sup : macro_empty ? 32.f : meso_empty ? 16.f : 8.f;
        const float eps = super_empty ? 1e-4f * (float)sup : macro_empty ? 3.2e-3f : meso_empty ? 4e-3f : 8e-3f;       // eps: 1e-4 / 1e-4 / 2.5e-4 / 1e-3 of the cell edge, in voxels
        // the exit parameter only has to be conservative (eps and the 1e-6 t margin absorb a few ulps)
        const float dx = __builtin_fmaf(qx - (float)(gx & mask), sgn.x, up.x * edge) - eps;
        const float dy = __builtin_fmaf(qy - (float)(gy & mask), sgn.y, up.y * edge) - eps;
        const float dz = __builtin_fmaf(qz - (float)(gz & mask), sgn.z, up.z * edge) - eps;
        const float dt = fminf(fminf(dx * per_vox.x, dy * per_vox.y), dz * per_vox.z);
        const float t_exit = fminf(t + dt - 1e-6f * t, t_end);
        RC_ADVANCE(t, t_prev, a.inc, t_exit);                   // the reference's own repeated addition: identical sample parameters
      } else { t_prev = t; t += a.inc; }
      have_last = false;
      continue;
    }
    ++n_samp;
    const float sdf = RC_TSDF_IN_SLOT(v, slot, ((gz & 7) << 6) | ((gy & 7) << 3) | (gx & 7));
    if (sdf < 0.0f) {
      if (!have_last) {                                                    // the previous sample's tsdf was never fetched: fetch it now
        const float3 last_pos = kf_add(org, kf_scale(dir, t_prev));        // recomputed exactly as the march computed it
        const int lx = rc_clamp_voxel(kf_f2i(to_voxels(last_pos.x)), R), ly = rc_clamp_voxel(kf_f2i(to_voxels(last_pos.y)), R), lz = rc_clamp_voxel(kf_f2i(to_voxels(last_pos.z)), R);
        last_sdf = (lz >= zs0 && lz < zs1) ? RC_TSDF_AT(v, lx, ly, lz) : 0.f;
        have_last = true;
      }
      if (last_sdf > 0.0f) { t_cross = t; t_cross_prev = t_prev; break; }  // zero crossing :83
    }
    last_sdf = sdf; have_last = true; t_prev = t;
    t += a.inc;
  }
}
// the instantiation of a launch: every quantity is a kernel argument, so the branches are uniform and taken once per ray, outside the loop
__device__ __forceinline__ void rc_march(const RaycastArgs& a, const RC_VOL& v, const unsigned* s_macro, const unsigned* s_super, const unsigned* s_meso, const unsigned* s_neg, bool neg_in_lds, const RcRay& ray,
                                         const KfRecip& rS, float t_end, float& t, float& t_prev, bool& have_last, float& last_sdf,
                                         float& t_cross, float& t_cross_prev, int& n_iter, int& n_samp, int& n_macro) {
#define RC_MARCH_AS(SCALE) rc_march_loop<SCALE>(a, v, s_macro, s_super, s_meso, s_neg, neg_in_lds, ray, rS, t_end, t, t_prev, have_last, last_sdf, t_cross, t_cross_prev, n_iter, n_samp, n_macro)
  if (RC_TRIP_OFF & 32) { RC_MARCH_AS(RC_SCALE_ANY); return; }
  const bool size_pow2 = (__float_as_uint(v.size) & 0x007FFFFFu) == 0u;
  const bool one_mul = !(RC_TRIP_OFF & 1) && size_pow2 && (v.res & (v.res - 1)) == 0 && (float)v.res >= v.size;
  if (one_mul) RC_MARCH_AS(RC_SCALE_MUL1);
  else if (size_pow2) RC_MARCH_AS(RC_SCALE_MUL2);
  else RC_MARCH_AS(RC_SCALE_DIV);
#undef RC_MARCH_AS
}

// the ray of pixel (x, y) -- raycastKernel :136-150.  One function for the march and for k_slab_rays_unpack, which rebuilds a vertex from
// its ray parameter: the same operations in the same order give the same bits.
__device__ __forceinline__ void rc_pixel_ray(const KfCam& cam, const float* T, int x, int y, float3& org, float3& dir, float3& cam_dir) {
  cam_dir = kf_normalize(kf_depth_to_skeleton((unsigned)x, (unsigned)y, 1.0f, cam));
  org = kf3(T[3], T[7], T[11]);
  const float4 wd = kf_mat_vec(T, make_float4(cam_dir.x, cam_dir.y, cam_dir.z, 0.0f));
  dir = kf3(wd.x, wd.y, wd.z);
  dir.x = (dir.x == 0.f) ? (float)1e-15 : dir.x;
  dir.y = (dir.y == 0.f) ? (float)1e-15 : dir.y;
  dir.z = (dir.z == 0.f) ? (float)1e-15 : dir.z;
}

// a colour as the fourth word of the z-slab merge's candidates (b, g, r from the low byte up, as the uchar4 lies in memory); all-zero bits: none
__device__ __forceinline__ unsigned rc_color_word(uchar4 c) { return (unsigned)c.x | ((unsigned)c.y << 8) | ((unsigned)c.z << 16) | ((unsigned)c.w << 24); }
__device__ __forceinline__ uchar4 rc_word_color(unsigned w) { return make_uchar4((unsigned char)(w & 255u), (unsigned char)((w >> 8) & 255u), (unsigned char)((w >> 16) & 255u), (unsigned char)(w >> 24)); }

// [t_min, t_max) of a ray: getMinTime / getMaxTime (raycastingVolume.cu:44-63) clipped by the near / far planes (:152-153)
__device__ __forceinline__ void rc_ray_interval(float S, float near_plane, float far_plane, float3 org, float3 dir, float3 cam_dir, float& tmin, float& tmax) {
  tmin = fmaxf(fmaxf(((dir.x > 0 ? 0.f : S) - org.x) / dir.x, ((dir.y > 0 ? 0.f : S) - org.y) / dir.y), ((dir.z > 0 ? 0.f : S) - org.z) / dir.z);
  tmax = fminf(fminf(((dir.x > 0 ? S : 0.f) - org.x) / dir.x, ((dir.y > 0 ? S : 0.f) - org.y) / dir.y), ((dir.z > 0 ? S : 0.f) - org.z) / dir.z);
  tmin = fmaxf(tmin, near_plane / cam_dir.z);
  tmax = fminf(tmax, far_plane / cam_dir.z);
}

// ---- where along its rays can a 32x16 pixel tile meet a surface at all? ---------------------------------------------------------------------------------
// A crossing's negative sample lies in a macro cell (32^3 voxels) whose bit is set.  Before the march the workgroup intersects the tile's frustum (four planes
// through the camera centre, half a pixel of margin) with the bounding spheres of the non-empty SUPER cells, then of the non-empty MACRO cells inside those that
// pass, and keeps the smallest / largest distance from the camera centre any of them reaches: [t_lo, t_hi].  A ray parameter IS the distance from the camera
// centre (unit directions), so every sample outside that interval lies in an empty cell and can be skipped exactly like the march skips one empty cell at a
// time -- only all at once: the parameter is brought to t_lo by the reference's own chain of additions (kf_ray_advance, the closed form of that chain) and the
// march ends at t_hi.  At 512^3 the walk to the first surface was 5.8 of a ray's 11.7 loop trips (profiles/r03_raycast_levels.txt), each ~340 instructions for
// the whole wave.  Conservative by construction: spheres are inflated by 1 % + 1e-3 of the volume (the pose's rotation block is orthonormal to ~1e-6 only);
// more candidates than RC_BOUNDS_MAX: no bounds.  s_rb: RC_BOUNDS_WORDS words of LDS, s_rb[0..3] initialised (0, +inf bits, 0, 0) before the tables' barrier.
#define RC_BOUNDS_MAX 512
#define RC_BOUNDS_WORDS (4 + RC_BOUNDS_MAX)
struct RcFrustum { float ox, oy, oz; float r0, r1, r2, r3, r4, r5, r6, r7, r8; float aL, aR, bT, bB, nL, nR, nT, nB; };
__device__ __forceinline__ bool rc_sphere_in_frustum(const RcFrustum& f, float cx, float cy, float cz, float r, float& dist) {
  const float dx = cx - f.ox, dy = cy - f.oy, dz = cz - f.oz;
  const float px = f.r0 * dx + f.r3 * dy + f.r6 * dz, py = f.r1 * dx + f.r4 * dy + f.r7 * dz, pz = f.r2 * dx + f.r5 * dy + f.r8 * dz;     // R^T (c - org)
  dist = sqrtf(dx * dx + dy * dy + dz * dz);
  return pz + r > 0.f && (px - f.aL * pz) >= -r * f.nL && (f.aR * pz - px) >= -r * f.nR && (py - f.bT * pz) >= -r * f.nT && (f.bB * pz - py) >= -r * f.nB;
}
// the frustum of the pixel rectangle [x0, x1] x [y0, y1] (pixel centres, half a pixel of margin)
__device__ __forceinline__ void rc_set_window(RcFrustum& f, const KfCam& cam, int x0, int y0, int x1, int y1) {
  f.aL = ((float)x0 - 0.5f - cam.cx) / cam.fx; f.aR = ((float)x1 + 0.5f - cam.cx) / cam.fx;
  f.bT = ((float)y0 - 0.5f - cam.cy) / cam.fy; f.bB = ((float)y1 + 0.5f - cam.cy) / cam.fy;
  f.nL = sqrtf(1.f + f.aL * f.aL); f.nR = sqrtf(1.f + f.aR * f.aR); f.nT = sqrtf(1.f + f.bT * f.bT); f.nB = sqrtf(1.f + f.bB * f.bB);
}
// s_rb: [0] super-cell candidates, [1] / [2] the tile's bounds as bits, [3] spare, then the candidate list.
// (A third level -- every wave testing the 64 bricks of each candidate macro cell against its own 8x8 patch's frustum -- was built and measured: the tests cost
// more than the shorter march saves, 48.7 vs 46.2 us at 512^3 and 103 vs 85 us at 1024^3 where the bricks' bits do not fit into LDS; profiles/r05_raycast_bounds.txt)
__device__ __forceinline__ void rc_tile_bounds(const RaycastArgs& a, const unsigned* s_macro, const unsigned* s_super, const unsigned* s_meso, const unsigned* s_neg, bool neg_in_lds, const float* T,
                                               int tile_x, int tile_y, unsigned* s_rb, float& t_lo, float& t_hi) {
  const KfVolume& v = a.vol;
  RcFrustum f;
  f.ox = T[3]; f.oy = T[7]; f.oz = T[11];
  f.r0 = T[0]; f.r1 = T[1]; f.r2 = T[2]; f.r3 = T[4]; f.r4 = T[5]; f.r5 = T[6]; f.r6 = T[8]; f.r7 = T[9]; f.r8 = T[10];      // rows of R (camera -> world): R^T applied column-wise above
  const int x0 = tile_x * 32, y0 = tile_y * 16;
  rc_set_window(f, a.cam, x0, y0, min(x0 + 31, a.cam.cols - 1), min(y0 + 15, a.cam.rows - 1));
  const int nm = v.nm, ns = v.ns;
  const float cell = v.cell, slack = 1e-3f * v.size;
  const float r_super = 0.8660254f * 1.01f * (float)(KF_MACRO << KF_SUPER_SHIFT) * cell + slack, r_macro = 0.8660254f * 1.01f * (float)KF_MACRO * cell + slack;
  unsigned* list = s_rb + 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float lo = __builtin_huge_valf(), hi = 0.f;
  unsigned n = 0u;
  // small volumes (up to 256^3: 16^3 = 4096 meso cells of 16^3 voxels): the same scan over the MESO table -- cells half as wide, bounds twice as tight, where
  // a 256^3 volume has only 8^3 macro cells (RaycastArgs::bounds_meso; the table is in LDS)
  const int nq = v.nq;
  const bool by_meso = a.bounds_meso && a.meso_words != 0 && nq * nq * nq <= RAYCAST_THREADS * 16;
  if (a.tile_bounds != 2 && (by_meso || nm * nm * nm <= RAYCAST_THREADS * 16)) {
    // few cells (macro: up to 512^3 = 4096): every thread tests its share of them directly -- one barrier instead of two, no list.  A thread takes whole BYTES of the
    // table (one LDS read per eight cells, then only the set bits), cells numbered x-fastest
    const unsigned* tbl = by_meso ? s_meso : s_macro;
    const int nc = by_meso ? nq : nm;
    const float edge = by_meso ? 16.f : (float)KF_MACRO;
    const float r_cell = by_meso ? 0.8660254f * 1.01f * 16.f * cell + slack : r_macro;
    const int n_cells = nc * nc * nc;
    const float inv_nc = 1.0f / (float)nc;
    for (int byte = (int)threadIdx.x; byte * 8 < n_cells; byte += RAYCAST_THREADS) {
      unsigned bits = (tbl[byte >> 2] >> ((byte & 3) * 8)) & 0xFFu;
      while (bits) {
        const int m = byte * 8 + (int)__builtin_ctz(bits);
        bits &= bits - 1u;
        if (m >= n_cells) break;
        // m = (mz * nc + my) * nc + mx by two exact float quotients (m < 2^13, nc <= 20: the products are far from the rounding boundary after the +0.5)
        const int q = (int)(((float)m + 0.5f) * inv_nc), mx = m - q * nc, mz = (int)(((float)q + 0.5f) * inv_nc), my = q - mz * nc;
        float dist;
        if (rc_sphere_in_frustum(f, ((float)mx * edge + 0.5f * edge) * cell, ((float)my * edge + 0.5f * edge) * cell, ((float)mz * edge + 0.5f * edge) * cell, r_cell, dist)) {
          lo = fminf(lo, fmaxf(dist - r_cell, 0.f)); hi = fmaxf(hi, dist + r_cell);
        }
      }
    }
  } else {
    // level 0: non-empty super cells that meet the tile's frustum -> the list
    for (int s = (int)threadIdx.x; s < ns * ns * ns; s += RAYCAST_THREADS) {
      if (!rc_bit(s_super, (unsigned)s)) continue;
      const int sx = s % ns, sy = (s / ns) % ns, sz = s / (ns * ns);
      const float h = 0.5f * (float)(KF_MACRO << KF_SUPER_SHIFT);
      float dist;
      if (rc_sphere_in_frustum(f, ((float)(sx * (KF_MACRO << KF_SUPER_SHIFT)) + h) * cell, ((float)(sy * (KF_MACRO << KF_SUPER_SHIFT)) + h) * cell,
                               ((float)(sz * (KF_MACRO << KF_SUPER_SHIFT)) + h) * cell, r_super, dist)) {
        const unsigned k = atomicAdd(&s_rb[0], 1u);
        if (k < RC_BOUNDS_MAX) list[k] = (unsigned)s;
      }
    }
    __syncthreads();
    n = s_rb[0];
    if (n <= RC_BOUNDS_MAX) {
      // level 1: the macro cells of the listed super cells, one super cell per wave and round, one macro cell per lane
      for (unsigned k = (unsigned)wave; k < n; k += RAYCAST_THREADS / 64) {
        const int s = (int)list[k];
        const int mx = ((s % ns) << KF_SUPER_SHIFT) + (lane & 3), my = (((s / ns) % ns) << KF_SUPER_SHIFT) + ((lane >> 2) & 3), mz = ((s / (ns * ns)) << KF_SUPER_SHIFT) + (lane >> 4);
        if (mx >= nm || my >= nm || mz >= nm) continue;
        const unsigned mi = __umul24(__umul24((unsigned)mz, (unsigned)nm) + (unsigned)my, (unsigned)nm) + (unsigned)mx;
        if (!rc_bit(s_macro, mi)) continue;
        float dist;
        if (rc_sphere_in_frustum(f, ((float)(mx * KF_MACRO) + 0.5f * KF_MACRO) * cell, ((float)(my * KF_MACRO) + 0.5f * KF_MACRO) * cell, ((float)(mz * KF_MACRO) + 0.5f * KF_MACRO) * cell, r_macro, dist)) {
          lo = fminf(lo, fmaxf(dist - r_macro, 0.f)); hi = fmaxf(hi, dist + r_macro);
        }
      }
    }
  }
  // the few lanes that found a cell in sight put their extremes into LDS themselves (non-negative floats order like their bits): a dozen atomics per workgroup
  // are cheaper than twelve cross-lane shuffles per wave
  (void)lane;
  if (hi > 0.f) { atomicMin(&s_rb[1], __float_as_uint(lo)); atomicMax(&s_rb[2], __float_as_uint(hi)); }
  __syncthreads();
  if (n > RC_BOUNDS_MAX) { t_lo = 0.f; t_hi = __builtin_huge_valf(); return; }
  t_lo = __uint_as_float(s_rb[1]); t_hi = __uint_as_float(s_rb[2]);
}

// one 32x16 pixel tile (tile_x, tile_y) by the 512 threads of a workgroup; s_tables: the workgroup's dynamic LDS
// SPEC_COLOR (compile time; kf_raycast_volume_slab_cross_spec_color): the z-slab speculation carries a fourth word per pixel, interpolateColor at the
// vertex under the same ownership test as the gradient -- out_spec then has 4 words per pixel.  false: the code of every other form, unchanged.
// VIEW (compile time; kf_render_view): 0, or 1 + KF_VIEW_* -- the epilogue turns the lane's vertex, normal and colour into one display word in registers
// (view_pixel.h) and stores it to view_img; the float4 maps only where the caller gave buffers (a.out_v / a.out_n may be null), no colour map, no
// crossing words, no pyramid, no work counters.  a.cam is then the CALLER's camera: the grid, the tile bounds and the pixel index all follow it.
// VIEW == RC_VIEW_CROSS (compile time; kf_view_slab_cross): the z-slab march with speculation -- out_ta, own_ta and out_spec are all given, 3 or (SPEC_COLOR)
// 4 speculative words per pixel -- for the CALLER's camera, as a member's step of a merged view: the crossing words are the only stores; no model
// maps, no out_t / out_rgb, no pyramid, no work counters.
#define RC_VIEW_CROSS (-1)
template <bool SPEC_COLOR, int VIEW = 0>
__device__ __forceinline__ void raycast_tile(const RaycastArgs& a, int tile_x, int tile_y, unsigned* s_tables, unsigned* view_img = nullptr) {
  const RC_VOL& v = a.vol;
  constexpr bool CROSS = VIEW == RC_VIEW_CROSS;
  // Packed bit tables live in LDS so that the empty-space walk costs LDS reads instead of dependent L2 round trips: one bit
  // per 32^3-voxel macro cell and per 128^3-voxel super cell of the whole volume (KfVolume::macrobits, kept current by the
  // fusion pass with atomicOr: copied as they are), and -- when it fits -- one bit per stored 8^3 brick (KfVolume::negbits).
#ifdef KF_EXPERIMENTS
  const unsigned long long st0 = __builtin_amdgcn_s_memtime();
#endif
  const int skip_words = v.macro_words + v.super_words + a.meso_words;   // multiples of 4: everything is moved as uint4 (the meso table lies behind the other two: one copy)
  const unsigned* s_macro = s_tables;
  const unsigned* s_super = s_tables + v.macro_words;
  const unsigned* s_meso = s_tables + v.macro_words + v.super_words;
  const unsigned* s_neg = s_tables + skip_words;
  __shared__ unsigned s_rb[RC_BOUNDS_WORDS];
  if (threadIdx.x == 0) { s_rb[0] = 0u; s_rb[1] = 0x7F800000u; s_rb[2] = 0u; s_rb[3] = 0u; }
  {
    const uint4* msrc = reinterpret_cast<const uint4*>(v.macrobits);
    uint4* mdst = reinterpret_cast<uint4*>(s_tables);
    for (int i = threadIdx.x; i < skip_words / 4; i += RAYCAST_THREADS) mdst[i] = msrc[i];
    if (a.neg_words) {
      const uint4* nsrc = reinterpret_cast<const uint4*>(v.negbits);
      uint4* ndst = reinterpret_cast<uint4*>(s_tables + skip_words);
      for (int i = threadIdx.x; i < a.neg_words / 4; i += RAYCAST_THREADS) ndst[i] = nsrc[i];
    }
    __syncthreads();
  }
  const bool neg_in_lds = a.neg_words != 0;
  float tile_lo = 0.f, tile_hi = __builtin_huge_valf();
  if (a.tile_bounds) rc_tile_bounds(a, s_macro, s_super, s_meso, s_neg, neg_in_lds, a.pose ? a.pose : a.pose_val.m, tile_x, tile_y, s_rb, tile_lo, tile_hi);     // (uniform)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // a workgroup is a 32x16 pixel tile, a wave an 8x8 patch of it
  const int x = tile_x * 32 + (wave & 3) * 8 + (lane & 7), y = tile_y * 16 + (wave >> 2) * 8 + (lane >> 3);
  // (pixels outside the image and the timing experiment "half the rays" -- latency- or throughput-bound? -- march nothing but stay for the epilogue)
  const bool live = x < a.cam.cols && y < a.cam.rows && !(KF_EXP_MODE(a) == 2 && ((tile_x + tile_y) & 1));
  float4 out_v = make_float4(0.f, 0.f, 0.f, 0.f), out_n = make_float4(0.f, 0.f, 0.f, 0.f);
  auto march_pixel = [&]() {
  const int pix = y * a.cam.cols + x;
  const float inf = __builtin_huge_valf();
  uchar4 out_c = make_uchar4(0, 0, 0, 0);
  float t_cross = inf, t_cross_prev = 0.f, out_alpha = 0.f;
  const float* T = a.pose ? a.pose : a.pose_val.m;
  float3 org, dir, cam_dir;
  rc_pixel_ray(a.cam, T, x, y, org, dir, cam_dir);
  const float S = v.size;
  float tmin, tmax;
  rc_ray_interval(S, a.near_plane, a.far_plane, org, dir, cam_dir, tmin, tmax);
  const float ref_tmin = tmin, ref_tmax = tmax;
#ifdef KF_EXPERIMENTS
  unsigned long long st1 = __builtin_amdgcn_s_memtime(), st2 = st1;
#endif
  int n_iter = 0, n_samp = 0, n_macro = 0;
  if (tmin < tmax) {
    // raySample :65-119
    const int R = v.res;
    const KfRecip rS = kf_recip(S);                                       // `worldPos.x*_resolution.x/_size.x`: shared divisor
    const KfRecip rcell = kf_recip(v.cell);
    float t = tmin, t_prev = tmin;
    float last_sdf = 0.f; bool have_last = true;
    RcRay ray; ray.org = org; ray.dir = dir; ray.inv_dir = kf3(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
    // z-slabs: only samples inside the owned layers can be this context's candidates, so the march is clipped to the ray's
    // passage through them (one cell of margin on either side); the parameter still reaches the first such sample by the
    // reference's repeated addition, and the previous sample is fetched lazily like after any other skip
    float t_end = tmax, t_first = tmin;
    if (v.own_z0 > 0 || v.own_z1 < R) {
      const float za = ((float)(v.own_z0 - 1) * v.cell - org.z) * ray.inv_dir.z, zb = ((float)(v.own_z1 + 1) * v.cell - org.z) * ray.inv_dir.z;
      const float t_in = fminf(za, zb), t_out = fmaxf(za, zb);
      t_end = fminf(tmax, t_out);
      t_first = fmaxf(tmin, fminf(t_in - 1e-6f * fabsf(t_in), t_end));
    }
    if (t < t_first) { RC_ADVANCE(t, t_prev, a.inc, t_first); have_last = false; }
    // the tile's bounds (rc_tile_bounds): nothing before tile_lo or from tile_hi on can be a crossing's negative sample; the long first walk in closed form
    t_end = fminf(t_end, tile_hi);
    if (t < tile_lo && t < t_end) { kf_ray_advance(t, t_prev, a.inc, fminf(tile_lo, t_end)); have_last = false; }
    rc_march(a, v, s_macro, s_super, s_meso, s_neg, neg_in_lds, ray, rS, t_end, t, t_prev, have_last, last_sdf, t_cross, t_cross_prev, n_iter, n_samp, n_macro);
#ifdef KF_EXPERIMENTS
    st2 = __builtin_amdgcn_s_memtime();
#endif
    // The crossing is evaluated HERE, after the march loop, not inside it: lanes of a wave meet their crossings at
    // different iterations, and inside the loop the 64-gather evaluation would run once per distinct iteration with a
    // handful of active lanes each time.  After the loop every lane that found a crossing evaluates together.
    if (t_cross < inf && KF_EXP_MODE(a) != 1) {
      const float3 pos = kf_add(org, kf_scale(dir, t_cross)), last_pos = kf_add(org, kf_scale(dir, t_cross_prev));
      float ftdt, ft; bool ok_cur, ok_last;
      RC_INTERP_SDF_PAIR(v, pos, last_pos, rS, rcell, ok_cur, ftdt, ok_last, ft);
      // :87-88 `break` on either failure.  One gradient evaluation serves both outputs: the model maps (vertex, normal) -- or, z-slabs, the speculative normal.
      // z-slabs: the vertex org + dir * alpha may lie ANYWHERE along the ray -- alpha = t - inc * f(t) / (f(t) - f(t - inc)) extrapolates without bound when the
      // two interpolated values nearly agree (an isolated negative voxel at a silhouette) -- so its gradient taps are not this slab's to read unless the vertex
      // lies in the layers it OWNS (the owner's part of k_slab_ray_normals, for this context's own crossing: same vertex, same layer test, same gradient;
      // last_pos is the march's own previous sample -- what that kernel finds by replaying the chain of additions); alpha leaves either way.
      if (ok_cur && ok_last) {
        const float alpha = t_cross - a.inc * ftdt / (ftdt - ft);
        const float3 vtx = kf_add(org, kf_scale(dir, alpha));
        bool want = true;
        if (CROSS || a.out_ta) {
          out_alpha = alpha;
          int gzv = kf_f2i(kf_div(vtx.z * (float)v.res, rS));
          gzv = max(0, min(gzv, v.res - 1));
          want = (CROSS || a.out_spec != nullptr) && __float_as_uint(alpha) != 0u && gzv >= v.own_z0 && gzv < v.own_z1;
          // the colour at the vertex (:91-92), before and independently of the gradient: it stays whether or not a normal is found
          if (SPEC_COLOR && want) { uchar4 c = make_uchar4(0, 0, 0, 0); RC_INTERP_COLOR(v, vtx, c); out_c = c; }
        } else if (a.has_color) { uchar4 c = make_uchar4(0, 0, 0, 0); RC_INTERP_COLOR(v, vtx, c); out_c = c; }
        float3 grad;
        if (want && gradient_for_point_either<RC_GRAD_BATCH, RC_GRAD_ROUNDS>(a.shared_grad, ((tile_x + tile_y + wave) & 1) != 0, v, last_pos, vtx, rS, rcell, grad)) {
          out_n = make_float4(grad.x, grad.y, grad.z, 0.f);
          if (!CROSS && !a.out_ta) { out_v = make_float4(vtx.x, vtx.y, vtx.z, 1.0f); out_alpha = alpha; }
        }
      }
    } else if (t_cross < inf) out_v = make_float4(t_cross, 0.f, 0.f, 1.f);
  }
#ifdef KF_EXPERIMENTS
  if (KF_EXP_MODE(a) == 3) {                                                // diagnostics: shader-clock ticks of the three phases, loop trips
    const unsigned long long st3 = __builtin_amdgcn_s_memtime();
    out_v = make_float4((float)(st1 - st0), (float)(st2 - st1), (float)(st3 - st2), (float)n_iter);
    out_n = make_float4((float)n_samp, (float)(n_macro & 0xFFFF), (float)(n_macro >> 16), 0.f);
  }
#endif
  if (VIEW > 0) {
    if (a.out_v) a.out_v[pix] = out_v;
    if (a.out_n) a.out_n[pix] = out_n;
    view_img[pix] = kf_view_pixel<(VIEW > 0 ? VIEW - 1 : 0)>(out_v, out_n, out_c, org);     // the eye is the pose's translation: the ray origin
  } else
  if (CROSS || a.out_ta) {
    const unsigned long long word = ((unsigned long long)__float_as_uint(t_cross) << 32) | (unsigned long long)(t_cross < inf ? __float_as_uint(out_alpha) : 0u);
    a.out_ta[pix] = word;
    if (SPEC_COLOR) {
      a.own_ta[pix] = word; a.out_spec[4 * pix] = out_n.x; a.out_spec[4 * pix + 1] = out_n.y; a.out_spec[4 * pix + 2] = out_n.z;
      a.out_spec[4 * pix + 3] = __uint_as_float(rc_color_word(out_c));
    } else
    if (CROSS || a.out_spec) { a.own_ta[pix] = word; a.out_spec[3 * pix] = out_n.x; a.out_spec[3 * pix + 1] = out_n.y; a.out_spec[3 * pix + 2] = out_n.z; }
  }
  else { a.out_v[pix] = out_v; a.out_n[pix] = out_n; }
  if (VIEW == 0 && a.work) {
    // what the REFERENCE's march reads for this ray (raycastingVolume.cu:65-119): one voxel per sample from t_min up to the
    // crossing (or t_max); a crossing is evaluated with 2 + 6 trilinear look-ups of 8 voxels each
    const float t_stop = t_cross < inf ? t_cross : ref_tmax;
    const float n_s = (ref_tmin < ref_tmax) ? floorf((t_stop - ref_tmin) / a.inc) + 1.f : 0.f;
    const float steps = kf_wave_sum(n_s), hits = kf_wave_sum(t_cross < inf ? 1.f : 0.f);
    if ((threadIdx.x & 63) == 0) {
      const unsigned sh = ((unsigned)(tile_y * 61 + tile_x) * 8u + (threadIdx.x >> 6)) & 63u;
      atomicAdd(&a.work->rc_steps[sh * 16], (unsigned long long)steps);
      atomicAdd(&a.work->rc_hits[sh * 16], (unsigned long long)hits);
    }
  }
  if (VIEW == 0 && a.out_t) a.out_t[pix] = t_cross;
  if (VIEW == 0 && a.has_color) a.out_rgb[pix] = out_c;
  };
  if (live) march_pixel();
  // Levels 1 and 2 of the model maps' pyramids, which the NEXT frame's tracker reads first (ICP.cpp:57-60): a 32x16 tile holds whole 2x2 and
  // 4x4 blocks, so the workgroup that produced the texels averages them itself -- through the LDS the bit tables occupied until its last wave
  // left the march -- and the tracker's pyramid launch (a pass over four maps, ~8 us) has nothing left to do.
  if (VIEW == 0 && a.pyr.v1) {                                                 // uniform
    __syncthreads();                                                         // every wave is done with the tables
    float4* s_v = reinterpret_cast<float4*>(s_tables);
    float4* s_n = s_v + 32 * 16, *s1_v = s_n + 32 * 16, *s1_n = s1_v + 16 * 8;
    const int li = ((wave >> 2) * 8 + (lane >> 3)) * 32 + (wave & 3) * 8 + (lane & 7);
    s_v[li] = out_v; s_n[li] = out_n;
    kf_tile_pyramid<32, 16>(a.pyr, tile_x * 32, tile_y * 16, (int)threadIdx.x, s_v, s_n, s1_v, s1_n, [] { __syncthreads(); });
  }
}

// What a raycast launch writes: the context's model maps (KF_RC_OUT_MAPS: no pointer set), or what RaycastArgs calls out_t / out_v / out_n (KF_RC_OUT_T), out_ta
// (KF_RC_OUT_TA), out_ta / own_ta / out_spec (KF_RC_OUT_TA_SPEC; with `color` the speculation carries the colour word too: 4 words per pixel, a kernel of its own)
struct RaycastOut { int output; bool color; float* t; float4* v; float4* n; unsigned long long* ta; unsigned long long* own_ta; float* spec; };

// The kernel's arguments, the LDS tables' placement (lds: bytes the plain kernel needs) and the form's description, all from the same quantities
static int raycast_args(kf_ctx* c, int has_color, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                        float near_plane, float far_plane, const RaycastOut& out, RaycastArgs& a, kf_raycast_form& form, size_t& lds) {
  const bool maps = out.output == KF_RC_OUT_MAPS;
  RC_VOL_ASSIGN(a.vol, c->vol); a.cam = kf_to_cam(cam);
  kf_pose_arg(c, transform, a.pose, a.pose_val);
  memset(&a.pyr, 0, sizeof(a.pyr));
  const bool model_pyr = kf_switch(KF_SW_RAYCAST_PYRAMID) && maps && c->levels == 3;      // the model maps themselves, stock pyramid depth
  if (model_pyr) kf_pyr_arg(a.pyr, c->model_v + 1, c->model_n + 1, c->cols, c->rows);
  a.out_v = out.v ? out.v : c->model_v[0]; a.out_n = out.n ? out.n : c->model_n[0]; a.out_rgb = c->raycast_rgb; a.out_t = out.t; a.out_ta = out.ta;
  a.own_ta = out.own_ta; a.out_spec = out.spec;
  a.inc = rp->ray_increment; a.near_plane = near_plane; a.far_plane = far_plane; a.has_color = has_color;
  a.exp_mode = KF_EXP_ENV(RAYCAST_EXP);
  a.tile_bounds = kf_switch(KF_SW_RAYCAST_BOUNDS); a.bounds_meso = kf_switch(KF_SW_RAYCAST_BOUNDS_MESO); a.shared_grad = rc_shared_grad_for(c->vol);
  a.work = c->count_work ? c->counters : nullptr;
  size_t macro_bytes = (size_t)(c->vol.macro_words + c->vol.super_words) * 4;
  const size_t neg_bytes = kf_negbit_words(c->n_stored_bricks) * 4, meso_bytes = (size_t)c->vol.meso_words * 4;
  if (macro_bytes > RAYCAST_LDS_BYTES) return KF_ERR_STATE;
  a.meso_words = (kf_switch(KF_SW_RAYCAST_MESO) && macro_bytes + meso_bytes <= RAYCAST_LDS_BYTES) ? c->vol.meso_words : 0;      // (2048^3: 256 KiB, no)
  macro_bytes += (size_t)a.meso_words * 4;                  // from here on: everything in front of the per-brick bits
  a.neg_words = (kf_switch(KF_SW_RAYCAST_NEG_LDS) && macro_bytes + neg_bytes <= RAYCAST_LDS_BYTES) ? (int)(neg_bytes / 4) : 0;
  const size_t pyr_lds = model_pyr ? (size_t)(32 * 16 + 16 * 8) * 2 * sizeof(float4) : 0;      // the tile's two maps and their level 1
  lds = macro_bytes + (size_t)a.neg_words * 4 > pyr_lds ? macro_bytes + (size_t)a.neg_words * 4 : pyr_lds;
  // (kf_get_raycast_form) what this launch is; the kernel and the grid are noted where it is launched
  memset(&form, 0, sizeof(form));
  form.output = out.output;
  form.tile_bounds = a.tile_bounds ? 1 : 0;
  if (a.tile_bounds) {                                      // rc_tile_bounds' choice, from the same quantities
    const int nq = c->vol.nq, nm = c->vol.nm;
    const bool by_meso = a.bounds_meso && a.meso_words != 0 && nq * nq * nq <= RAYCAST_THREADS * 16;
    form.bounds_path = (a.tile_bounds != 2 && by_meso) ? KF_RC_BOUNDS_MESO : (a.tile_bounds != 2 && nm * nm * nm <= RAYCAST_THREADS * 16) ? KF_RC_BOUNDS_MACRO : KF_RC_BOUNDS_LIST;
  }
  form.meso_lds = a.meso_words != 0; form.neg_lds = a.neg_words != 0;
  form.shared_grad = a.shared_grad & 255; form.view_half = a.shared_grad >> 8; form.pyramid = model_pyr ? 1 : 0;
  form.calls = c->raycast_form.calls + 1;
  return 0;
}

static bool view_cam_ok(const kf_camera_params* cam) {
  return cam && cam->cols >= 1 && cam->cols <= 4096 && cam->rows >= 1 && cam->rows <= 4096 && cam->fx != 0.f && cam->fy != 0.f &&
         cam->fx == cam->fx && cam->fy == cam->fy && cam->cx == cam->cx && cam->cy == cam->cy;
}
