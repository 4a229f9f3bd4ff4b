// group.hip -- slab groups (include/hybkf_group.h): N z-slab contexts and the per-frame collective sequence of the slab merge, over RCCL
// (one member per device) or on one device (KF_GROUP_LOCAL, whose two all-reduces are the streaming kernels below).  Uses only the public
// kf_* ABI of libhybkf.so.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <math.h>
#include <string.h>
#include <new>
#include <utility>
#include <vector>
#include "hybkf_group.h"

#define KF_GROUP_BLOCK 256

// ---- LOCAL backend: the two all-reduces as kernels ------------------------------------------------------------------------------------------
// Each lane moves 16 B per member per step (global_load_dwordx4): the M loads of a step are independent and issued back to back, then reduced
// in registers and stored once.  No LDS, no atomics; grid-stride over the buffer with a grid of a few workgroups per CU.  The odd tail (a
// buffer whose length is not a multiple of 16 B) is done by the first lanes of workgroup 0.
struct GroupReduceArgs {
  const void* src[KF_GROUP_MAX_MEMBERS];
  void* dst;
  unsigned n16;     // 16-byte units
  unsigned tail;    // elements past n16 * 16 B (u64: 0 or 1; u32: 0..3)
};

// crossing words: the first crossing along each ray wins (positive floats order like their bits; +inf << 32 where a member met none)
template <int M>
__global__ void __launch_bounds__(KF_GROUP_BLOCK) k_group_min_u64(GroupReduceArgs a) {
  const unsigned stride = gridDim.x * KF_GROUP_BLOCK;
  for (unsigned i = blockIdx.x * KF_GROUP_BLOCK + threadIdx.x; i < a.n16; i += stride) {
    ulonglong2 v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = ((const ulonglong2*)a.src[m])[i];
    ulonglong2 r = v[0];
#pragma unroll
    for (int m = 1; m < M; ++m) { r.x = v[m].x < r.x ? v[m].x : r.x; r.y = v[m].y < r.y ? v[m].y : r.y; }
    ((ulonglong2*)a.dst)[i] = r;
  }
  if (blockIdx.x == 0 && threadIdx.x < a.tail) {
    const unsigned e = a.n16 * 2 + threadIdx.x;
    unsigned long long r = ((const unsigned long long*)a.src[0])[e];
#pragma unroll
    for (int m = 1; m < M; ++m) { const unsigned long long x = ((const unsigned long long*)a.src[m])[e]; r = x < r ? x : r; }
    ((unsigned long long*)a.dst)[e] = r;
  }
}

// normal candidates (3 words per pixel; a colour group: 4, the colour word last): exactly one member contributes non-zero bits per pixel, so the integer
// sum is that member's bits (-0.0 included).  The kernel reduces a flat run of words: nothing in it knows the stride
template <int M>
__global__ void __launch_bounds__(KF_GROUP_BLOCK) k_group_sum_u32(GroupReduceArgs a) {
  const unsigned stride = gridDim.x * KF_GROUP_BLOCK;
  for (unsigned i = blockIdx.x * KF_GROUP_BLOCK + threadIdx.x; i < a.n16; i += stride) {
    uint4 v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = ((const uint4*)a.src[m])[i];
    uint4 r = v[0];
#pragma unroll
    for (int m = 1; m < M; ++m) { r.x += v[m].x; r.y += v[m].y; r.z += v[m].z; r.w += v[m].w; }
    ((uint4*)a.dst)[i] = r;
  }
  if (blockIdx.x == 0 && threadIdx.x < a.tail) {
    const unsigned e = a.n16 * 4 + threadIdx.x;
    unsigned r = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) r += ((const unsigned*)a.src[m])[e];
    ((unsigned*)a.dst)[e] = r;
  }
}

#define KF_GROUP_DISPATCH(kernel, members, grid, stream, args)                                                                               \
  switch (members) {                                                                                                                        \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 5: hipLaunchKernelGGL(kernel<5>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 6: hipLaunchKernelGGL(kernel<6>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 7: hipLaunchKernelGGL(kernel<7>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 8: hipLaunchKernelGGL(kernel<8>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 9: hipLaunchKernelGGL(kernel<9>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                             \
    case 10: hipLaunchKernelGGL(kernel<10>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
    case 11: hipLaunchKernelGGL(kernel<11>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
    case 12: hipLaunchKernelGGL(kernel<12>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
    case 13: hipLaunchKernelGGL(kernel<13>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
    case 14: hipLaunchKernelGGL(kernel<14>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
    case 15: hipLaunchKernelGGL(kernel<15>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
    default: hipLaunchKernelGGL(kernel<16>, grid, dim3(KF_GROUP_BLOCK), 0, stream, args); break;                                           \
  }

// ---- the group ----------------------------------------------------------------------------------------------------------------------------------
struct kf_group {
  int backend = KF_GROUP_LOCAL;
  uint32_t n = 0, halo = 0, rank = 0, world = 1;
  kf_config base;
  kf_group_params p;
  uint32_t cuts[KF_GROUP_MAX_MEMBERS + 1];
  int32_t dev[KF_GROUP_MAX_MEMBERS];
  kf_ctx* m[KF_GROUP_MAX_MEMBERS] = {};
  ncclComm_t comm[KF_GROUP_MAX_MEMBERS] = {};
  // per member: crossing words (all-reduced in place on RCCL), a second copy of them (RCCL only: LOCAL never overwrites its words), the
  // speculative normals, the normal candidates (all-reduced in place on RCCL), the depth frame of a host-fed frame (one per device)
  uint64_t* ta[KF_GROUP_MAX_MEMBERS] = {};
  uint64_t* ta_own[KF_GROUP_MAX_MEMBERS] = {};
  float* spec[KF_GROUP_MAX_MEMBERS] = {};
  float* cand[KF_GROUP_MAX_MEMBERS] = {};
  uint16_t* depth[KF_GROUP_MAX_MEMBERS] = {};
  // a colour group (kf_group_create_color): speculation and candidates carry 4 words per pixel, members integrate / extract with colour, and a
  // host-fed frame's BGR image has a buffer per device like the depth frame
  bool color = false;
  int angle_weight = 0;
  uint32_t words = 3;
  uint8_t* rgb[KF_GROUP_MAX_MEMBERS] = {};
  // LOCAL: the group stream and the two group buffers every member reads after a reduction
  hipStream_t stream = nullptr;
  uint64_t* ta_min = nullptr;
  float* cand_sum = nullptr;
  int grid = 0;
  // merged views (kf_group_render_view): buffers of the group's own, so a view never touches a frame's; they hold view_cap_px pixels (g->words
  // words per candidate pixel), grow on demand and mirror the frame's set -- per member ta / spec / cand, on RCCL ta_own, on LOCAL the two group buffers
  uint64_t* view_ta[KF_GROUP_MAX_MEMBERS] = {};
  uint64_t* view_ta_own[KF_GROUP_MAX_MEMBERS] = {};
  float* view_spec[KF_GROUP_MAX_MEMBERS] = {};
  float* view_cand[KF_GROUP_MAX_MEMBERS] = {};
  uint64_t* view_ta_min = nullptr;
  float* view_cand_sum = nullptr;
  size_t view_cap_px = 0;
  // the moving volume (kf_group_shift_volume): per member the feed buffer its move reads and, on RCCL, the send buffer its packs go to; sized to the
  // plan, grown on demand.  world_cuts: the whole layout -- the group's own cuts, or on RCCL_RANK what the first shift gathered from the ranks
  uint8_t* feed[KF_GROUP_MAX_MEMBERS] = {};
  uint8_t* sendb[KF_GROUP_MAX_MEMBERS] = {};
  size_t feed_cap[KF_GROUP_MAX_MEMBERS] = {}, send_cap[KF_GROUP_MAX_MEMBERS] = {};
  std::vector<uint32_t> world_cuts;
  bool failed = false;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;   // merge timers: a pool of at most KF_GROUP_MAX_TIMED_FRAMES, ev_used of them recorded since the last read
  size_t ev_used = 0;
};

namespace {
struct DeviceGuard {   // the caller's current device comes back on every return
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};

int fail(kf_group* g, int st) { if (st) g->failed = true; return st; }
int nccl_status(ncclResult_t r) { return r == ncclSuccess ? 0 : KF_GROUP_ERR_RCCL; }
hipStream_t member_stream(kf_group* g, uint32_t i) { return g->backend == KF_GROUP_LOCAL ? g->stream : (hipStream_t)kf_stream(g->m[i]); }

// pipeline.slab_halo_layers with the arithmetic of libhybkf's own halo check (ceilf(inc / cell) + 2), rounded up to whole bricks
uint32_t needed_halo(const kf_config* base, const kf_group_params* p) {
  const float cell = base->volume.size_m / (float)base->volume.resolution;
  const int need = (int)ceilf(p->raycast.ray_increment / cell) + 2;
  return (uint32_t)((need + 7) / 8 * 8);
}

int validate(const kf_config* base, const kf_group_params* p, int backend, uint32_t members, const uint32_t* z_cuts, const int32_t* devices,
             uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world, bool color) {
  if (!base || !p || !z_cuts) return KF_GROUP_ERR_ARG;
  if (members < 1 || members > KF_GROUP_MAX_MEMBERS) return KF_GROUP_ERR_ARG;
  if (backend != KF_GROUP_LOCAL && backend != KF_GROUP_RCCL_ALL && backend != KF_GROUP_RCCL_RANK) return KF_GROUP_ERR_ARG;
  const uint32_t res = base->volume.resolution;
  if (res == 0 || res % 8 || !(base->volume.size_m > 0.f) || !(p->raycast.ray_increment > 0.f)) return KF_GROUP_ERR_ARG;
  if (backend == KF_GROUP_RCCL_RANK) {
    // one member: z_cuts = this rank's own [z0, z1).  The ranks' slabs tile the volume in rank order, so rank 0 starts at 0, the last rank
    // ends at the resolution, and every other rank lies strictly inside
    if (members != 1 || !unique_id || world < 1 || rank >= world || world > res / 8) return KF_GROUP_ERR_ARG;
    const uint32_t z0 = z_cuts[0], z1 = z_cuts[1];
    if (z0 % 8 || z1 % 8 || z0 >= z1 || z1 > res) return KF_GROUP_ERR_ARG;
    if ((rank == 0) != (z0 == 0) || (rank == world - 1) != (z1 == res)) return KF_GROUP_ERR_ARG;
  } else {
    // the whole layout: members + 1 cuts from 0 to the resolution
    if (z_cuts[0] != 0 || z_cuts[members] != res) return KF_GROUP_ERR_ARG;
    for (uint32_t i = 0; i < members; ++i)
      if (z_cuts[i + 1] <= z_cuts[i] || z_cuts[i + 1] % 8) return KF_GROUP_ERR_ARG;
  }
  if (halo != 0 && halo < needed_halo(base, p)) return KF_GROUP_ERR_ARG;
  if (color ? (base->has_color != 1 || base->rgb_camera.cols == 0 || base->rgb_camera.rows == 0) : base->has_color != 0) return KF_GROUP_ERR_ARG;
  if (base->depth_camera.cols == 0 || base->depth_camera.rows == 0) return KF_GROUP_ERR_ARG;
  for (uint32_t i = 0; i < members; ++i) {
    const int32_t di = devices ? devices[i] : base->device;
    if (di < 0) return KF_GROUP_ERR_ARG;
    for (uint32_t j = 0; j < i; ++j) {
      const int32_t dj = devices ? devices[j] : base->device;
      if (backend == KF_GROUP_LOCAL && di != dj) return KF_GROUP_ERR_ARG;        // one device, one stream
      if (backend == KF_GROUP_RCCL_ALL && di == dj) return KF_GROUP_ERR_ARG;     // ncclCommInitAll refuses a repeated device
    }
  }
  return 0;
}

int group_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? 0 : KF_GROUP_ERR_ALLOC; }

void release(kf_group* g) {
  for (uint32_t i = 0; i < g->n; ++i) {
    hipSetDevice(g->dev[i]);
    if (g->m[i]) kf_synchronize(g->m[i]);
  }
  for (uint32_t i = 0; i < g->n; ++i) {
    hipSetDevice(g->dev[i]);
    if (g->comm[i]) ncclCommDestroy(g->comm[i]);
    if (g->m[i]) kf_destroy(g->m[i]);            // (a member on the group stream returns to its own stream first)
    void* bufs[] = {g->ta[i], g->ta_own[i], g->spec[i], g->cand[i], g->depth[i], g->rgb[i], g->view_ta[i], g->view_ta_own[i], g->view_spec[i], g->view_cand[i],
                    g->feed[i], g->sendb[i]};
    for (void* b : bufs) if (b) hipFree(b);
  }
  if (g->n) hipSetDevice(g->dev[0]);
  for (auto& e : g->ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (g->ta_min) hipFree(g->ta_min);
  if (g->cand_sum) hipFree(g->cand_sum);
  if (g->view_ta_min) hipFree(g->view_ta_min);
  if (g->view_cand_sum) hipFree(g->view_cand_sum);
  if (g->stream) { hipStreamSynchronize(g->stream); hipStreamDestroy(g->stream); }
}

int build(kf_group* g, const uint8_t* unique_id) {
  const size_t npx = (size_t)g->base.depth_camera.cols * g->base.depth_camera.rows;
  int st = 0;
  if (g->backend == KF_GROUP_RCCL_ALL) {
    if ((st = nccl_status(ncclCommInitAll(g->comm, (int)g->n, g->dev)))) return st;
  } else if (g->backend == KF_GROUP_RCCL_RANK) {
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) == KF_GROUP_UNIQUE_ID_BYTES, "ncclUniqueId size");
    memcpy(&id, unique_id, sizeof(id));
    if (hipSetDevice(g->dev[0]) != hipSuccess) return KF_GROUP_ERR_ARG;
    if ((st = nccl_status(ncclCommInitRank(&g->comm[0], (int)g->world, id, (int)g->rank)))) return st;
  }
  for (uint32_t i = 0; i < g->n; ++i) {
    if ((st = (int)hipSetDevice(g->dev[i]))) return st;
    kf_config c = g->base;
    c.device = g->dev[i]; c.slab_z_begin = g->cuts[i]; c.slab_z_end = g->cuts[i + 1]; c.slab_halo = g->halo;
    if ((st = kf_create(&c, &g->m[i]))) return st;
    if ((st = hipSetDevice(g->dev[i]))) return st;
    if ((st = group_alloc((void**)&g->ta[i], npx * 8))) return st;
    if ((st = group_alloc((void**)&g->spec[i], npx * 4 * g->words))) return st;
    if ((st = group_alloc((void**)&g->cand[i], npx * 4 * g->words))) return st;
    if (g->backend != KF_GROUP_LOCAL && (st = group_alloc((void**)&g->ta_own[i], npx * 8))) return st;
    if ((g->backend != KF_GROUP_LOCAL || i == 0) && (st = group_alloc((void**)&g->depth[i], npx * 2))) return st;
    if (g->color && (g->backend != KF_GROUP_LOCAL || i == 0) &&
        (st = group_alloc((void**)&g->rgb[i], (size_t)g->base.rgb_camera.cols * g->base.rgb_camera.rows * 3))) return st;
    kf_mat44 pose0;                                   // HybKinectfu::init: identity, camera at the centre of the front face, trunc_min in front of it
    memset(&pose0, 0, sizeof(pose0));
    pose0.m[0] = pose0.m[5] = pose0.m[10] = pose0.m[15] = 1.f;
    pose0.m[3] = pose0.m[7] = (float)(g->base.volume.size_m / 2.0);
    pose0.m[11] = -g->p.trunc_min;
    if ((st = kf_set_pose(g->m[i], &pose0))) return st;
  }
  if (g->backend == KF_GROUP_LOCAL) {
    if ((st = (int)hipSetDevice(g->dev[0]))) return st;
    if ((st = (int)hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking))) return st;
    for (uint32_t i = 0; i < g->n; ++i) if ((st = kf_set_stream(g->m[i], g->stream))) return st;   // one stream: ordering is implicit
    if ((st = group_alloc((void**)&g->ta_min, npx * 8))) return st;
    if ((st = group_alloc((void**)&g->cand_sum, npx * 4 * g->words))) return st;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->dev[0]) != hipSuccess || cus <= 0) cus = 256;
    g->grid = 4 * cus;
  }
  return 0;
}

// words: the MIN over `elems` 64-bit crossing words, else the integer SUM over `elems` 32-bit candidate words; src: one buffer per member
int reduce_local(kf_group* g, bool words, size_t elems, const void* const* src, void* dst) {
  GroupReduceArgs a;
  memset(&a, 0, sizeof(a));
  for (uint32_t i = 0; i < g->n; ++i) a.src[i] = src[i];
  a.dst = dst;
  const size_t per16 = words ? 2 : 4;
  a.n16 = (unsigned)(elems / per16);
  a.tail = (unsigned)(elems % per16);
  const unsigned need = (a.n16 + KF_GROUP_BLOCK - 1) / KF_GROUP_BLOCK;
  const dim3 grid(need == 0 ? 1 : (need < (unsigned)g->grid ? need : (unsigned)g->grid));
  if (words) { KF_GROUP_DISPATCH(k_group_min_u64, g->n, grid, g->stream, a) }
  else { KF_GROUP_DISPATCH(k_group_sum_u32, g->n, grid, g->stream, a) }
  return (int)hipGetLastError();
}

// steps 7 and 9 of the frame in the group's kind: the colour forms carry the fourth word
int member_normals(kf_group* g, uint32_t i, const uint64_t* ta_min, const uint64_t* ta_own) {
  const kf_group_params& p = g->p;
  return g->color ? kf_slab_ray_normals_color(g->m[i], nullptr, &p.raycast, &g->base.depth_camera, p.trunc_min, p.trunc_max, ta_min, ta_own, g->spec[i], g->cand[i])
                  : kf_slab_ray_normals_spec(g->m[i], nullptr, &p.raycast, &g->base.depth_camera, p.trunc_min, p.trunc_max, ta_min, ta_own, g->spec[i], g->cand[i]);
}
int member_maps(kf_group* g, uint32_t i, const uint64_t* ta_min, const float* cand) {
  return g->color ? kf_set_model_maps_rays_color(g->m[i], nullptr, &g->base.depth_camera, ta_min, cand)
                  : kf_set_model_maps_rays(g->m[i], nullptr, &g->base.depth_camera, ta_min, cand);
}

// step 5 of the frame in the group's kind
int member_cross(kf_group* g, uint32_t i) {
  const kf_group_params& p = g->p;
  const kf_camera_params* cam = &g->base.depth_camera;
  uint64_t* own = g->backend == KF_GROUP_LOCAL ? g->ta[i] : g->ta_own[i];
  return g->color ? kf_raycast_volume_slab_cross_spec_color(g->m[i], nullptr, &p.raycast, cam, p.trunc_min, p.trunc_max, g->ta[i], own, g->spec[i])
                  : kf_raycast_volume_slab_cross_spec(g->m[i], nullptr, &p.raycast, cam, p.trunc_min, p.trunc_max, g->ta[i], own, g->spec[i]);
}

// steps 6-9 of the frame
int merge(kf_group* g) {
  const kf_camera_params* cam = &g->base.depth_camera;
  const uint32_t n = g->n;
  const size_t npx = (size_t)cam->cols * cam->rows;
  int st = 0;
  if (g->backend == KF_GROUP_LOCAL) {
    if ((st = reduce_local(g, true, npx, (const void* const*)g->ta, g->ta_min))) return st;
    for (uint32_t i = 0; i < n; ++i)
      if ((st = member_normals(g, i, g->ta_min, g->ta[i]))) return st;
    if ((st = reduce_local(g, false, g->words * npx, (const void* const*)g->cand, g->cand_sum))) return st;
    for (uint32_t i = 0; i < n; ++i)
      if ((st = member_maps(g, i, g->ta_min, g->cand_sum))) return st;
    return 0;
  }
  if ((st = nccl_status(ncclGroupStart()))) return st;
  for (uint32_t i = 0; i < n && !st; ++i)
    st = nccl_status(ncclAllReduce(g->ta[i], g->ta[i], npx, ncclUint64, ncclMin, g->comm[i], member_stream(g, i)));
  const int st_end = nccl_status(ncclGroupEnd());
  if (st || st_end) return st ? st : st_end;
  for (uint32_t i = 0; i < n; ++i) {
    if ((st = hipSetDevice(g->dev[i]))) return st;
    if ((st = member_normals(g, i, g->ta[i], g->ta_own[i]))) return st;
  }
  if ((st = nccl_status(ncclGroupStart()))) return st;
  for (uint32_t i = 0; i < n && !st; ++i)
    st = nccl_status(ncclAllReduce(g->cand[i], g->cand[i], g->words * npx, ncclInt32, ncclSum, g->comm[i], member_stream(g, i)));
  const int st_end2 = nccl_status(ncclGroupEnd());
  if (st || st_end2) return st ? st : st_end2;
  for (uint32_t i = 0; i < n; ++i) {
    if ((st = hipSetDevice(g->dev[i]))) return st;
    if ((st = member_maps(g, i, g->ta[i], g->cand[i]))) return st;
  }
  return 0;
}

// dev_bgr / host_bgr: a colour group's BGR frame, where the depth frame lies (both null for a colourless group)
int frame(kf_group* g, const uint16_t* const* dev_mm, const uint16_t* host_mm, uint32_t frame_id, const uint8_t* const* dev_bgr = nullptr,
          const uint8_t* host_bgr = nullptr) {
  const kf_group_params& p = g->p;
  const kf_camera_params* cam = &g->base.depth_camera;
  const kf_camera_params* rcam = &g->base.rgb_camera;
  const size_t bytes = (size_t)cam->cols * cam->rows * sizeof(uint16_t), rgb_bytes = (size_t)rcam->cols * rcam->rows * 3;
  int st = 0;
  for (uint32_t i = 0; i < g->n; ++i) {
    kf_ctx* c = g->m[i];
    if ((st = hipSetDevice(g->dev[i]))) return st;
    const uint16_t* mm = dev_mm ? dev_mm[i] : nullptr;
    if (host_mm) {
      const uint32_t slot = g->backend == KF_GROUP_LOCAL ? 0 : i;     // once per device
      if (slot == i && (st = (int)hipMemcpyAsync(g->depth[slot], host_mm, bytes, hipMemcpyHostToDevice, member_stream(g, i)))) return st;
      mm = g->depth[slot];
    }
    if ((st = kf_set_depth_mm_device(c, mm, cam->cols, cam->rows))) return st;
    if (g->color) {
      const uint8_t* bgr = dev_bgr ? dev_bgr[i] : nullptr;
      if (host_bgr) {
        const uint32_t slot = g->backend == KF_GROUP_LOCAL ? 0 : i;     // once per device
        if (slot == i && (st = (int)hipMemcpyAsync(g->rgb[slot], host_bgr, rgb_bytes, hipMemcpyHostToDevice, member_stream(g, i)))) return st;
        bgr = g->rgb[slot];
      }
      if ((st = kf_set_rgb_device(c, bgr, rcam->cols, rcam->rows))) return st;
    }
    if ((st = kf_preprocess(c, p.trunc_min, p.trunc_max, p.sigma_pixel, p.sigma_depth, cam))) return st;
    if ((st = kf_icp_track(c, frame_id, &p.icp, cam))) return st;
    if ((st = g->color ? kf_integrate_volume(c, 1, g->angle_weight, nullptr, &p.integrate, cam, rcam) : kf_integrate_volume(c, 0, 0, nullptr, &p.integrate, cam, cam))) return st;
    if ((st = member_cross(g, i))) return st;
  }
  hipEvent_t e1 = nullptr;
  if (g->timing && g->ev_used < KF_GROUP_MAX_TIMED_FRAMES) {          // (a full pool: this frame's merge goes untimed until the next read)
    if ((st = hipSetDevice(g->dev[0]))) return st;
    if (g->ev_used == g->ev.size()) {
      hipEvent_t a, b;
      if ((st = hipEventCreate(&a))) return st;
      if ((st = hipEventCreate(&b))) { hipEventDestroy(a); return st; }
      g->ev.emplace_back(a, b);
    }
    if ((st = hipEventRecord(g->ev[g->ev_used].first, member_stream(g, 0)))) return st;
    e1 = g->ev[g->ev_used].second;
  }
  if ((st = merge(g))) return st;
  if (e1) {
    if ((st = hipSetDevice(g->dev[0]))) return st;
    if ((st = hipEventRecord(e1, member_stream(g, 0)))) return st;
    ++g->ev_used;
  }
  return 0;
}

// ---- merged views ---------------------------------------------------------------------------------------------------------------------------
bool view_cam_ok(const kf_camera_params* cam) {      // kf_render_view's limits
  return cam && cam->cols >= 1 && cam->cols <= 4096 && cam->rows >= 1 && cam->rows <= 4096 && cam->fx != 0.f && cam->fy != 0.f &&
         cam->fx == cam->fx && cam->fy == cam->fy && cam->cx == cam->cx && cam->cy == cam->cy;
}

// the view buffers for npx pixels: growing frees the old ones (hipFree waits for the work that still uses them)
int view_reserve(kf_group* g, size_t npx) {
  if (npx <= g->view_cap_px) return 0;
  int st = 0;
  g->view_cap_px = 0;
  for (uint32_t i = 0; i < g->n; ++i) {
    if ((st = (int)hipSetDevice(g->dev[i]))) return st;
    void** bufs[] = {(void**)&g->view_ta[i], (void**)&g->view_ta_own[i], (void**)&g->view_spec[i], (void**)&g->view_cand[i]};
    for (void** b : bufs) if (*b) { hipFree(*b); *b = nullptr; }
    if ((st = group_alloc((void**)&g->view_ta[i], npx * 8))) return st;
    if ((st = group_alloc((void**)&g->view_spec[i], npx * 4 * g->words))) return st;
    if ((st = group_alloc((void**)&g->view_cand[i], npx * 4 * g->words))) return st;
    if (g->backend != KF_GROUP_LOCAL && (st = group_alloc((void**)&g->view_ta_own[i], npx * 8))) return st;
  }
  if (g->backend == KF_GROUP_LOCAL) {
    if ((st = (int)hipSetDevice(g->dev[0]))) return st;
    if (g->view_ta_min) { hipFree(g->view_ta_min); g->view_ta_min = nullptr; }
    if (g->view_cand_sum) { hipFree(g->view_cand_sum); g->view_cand_sum = nullptr; }
    if ((st = group_alloc((void**)&g->view_ta_min, npx * 8))) return st;
    if ((st = group_alloc((void**)&g->view_cand_sum, npx * 4 * g->words))) return st;
  }
  g->view_cap_px = npx;
  return 0;
}

// the five steps of kf_group_render_view; the arguments have passed kf_group_view_validate
int view(kf_group* g, int mode, const kf_mat44* pose, const kf_camera_params* cam, float near_plane, float far_plane, float* dev_v, float* dev_n) {
  const int color = mode == KF_VIEW_COLOR ? 1 : 0;
  const uint32_t n = g->n, words = color ? 4 : 3;                 // (words <= g->words: KF_VIEW_COLOR only on a colour group)
  const size_t npx = (size_t)cam->cols * cam->rows;
  const kf_raycast_params* rp = &g->p.raycast;
  const bool local = g->backend == KF_GROUP_LOCAL;
  int st = 0;
  if ((st = view_reserve(g, npx))) return st;
  for (uint32_t i = 0; i < n; ++i) {
    if ((st = hipSetDevice(g->dev[i]))) return st;
    if ((st = kf_view_slab_cross(g->m[i], color, pose, cam, rp, near_plane, far_plane, g->view_ta[i], local ? g->view_ta[i] : g->view_ta_own[i], g->view_spec[i]))) return st;
  }
  if (local) {
    if ((st = reduce_local(g, true, npx, (const void* const*)g->view_ta, g->view_ta_min))) return st;
  } else {
    if ((st = nccl_status(ncclGroupStart()))) return st;
    for (uint32_t i = 0; i < n && !st; ++i)
      st = nccl_status(ncclAllReduce(g->view_ta[i], g->view_ta[i], npx, ncclUint64, ncclMin, g->comm[i], member_stream(g, i)));
    const int st_end = nccl_status(ncclGroupEnd());
    if (st || st_end) return st ? st : st_end;
  }
  for (uint32_t i = 0; i < n; ++i) {
    if ((st = hipSetDevice(g->dev[i]))) return st;
    if ((st = kf_view_slab_normals(g->m[i], color, pose, cam, rp, near_plane, far_plane, local ? g->view_ta_min : g->view_ta[i],
                                   local ? g->view_ta[i] : g->view_ta_own[i], g->view_spec[i], g->view_cand[i]))) return st;
  }
  if (local) {
    if ((st = reduce_local(g, false, words * npx, (const void* const*)g->view_cand, g->view_cand_sum))) return st;
  } else {
    if ((st = nccl_status(ncclGroupStart()))) return st;
    for (uint32_t i = 0; i < n && !st; ++i)
      st = nccl_status(ncclAllReduce(g->view_cand[i], g->view_cand[i], words * npx, ncclInt32, ncclSum, g->comm[i], member_stream(g, i)));
    const int st_end = nccl_status(ncclGroupEnd());
    if (st || st_end) return st ? st : st_end;
  }
  if ((st = hipSetDevice(g->dev[0]))) return st;
  return kf_view_from_rays(g->m[0], mode, pose, cam, local ? g->view_ta_min : g->view_ta[0], local ? g->view_cand_sum : g->view_cand[0], words, dev_v, dev_n);
}

// ---- the moving volume ----------------------------------------------------------------------------------------------------------------------
// stored voxel layers of the member that owns [z0, z1) with `halo` layers around them (kf_create's arithmetic: whole bricks, clamped to the volume)
void stored_layers(uint32_t res, uint32_t z0, uint32_t z1, uint32_t halo, uint32_t* s0, uint32_t* s1) {
  const uint32_t h = (halo + 7) / 8 * 8;
  *s0 = z0 > h ? z0 - h : 0;
  *s1 = z1 + h < res ? z1 + h : res;
}
bool layout_ok(uint32_t res, uint32_t members, const uint32_t* cuts) {
  if (res == 0 || res % 8 || members < 1 || members > res / 8 || !cuts || cuts[0] != 0 || cuts[members] != res) return false;
  for (uint32_t i = 0; i < members; ++i) if (cuts[i + 1] <= cuts[i] || cuts[i + 1] % 8) return false;
  return true;
}

int grow(uint8_t** buf, size_t* cap, size_t bytes) {      // (hipFree waits for the work that still reads the old buffer)
  if (bytes <= *cap) return 0;
  if (*buf) { hipFree(*buf); *buf = nullptr; *cap = 0; }
  const int st = group_alloc((void**)buf, bytes);
  if (!st) *cap = bytes;
  return st;
}

// RCCL_RANK: the ranks' (z0, z1), gathered once (blocking) and kept; LOCAL / RCCL_ALL: the group's own cuts
int world_layout(kf_group* g) {
  if (!g->world_cuts.empty()) return 0;
  if (g->backend != KF_GROUP_RCCL_RANK || g->world == 1) {
    g->world_cuts.assign(g->cuts, g->cuts + g->n + 1);
    return 0;
  }
  int st = 0;
  uint32_t* dev = nullptr;
  std::vector<uint32_t> pairs(2 * (size_t)g->world);
  if ((st = (int)hipSetDevice(g->dev[0]))) return st;
  if ((st = group_alloc((void**)&dev, pairs.size() * sizeof(uint32_t)))) return st;
  hipStream_t s = member_stream(g, 0);
  st = (int)hipMemcpyAsync(dev + 2 * g->rank, g->cuts, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  if (!st) st = nccl_status(ncclAllGather(dev + 2 * g->rank, dev, 2, ncclUint32, g->comm[0], s));
  if (!st) st = (int)hipMemcpyAsync(pairs.data(), dev, pairs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (!st) st = (int)hipStreamSynchronize(s);
  hipFree(dev);
  if (st) return st;
  std::vector<uint32_t> cuts(g->world + 1);
  cuts[0] = pairs[0];
  for (uint32_t r = 0; r < g->world; ++r) {
    if (pairs[2 * r] != cuts[r]) return KF_GROUP_ERR_STATE;       // the ranks' slabs do not tile the volume in rank order
    cuts[r + 1] = pairs[2 * r + 1];
  }
  if (!layout_ok(g->base.volume.resolution, g->world, cuts.data())) return KF_GROUP_ERR_STATE;
  g->world_cuts = cuts;
  return 0;
}

// the three steps of kf_group_shift_volume; the arguments have passed its checks
int shift(kf_group* g, int32_t dx, int32_t dy, int32_t dz) {
  int st = 0;
  if ((st = world_layout(g))) return st;
  const uint32_t world = (uint32_t)g->world_cuts.size() - 1;
  const bool local = g->backend == KF_GROUP_LOCAL, by_rank = g->backend == KF_GROUP_RCCL_RANK;
  std::vector<kf_group_transfer> plan(2 * (size_t)world + 2);
  int n_plan = kf_group_shift_plan(g->base.volume.resolution, world, g->world_cuts.data(), g->halo, dz, plan.data(), (uint32_t)plan.size());
  if (n_plan > (int)plan.size()) {
    plan.resize((size_t)n_plan);
    n_plan = kf_group_shift_plan(g->base.volume.resolution, world, g->world_cuts.data(), g->halo, dz, plan.data(), (uint32_t)plan.size());
  }
  if (n_plan < 0) return KF_GROUP_ERR_STATE;
  plan.resize((size_t)n_plan);
  // member r of the layout is member `at(r)` of this process (or none of its members)
  auto at = [&](uint32_t r) -> int { return by_rank ? (r == g->rank ? 0 : -1) : (int)r; };
  const size_t lb = kf_slab_layer_bytes(g->m[0]);
  uint32_t need0[KF_GROUP_MAX_MEMBERS], need1[KF_GROUP_MAX_MEMBERS];
  size_t fed[KF_GROUP_MAX_MEMBERS] = {}, sent[KF_GROUP_MAX_MEMBERS] = {};
  for (uint32_t i = 0; i < g->n; ++i)
    if ((st = kf_slab_shift_needs(g->m[i], dz, &need0[i], &need1[i]))) return st;
  for (const kf_group_transfer& t : plan) {                      // the plan feeds every member exactly what it needs: checked before a byte moves
    const int to = at(t.to_member), from = at(t.from_member);
    if (to >= 0) {
      if (t.bz_begin != need0[to] + fed[to] || t.bz_end > need1[to]) return KF_GROUP_ERR_STATE;
      fed[to] += t.bz_end - t.bz_begin;
    }
    if (from >= 0) sent[from] += t.bz_end - t.bz_begin;
  }
  for (uint32_t i = 0; i < g->n; ++i) {
    if (fed[i] != need1[i] - need0[i]) return KF_GROUP_ERR_STATE;
    if ((st = (int)hipSetDevice(g->dev[i]))) return st;
    if ((st = grow(&g->feed[i], &g->feed_cap[i], fed[i] * lb))) return st;
    if (!local && (st = grow(&g->sendb[i], &g->send_cap[i], sent[i] * lb))) return st;
  }
  // 1. every owner packs what the plan sends: LOCAL straight into the receiver's feed, RCCL into its send buffer in plan order
  size_t off[KF_GROUP_MAX_MEMBERS] = {};
  for (const kf_group_transfer& t : plan) {
    const int from = at(t.from_member);
    if (from < 0) continue;
    uint8_t* dst = local ? g->feed[t.to_member] + (size_t)(t.bz_begin - need0[t.to_member]) * lb : g->sendb[from] + off[from];
    off[from] += (size_t)(t.bz_end - t.bz_begin) * lb;
    if ((st = (int)hipSetDevice(g->dev[from]))) return st;
    if ((st = kf_slab_pack_layers(g->m[from], t.bz_begin, t.bz_end, dst))) return st;
  }
  // 2. the exchange.  LOCAL: none -- one stream, and every pack above precedes every move below
  if (!local && !plan.empty()) {
    for (uint32_t i = 0; i < g->n; ++i) off[i] = 0;
    if ((st = nccl_status(ncclGroupStart()))) return st;
    for (size_t k = 0; k < plan.size() && !st; ++k) {
      const kf_group_transfer& t = plan[k];
      const int from = at(t.from_member), to = at(t.to_member);
      const size_t bytes = (size_t)(t.bz_end - t.bz_begin) * lb;
      if (from >= 0) {
        st = nccl_status(ncclSend(g->sendb[from] + off[from], bytes, ncclUint8, (int)t.to_member, g->comm[from], member_stream(g, (uint32_t)from)));
        off[from] += bytes;
      }
      if (to >= 0 && !st)
        st = nccl_status(ncclRecv(g->feed[to] + (size_t)(t.bz_begin - need0[to]) * lb, bytes, ncclUint8, (int)t.from_member, g->comm[to], member_stream(g, (uint32_t)to)));
    }
    const int st_end = nccl_status(ncclGroupEnd());
    if (st || st_end) return st ? st : st_end;
  }
  // 3. the move
  for (uint32_t i = 0; i < g->n; ++i) {
    if ((st = (int)hipSetDevice(g->dev[i]))) return st;
    if ((st = kf_shift_slab(g->m[i], dx, dy, dz, need0[i] < need1[i] ? g->feed[i] : nullptr, need0[i], need1[i]))) return st;
  }
  return 0;
}
}  // namespace

extern "C" {

const char* kf_group_error_string(int s) {
  if (s == KF_GROUP_ERR_RCCL) return "RCCL call failed";
  return kf_error_string(s);
}

int kf_group_unique_id(uint8_t out[128]) {
  if (!out) return KF_GROUP_ERR_ARG;
  ncclUniqueId id;
  const int st = nccl_status(ncclGetUniqueId(&id));
  if (!st) memcpy(out, &id, sizeof(id));
  return st;
}

int kf_group_validate(const kf_config* base, const kf_group_params* params, int backend, uint32_t members, const uint32_t* z_cuts,
                      const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world) {
  return validate(base, params, backend, members, z_cuts, devices, halo, unique_id, rank, world, false);
}

int kf_group_validate_color(const kf_config* base, const kf_group_params* params, int use_angle_weight_color, int backend, uint32_t members,
                            const uint32_t* z_cuts, const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world) {
  (void)use_angle_weight_color;                          // any value is a valid switch
  return validate(base, params, backend, members, z_cuts, devices, halo, unique_id, rank, world, true);
}

static int group_create(const kf_config* base, const kf_group_params* params, bool color, int use_angle_weight_color, int backend, uint32_t members,
                        const uint32_t* z_cuts, const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world, kf_group** out) {
  if (!out) return KF_GROUP_ERR_ARG;
  *out = nullptr;
  int st = validate(base, params, backend, members, z_cuts, devices, halo, unique_id, rank, world, color);
  if (st) return st;
  DeviceGuard guard;
  kf_group* g = new (std::nothrow) kf_group();
  if (!g) return KF_GROUP_ERR_ALLOC;
  g->backend = backend; g->n = members; g->base = *base; g->p = *params;
  g->color = color; g->angle_weight = use_angle_weight_color ? 1 : 0; g->words = color ? 4 : 3;
  g->p.icp.pyramid_levels = base->pyramid_levels;
  g->halo = halo ? halo : needed_halo(base, params);
  g->rank = backend == KF_GROUP_RCCL_RANK ? rank : 0;
  g->world = backend == KF_GROUP_RCCL_RANK ? world : members;
  for (uint32_t i = 0; i <= members; ++i) g->cuts[i] = z_cuts[i];
  for (uint32_t i = 0; i < members; ++i) g->dev[i] = devices ? devices[i] : base->device;
  if ((st = build(g, unique_id))) { release(g); delete g; return st; }
  *out = g;
  return 0;
}

int kf_group_create(const kf_config* base, const kf_group_params* params, int backend, uint32_t members, const uint32_t* z_cuts,
                    const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world, kf_group** out) {
  return group_create(base, params, false, 0, backend, members, z_cuts, devices, halo, unique_id, rank, world, out);
}

int kf_group_create_color(const kf_config* base, const kf_group_params* params, int use_angle_weight_color, int backend, uint32_t members,
                          const uint32_t* z_cuts, const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world,
                          kf_group** out) {
  return group_create(base, params, true, use_angle_weight_color, backend, members, z_cuts, devices, halo, unique_id, rank, world, out);
}

int kf_group_destroy(kf_group* g) {
  if (!g) return KF_GROUP_ERR_ARG;
  DeviceGuard guard;
  release(g);
  delete g;
  return 0;
}

int kf_group_members(kf_group* g, uint32_t* members, uint32_t* halo) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (members) *members = g->n;
  if (halo) *halo = g->halo;
  return 0;
}

int kf_group_frame(kf_group* g, const uint16_t* mm, int on_device, uint32_t cols, uint32_t rows, uint32_t frame_id) {
  if (!g || !mm || cols != g->base.depth_camera.cols || rows != g->base.depth_camera.rows) return KF_GROUP_ERR_ARG;
  if (g->failed || g->color) return KF_GROUP_ERR_STATE;      // (a colour group takes kf_group_frame_color: nothing is enqueued, the group stays usable)
  DeviceGuard guard;
  if (!on_device) return fail(g, frame(g, nullptr, mm, frame_id));
  const uint16_t* per[KF_GROUP_MAX_MEMBERS];
  for (uint32_t i = 0; i < g->n; ++i) per[i] = mm;
  return fail(g, frame(g, per, nullptr, frame_id));
}

int kf_group_frame_members(kf_group* g, const uint16_t* const* dev_mm, uint32_t cols, uint32_t rows, uint32_t frame_id) {
  if (!g || !dev_mm || cols != g->base.depth_camera.cols || rows != g->base.depth_camera.rows) return KF_GROUP_ERR_ARG;
  for (uint32_t i = 0; i < g->n; ++i) if (!dev_mm[i]) return KF_GROUP_ERR_ARG;
  if (g->failed || g->color) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  return fail(g, frame(g, dev_mm, nullptr, frame_id));
}

int kf_group_frame_color(kf_group* g, const uint16_t* mm, const uint8_t* bgr, int on_device, uint32_t cols, uint32_t rows, uint32_t frame_id) {
  if (!g || !mm || !bgr || cols != g->base.depth_camera.cols || rows != g->base.depth_camera.rows) return KF_GROUP_ERR_ARG;
  if (g->failed || !g->color) return KF_GROUP_ERR_STATE;     // (a colourless group takes kf_group_frame)
  DeviceGuard guard;
  if (!on_device) return fail(g, frame(g, nullptr, mm, frame_id, nullptr, bgr));
  const uint16_t* per[KF_GROUP_MAX_MEMBERS];
  const uint8_t* per_bgr[KF_GROUP_MAX_MEMBERS];
  for (uint32_t i = 0; i < g->n; ++i) { per[i] = mm; per_bgr[i] = bgr; }
  return fail(g, frame(g, per, nullptr, frame_id, per_bgr, nullptr));
}

int kf_group_frame_members_color(kf_group* g, const uint16_t* const* dev_mm, const uint8_t* const* dev_bgr, uint32_t cols, uint32_t rows, uint32_t frame_id) {
  if (!g || !dev_mm || !dev_bgr || cols != g->base.depth_camera.cols || rows != g->base.depth_camera.rows) return KF_GROUP_ERR_ARG;
  for (uint32_t i = 0; i < g->n; ++i) if (!dev_mm[i] || !dev_bgr[i]) return KF_GROUP_ERR_ARG;
  if (g->failed || !g->color) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  return fail(g, frame(g, dev_mm, nullptr, frame_id, dev_bgr, nullptr));
}

int kf_group_track_result(kf_group* g, kf_track_result* out, int check_lockstep) {
  if (!g || !out) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  int st = (int)hipSetDevice(g->dev[0]);
  if (!st) st = kf_read_track_result(g->m[0], out);
  if (st || !check_lockstep) return fail(g, st);
  kf_volume_stats s0;
  if ((st = kf_get_fusion_counters(g->m[0], &s0))) return fail(g, st);
  for (uint32_t i = 1; i < g->n; ++i) {
    kf_track_result r;
    kf_volume_stats s;
    if ((st = (int)hipSetDevice(g->dev[i])) || (st = kf_read_track_result(g->m[i], &r)) || (st = kf_get_fusion_counters(g->m[i], &s)))
      return fail(g, st);
    if (memcmp(r.pose.m, out->pose.m, sizeof(r.pose.m)) || r.tracked != out->tracked || r.status != out->status ||
        s.frames_fused != s0.frames_fused || s.frames_lost != s0.frames_lost)
      return KF_GROUP_ERR_STATE;
  }
  return 0;
}

int kf_group_set_pose(kf_group* g, const kf_mat44* pose) {
  if (!g || !pose) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  for (uint32_t i = 0; i < g->n; ++i) {
    int st = (int)hipSetDevice(g->dev[i]);
    if (!st) st = kf_set_pose(g->m[i], pose);
    if (st) return fail(g, st);
  }
  return 0;
}

int kf_group_member(kf_group* g, uint32_t i, kf_ctx** out) {
  if (!g || !out || i >= g->n) return KF_GROUP_ERR_ARG;
  *out = g->m[i];
  return 0;
}

void* kf_group_stream(kf_group* g, uint32_t i) {
  if (!g || i >= g->n) return nullptr;
  return (void*)member_stream(g, i);
}

int kf_group_view_validate(int color_group, int mode, const kf_camera_params* view_cam) {
  if (mode != KF_VIEW_NORMALS && mode != KF_VIEW_SHADED && mode != KF_VIEW_COLOR) return KF_GROUP_ERR_ARG;
  if (!view_cam_ok(view_cam)) return KF_GROUP_ERR_ARG;
  if (mode == KF_VIEW_COLOR && !color_group) return KF_GROUP_ERR_STATE;
  return 0;
}

int kf_group_render_view(kf_group* g, int mode, const kf_mat44* pose, const kf_camera_params* view_cam, float near_plane, float far_plane,
                         float* dev_v, float* dev_n) {
  if (!g) return KF_GROUP_ERR_ARG;
  const int st = kf_group_view_validate(g->color ? 1 : 0, mode, view_cam);
  if (st) return st;                                         // (nothing is enqueued, the group stays usable)
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  return fail(g, view(g, mode, pose, view_cam, near_plane, far_plane, dev_v, dev_n));
}

int kf_group_view_size(kf_group* g, uint32_t* cols, uint32_t* rows) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  return kf_view_size(g->m[0], cols, rows);                  // (KF_ERR_STATE before a view)
}

const uint8_t* kf_group_view_device(kf_group* g) { return (g && !g->failed) ? kf_view_device(g->m[0]) : nullptr; }

int kf_group_read_view(kf_group* g, uint8_t* dst, size_t dst_bytes) {
  if (!g || !dst) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  int st = (int)hipSetDevice(g->dev[0]);
  if (!st) st = kf_read_view(g->m[0], dst, dst_bytes);
  return (st == KF_GROUP_ERR_ARG || st == KF_GROUP_ERR_STATE) ? st : fail(g, st);      // (a buffer too small, no view yet: refusals, the group stays usable)
}

int kf_group_marching_cubes(kf_group* g, float threshold) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  for (uint32_t i = 0; i < g->n; ++i) {
    int st = (int)hipSetDevice(g->dev[i]);
    if (!st) st = kf_marching_cubes(g->m[i], g->color ? 1 : 0, threshold);
    if (st) return fail(g, st);
  }
  return 0;
}

int kf_group_triangle_count(kf_group* g, uint32_t* count) {
  if (!g || !count) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  uint64_t total = 0;
  for (uint32_t i = 0; i < g->n; ++i) {
    uint32_t c = 0;
    int st = (int)hipSetDevice(g->dev[i]);
    if (!st) st = kf_triangle_count(g->m[i], &c);
    if (st) return fail(g, st);
    total += c;
  }
  if (total > 0xFFFFFFFFull) return KF_GROUP_ERR_STATE;
  *count = (uint32_t)total;
  return 0;
}

int kf_group_read_triangles(kf_group* g, kf_triangle* dst, uint32_t first, uint32_t count) {
  if (!g || (!dst && count)) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  uint64_t base = 0, lo = first, hi = (uint64_t)first + count;
  for (uint32_t i = 0; i < g->n && lo < hi; ++i) {
    uint32_t c = 0;
    int st = (int)hipSetDevice(g->dev[i]);
    if (!st) st = kf_triangle_count(g->m[i], &c);
    if (st) return fail(g, st);
    const uint64_t b0 = base, b1 = base + c;
    base = b1;
    if (lo >= b1) continue;                              // this member's triangles lie before the range
    const uint64_t take = (hi < b1 ? hi : b1) - lo;
    if ((st = kf_read_triangles(g->m[i], dst + (lo - first), (uint32_t)(lo - b0), (uint32_t)take))) return fail(g, st);
    lo += take;
  }
  return lo == hi ? 0 : KF_GROUP_ERR_ARG;                // the range ran past the last triangle
}

int kf_group_merge_timing(kf_group* g, int on) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  g->timing = on != 0;
  return 0;
}

int kf_group_read_merge_ms(kf_group* g, float* total_ms, uint32_t* frames) {
  if (!g || !total_ms || !frames) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  float total = 0.f;
  int st = (int)hipSetDevice(g->dev[0]);
  for (size_t k = 0; k < g->ev_used && !st; ++k) {
    float ms = 0.f;
    if (!(st = (int)hipEventSynchronize(g->ev[k].second)) && !(st = (int)hipEventElapsedTime(&ms, g->ev[k].first, g->ev[k].second))) total += ms;
  }
  if (st) return fail(g, st);
  *total_ms = total;
  *frames = (uint32_t)g->ev_used;
  g->ev_used = 0;
  return 0;
}

int kf_group_shift_plan(uint32_t resolution, uint32_t members, const uint32_t* z_cuts, uint32_t halo, int32_t dz, kf_group_transfer* out, uint32_t cap) {
  if (!layout_ok(resolution, members, z_cuts) || dz % 8 || (!out && cap)) return -1;
  int n = 0;
  for (uint32_t to = 0; to < members; ++to) {
    uint32_t s0, s1, lo, hi;
    stored_layers(resolution, z_cuts[to], z_cuts[to + 1], halo, &s0, &s1);
    if (kf_slab_needs(resolution, s0, s1, dz, &lo, &hi)) return -1;      // the member's need range: libhybkf's own rule (kf_slab_shift_needs)
    for (uint32_t from = 0; from < members && lo < hi; ++from) {      // the owners in layer order: the need range cut by who owns each layer
      const uint32_t o1 = z_cuts[from + 1] / 8;                        // the owner of layer lo is the first member whose slab ends behind it
      if (o1 <= lo) continue;
      const uint32_t end = hi < o1 ? hi : o1;
      if ((uint32_t)n < cap) { out[n].from_member = from; out[n].to_member = to; out[n].bz_begin = lo; out[n].bz_end = end; }
      ++n;
      lo = end;
    }
  }
  return n;
}

int kf_group_shift_volume(kf_group* g, int32_t dx, int32_t dy, int32_t dz) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (dx % 8 || dy % 8 || dz % 8) return KF_GROUP_ERR_ARG;
  int32_t org[3];
  if (kf_volume_origin(g->m[0], org)) return KF_GROUP_ERR_ARG;
  const int32_t d[3] = {dx, dy, dz};
  for (int k = 0; k < 3; ++k) { const int64_t o = (int64_t)org[k] + d[k]; if (o > INT32_MAX || o < INT32_MIN) return KF_GROUP_ERR_ARG; }
  if (g->failed) return KF_GROUP_ERR_STATE;
  if (dx == 0 && dy == 0 && dz == 0) return 0;
  DeviceGuard guard;
  return fail(g, shift(g, dx, dy, dz));
}

int kf_group_raycast(kf_group* g) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  for (uint32_t i = 0; i < g->n; ++i) {
    int st = (int)hipSetDevice(g->dev[i]);
    if (!st) st = member_cross(g, i);
    if (st) return fail(g, st);
  }
  return fail(g, merge(g));
}

int kf_group_volume_origin(kf_group* g, int32_t origin_vox[3]) {
  if (!g || !origin_vox) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  int st = kf_volume_origin(g->m[0], origin_vox);
  for (uint32_t i = 1; i < g->n && !st; ++i) {
    int32_t o[3];
    if (!(st = kf_volume_origin(g->m[i], o)) && memcmp(o, origin_vox, sizeof(o))) return KF_GROUP_ERR_STATE;
  }
  return st;
}

int kf_group_synchronize(kf_group* g) {
  if (!g) return KF_GROUP_ERR_ARG;
  if (g->failed) return KF_GROUP_ERR_STATE;
  DeviceGuard guard;
  for (uint32_t i = 0; i < g->n; ++i) {
    int st = (int)hipSetDevice(g->dev[i]);
    if (!st) st = kf_synchronize(g->m[i]);
    if (st) return fail(g, st);
  }
  return 0;
}

}  // extern "C"
