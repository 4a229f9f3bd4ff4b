// meshparts.hip -- the connected parts of the welded mesh (weld.hip), labelled and dropped on the device.  The reference has nothing of
// the kind (MeshData knows removeIsolatedVertices, src/utils/mesh/meshData.cpp:320-356, and no part); the rule is written out in
// include/hybkf.h and restated sequentially in host/mesh_parts.hpp.
//
// Two vertices are connected when one face names both; a part's label is its smallest vertex index.  Labelling runs in rounds, the way the
// weld's cell selection does, and never as a lock-free union-find: within one launch a plain load may never see another compute unit's
// store, so a `find` that re-reads parent[] until a compare-and-swap succeeds can spin for ever.  Here no loop waits for another lane:
//   hook  : one lane per face, labels read as the previous launch left them (all of them roots: parent[l] == l).  For the pairs (a, b) and
//           (a, c) whose labels differ: atomicMin(&parent[larger label], smaller label).  parent[x] <= x always.
//   jump  : parent[v] <- parent[parent[v]], a few launches (every chain at most an eighth of its length, whatever a lane happens to read:
//           any value parent[] ever held is an ancestor), then one chase per vertex down its strictly descending chain to the root:
//           label[v] <- root, parent[v] <- root.  A lane writes its own words only.
//   loop  : the host reads one word per round -- did a hook find two labels -- and stops at zero.  Every non-final round joins two roots,
//           so there are at most n_v rounds.
// At the fixed point every face's vertices share a label, every label is a root, and a root is the minimum of its tree: the labels are the
// parts' smallest indices whatever the scheduling.  Sizes are integer atomicAdds per face, the largest part one 64-bit atomicMax of
// (size << 32) | ~label (ties: the smaller label), the counts flags and scans.  The drop is flags -> scans -> gathers into a second set of
// mesh buffers, which then changes places with the first.
#include "kf_internal.h"
#include "weld_mesh.h"
#include "scan.h"

#define PARTS_NONE 0xFFFFFFFFu
#define PARTS_DOUBLINGS 3
// device words: [0] a hook found two labels, [1] parts with a face, [2] orphans, [3] kept parts, [4, 5] the largest part's 64-bit key, [6] kept vertices, [7] kept faces
enum { PW_CHANGED = 0, PW_PARTS = 1, PW_ORPHANS = 2, PW_KEPT = 3, PW_BEST = 4, PW_NV = 6, PW_NF = 7, PW_WORDS = 8 };

// ---- labels --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_parts_init(unsigned n_v, unsigned* __restrict__ label, unsigned* __restrict__ parent, unsigned* __restrict__ size) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_v; i += (size_t)gridDim.x * 256u) { label[i] = (unsigned)i; parent[i] = (unsigned)i; size[i] = 0u; }
}
__global__ void __launch_bounds__(256) k_parts_hook(unsigned n_f, const unsigned* __restrict__ faces, const unsigned* __restrict__ label, unsigned* parent, unsigned* words) {
  bool any = false;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_f; i += (size_t)gridDim.x * 256u) {
    const unsigned ra = label[faces[3 * i]], rb = label[faces[3 * i + 1]], rc = label[faces[3 * i + 2]];
    if (ra != rb) { atomicMin(&parent[ra > rb ? ra : rb], ra < rb ? ra : rb); any = true; }
    if (ra != rc) { atomicMin(&parent[ra > rc ? ra : rc], ra < rc ? ra : rc); any = true; }
  }
  const unsigned long long m = __ballot(any);
  if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&words[PW_CHANGED], 1u);
}
__global__ void __launch_bounds__(256) k_parts_jump(unsigned n_v, unsigned* parent) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_v; i += (size_t)gridDim.x * 256u) {
    const unsigned p = parent[i];
    if (p == (unsigned)i) continue;
    const unsigned pp = parent[p];
    if (pp != p) parent[i] = pp;
  }
}
// the chase: bounded by the chain it reads (strictly descending indices)
__global__ void __launch_bounds__(256) k_parts_root(unsigned n_v, unsigned* parent, unsigned* __restrict__ label) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_v; i += (size_t)gridDim.x * 256u) {
    unsigned x = parent[i];
    for (;;) { const unsigned p = parent[x]; if (p >= x) break; x = p; }
    label[i] = x; parent[i] = x;
  }
}

// ---- sizes and counts ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_parts_sizes(unsigned n_f, const unsigned* __restrict__ faces, const unsigned* __restrict__ label, unsigned* size) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_f; i += (size_t)gridDim.x * 256u) atomicAdd(&size[label[faces[3 * i]]], 1u);
}
__global__ void __launch_bounds__(256) k_parts_stats(unsigned n_v, const unsigned* __restrict__ label, const unsigned* __restrict__ size, unsigned* __restrict__ vfaces,
                                                     unsigned* __restrict__ part_flag, unsigned* __restrict__ orphan_flag, unsigned long long* best) {
  unsigned long long key = 0ull;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_v; i += (size_t)gridDim.x * 256u) {
    const unsigned l = label[i], s = size[l];
    const bool part = l == (unsigned)i && s > 0u;
    vfaces[i] = s; part_flag[i] = part ? 1u : 0u; orphan_flag[i] = s == 0u ? 1u : 0u;
    if (part) { const unsigned long long k = ((unsigned long long)s << 32) | (unsigned long long)(~l); key = k > key ? k : key; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(key, off, 64); key = o > key ? o : key; }
  if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best, key);
}

// ---- drop ------------------------------------------------------------------------------------------------------------------------------
// a part stays iff it has thr faces or more and, with use_only, is the part `only`
__global__ void __launch_bounds__(256) k_drop_flags(unsigned n_v, unsigned n_f, const unsigned* __restrict__ faces, const unsigned* __restrict__ label,
                                                    const unsigned* __restrict__ size, unsigned thr, int use_only, unsigned only,
                                                    unsigned* __restrict__ vrank, unsigned* __restrict__ frank, unsigned* words) {
  unsigned kept = 0;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_v; i += (size_t)gridDim.x * 256u) {
    const unsigned l = label[i];
    const bool keep = size[l] >= thr && (!use_only || l == only);
    vrank[i] = keep ? 1u : 0u;
    if (keep && l == (unsigned)i) ++kept;
  }
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_f; i += (size_t)gridDim.x * 256u) {
    const unsigned l = label[faces[3 * i]];
    frank[i] = (size[l] >= thr && (!use_only || l == only)) ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kept += __shfl_down(kept, off, 64);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&words[PW_KEPT], kept);
}
// kept vertices in ascending old index, attributes copied verbatim
__global__ void __launch_bounds__(256) k_drop_vertices(unsigned n_v, const unsigned* __restrict__ vrank, const float* __restrict__ v, const float* __restrict__ n,
                                                       const float* __restrict__ c, float* __restrict__ out_v, float* __restrict__ out_n, float* __restrict__ out_c) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_v; i += (size_t)gridDim.x * 256u) {
    const size_t j = vrank[i];
    if (vrank[i + 1] == j) continue;
    out_v[3 * j] = v[3 * i]; out_v[3 * j + 1] = v[3 * i + 1]; out_v[3 * j + 2] = v[3 * i + 2];
    out_n[3 * j] = n[3 * i]; out_n[3 * j + 1] = n[3 * i + 1]; out_n[3 * j + 2] = n[3 * i + 2];
    if (c) { out_c[4 * j] = c[4 * i]; out_c[4 * j + 1] = c[4 * i + 1]; out_c[4 * j + 2] = c[4 * i + 2]; out_c[4 * j + 3] = c[4 * i + 3]; }
  }
}
// kept faces in face order, named by the new vertex ids
__global__ void __launch_bounds__(256) k_drop_faces(unsigned n_f, const unsigned* __restrict__ frank, const unsigned* __restrict__ vrank, const unsigned* __restrict__ faces,
                                                    unsigned* __restrict__ out_f) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_f; i += (size_t)gridDim.x * 256u) {
    const size_t j = frank[i];
    if (frank[i + 1] == j) continue;
    out_f[3 * j] = vrank[faces[3 * i]]; out_f[3 * j + 1] = vrank[faces[3 * i + 1]]; out_f[3 * j + 2] = vrank[faces[3 * i + 2]];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
#define PARTS_PTRS(w) {(void**)&(w)->p_label, (void**)&(w)->p_parent, (void**)&(w)->p_size, (void**)&(w)->p_vfaces, (void**)&(w)->p_vrank[0], (void**)&(w)->p_vrank[1], \
                       (void**)&(w)->p_frank, (void**)&(w)->p_partials, (void**)&(w)->p_words, (void**)&(w)->alt_v, (void**)&(w)->alt_n, (void**)&(w)->alt_c, (void**)&(w)->alt_f}
void kf_mesh_parts_free(KfWeld* w) {
  void** p[] = PARTS_PTRS(w);
  weld_free_list(p, 13);
  w->pcap_v = w->pcap_f = 0; w->pcap_color = 0; w->parts_valid = 0;
}
// the parts' buffers follow the mesh's capacities exactly: after a swap the weld finds buffers of the size it allocated
static int parts_reserve(KfWeld* w) {
  if (w->pcap_v == w->cap_v && w->pcap_f == w->cap_f && w->pcap_color == w->cap_color && w->p_words) return 0;
  const size_t cv = w->cap_v, cf = w->cap_f, big = cv > cf ? cv : cf;
  void** p[] = PARTS_PTRS(w);
  const size_t sizes[] = {cv * 4, cv * 4, cv * 4, cv * 4, (cv + 1) * 4, (cv + 1) * 4, (cf + 1) * 4, (big / KF_SCAN_CHUNK + 2) * 4, PW_WORDS * 4,
                          cv * 12, cv * 12, w->cap_color ? cv * 16 : 0, cf * 12};
  w->pcap_v = w->pcap_f = 0; w->pcap_color = 0;
  if (weld_alloc_list(p, sizes, 13)) return KF_ERR_ALLOC;
  w->pcap_v = cv; w->pcap_f = cf; w->pcap_color = w->cap_color;
  return 0;
}

static int parts_label(kf_ctx* c) {
  KfWeld* w = c->weld;
  if (w->parts_valid) return 0;
  w->n_parts = w->largest_faces = w->n_orphans = w->parts_rounds = 0; w->largest_label = PARTS_NONE;
  if (w->n_v == 0) { w->parts_valid = 1; return 0; }
  { const int e = parts_reserve(w); if (e) return e; }
  hipStream_t st = c->stream;
  const unsigned n_v = w->n_v, n_f = w->n_f;
  KF_CHECK(hipMemsetAsync(w->p_words, 0, PW_WORDS * 4, st));
  hipLaunchKernelGGL(k_parts_init, dim3(weld_grid(c, n_v)), dim3(256), 0, st, n_v, w->p_label, w->p_parent, w->p_size);
  unsigned rounds = 0;
  while (n_f) {
    if (rounds) KF_CHECK(hipMemsetAsync(&w->p_words[PW_CHANGED], 0, 4, st));
    hipLaunchKernelGGL(k_parts_hook, dim3(weld_grid(c, n_f)), dim3(256), 0, st, n_f, w->out_f, w->p_label, w->p_parent, w->p_words);
    for (int k = 0; k < PARTS_DOUBLINGS; ++k) hipLaunchKernelGGL(k_parts_jump, dim3(weld_grid(c, n_v)), dim3(256), 0, st, n_v, w->p_parent);
    hipLaunchKernelGGL(k_parts_root, dim3(weld_grid(c, n_v)), dim3(256), 0, st, n_v, w->p_parent, w->p_label);
    KF_CHECK(hipGetLastError());
    unsigned changed = 0;
    { const int e = weld_read_words(c, &w->p_words[PW_CHANGED], &changed, 1); if (e) return e; }
    ++rounds;
    if (changed == 0) break;
    if (rounds >= n_v) return KF_ERR_STATE;                            // every round but the last joins two roots: more rounds than vertices cannot be
  }
  if (n_f) hipLaunchKernelGGL(k_parts_sizes, dim3(weld_grid(c, n_f)), dim3(256), 0, st, n_f, w->out_f, w->p_label, w->p_size);
  hipLaunchKernelGGL(k_parts_stats, dim3(weld_grid(c, n_v)), dim3(256), 0, st, n_v, w->p_label, w->p_size, w->p_vfaces, w->p_vrank[0], w->p_vrank[1],
                     reinterpret_cast<unsigned long long*>(&w->p_words[PW_BEST]));
  kf_scan_in_place(w->p_vrank[0], n_v, w->p_partials, &w->p_words[PW_PARTS], st);
  kf_scan_in_place(w->p_vrank[1], n_v, w->p_partials, &w->p_words[PW_ORPHANS], st);
  KF_CHECK(hipGetLastError());
  unsigned got[PW_WORDS];
  { const int e = weld_read_words(c, w->p_words, got, PW_WORDS); if (e) return e; }
  w->n_parts = got[PW_PARTS]; w->n_orphans = got[PW_ORPHANS]; w->parts_rounds = rounds;
  if (w->n_parts) { w->largest_faces = got[PW_BEST + 1]; w->largest_label = ~got[PW_BEST]; }
  w->parts_valid = 1;
  return 0;
}

static int parts_enter(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!c->weld || !c->weld->valid) return KF_ERR_STATE;
  KF_CHECK(hipSetDevice(c->cfg.device));
  return parts_label(c);
}

extern "C" int kf_mesh_parts(kf_ctx* c, uint32_t* n_parts, uint32_t* largest_faces, uint32_t* n_orphans, uint32_t* n_rounds) {
  { const int e = parts_enter(c); if (e) return e; }
  const KfWeld* w = c->weld;
  if (n_parts) *n_parts = w->n_parts;
  if (largest_faces) *largest_faces = w->largest_faces;
  if (n_orphans) *n_orphans = w->n_orphans;
  if (n_rounds) *n_rounds = w->parts_rounds;
  return 0;
}

extern "C" int kf_read_mesh_parts(kf_ctx* c, uint32_t* vertex_label, uint32_t* vertex_part_faces) {
  { const int e = parts_enter(c); if (e) return e; }
  const KfWeld* w = c->weld;
  if (w->n_v) {
    if (vertex_label) KF_CHECK(hipMemcpyAsync(vertex_label, w->p_label, (size_t)w->n_v * 4, hipMemcpyDeviceToHost, c->stream));
    if (vertex_part_faces) KF_CHECK(hipMemcpyAsync(vertex_part_faces, w->p_vfaces, (size_t)w->n_v * 4, hipMemcpyDeviceToHost, c->stream));
  }
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int kf_mesh_drop_parts(kf_ctx* c, uint32_t min_faces, int largest_only, uint32_t* parts_dropped, uint32_t* orphans_dropped) {
  { const int e = parts_enter(c); if (e) return e; }
  KfWeld* w = c->weld;
  if (parts_dropped) *parts_dropped = 0;
  if (orphans_dropped) *orphans_dropped = 0;
  if (w->n_v == 0) return 0;
  unsigned thr = min_faces > 1u ? min_faces : 1u;
  if (largest_only && w->largest_faces < thr) thr = PARTS_NONE;       // no part reaches min_faces: nothing stays (no part has 2^32 - 1 faces)
  hipStream_t st = c->stream;
  const unsigned n_v = w->n_v, n_f = w->n_f;
  KF_CHECK(hipMemsetAsync(&w->p_words[PW_KEPT], 0, 4, st));
  KF_CHECK(hipMemsetAsync(&w->p_words[PW_NV], 0, 8, st));
  hipLaunchKernelGGL(k_drop_flags, dim3(weld_grid(c, n_v > n_f ? n_v : n_f)), dim3(256), 0, st, n_v, n_f, w->out_f, w->p_label, w->p_size, thr, largest_only != 0,
                     w->largest_label, w->p_vrank[0], w->p_frank, w->p_words);
  kf_scan_in_place(w->p_vrank[0], n_v, w->p_partials, &w->p_words[PW_NV], st);
  if (n_f) kf_scan_in_place(w->p_frank, n_f, w->p_partials, &w->p_words[PW_NF], st);
  hipLaunchKernelGGL(k_drop_vertices, dim3(weld_grid(c, n_v)), dim3(256), 0, st, n_v, w->p_vrank[0], w->out_v, w->out_n, w->has_color ? w->out_c : (float*)nullptr,
                     w->alt_v, w->alt_n, w->alt_c);
  if (n_f) hipLaunchKernelGGL(k_drop_faces, dim3(weld_grid(c, n_f)), dim3(256), 0, st, n_f, w->p_frank, w->p_vrank[0], w->out_f, w->alt_f);
  KF_CHECK(hipGetLastError());
  unsigned got[PW_WORDS];
  { const int e = weld_read_words(c, w->p_words, got, PW_WORDS); if (e) return e; }
  if (got[PW_NV] > n_v || got[PW_NF] > n_f || got[PW_KEPT] > w->n_parts) return KF_ERR_STATE;
  if (parts_dropped) *parts_dropped = w->n_parts - got[PW_KEPT];
  if (orphans_dropped) *orphans_dropped = w->n_orphans;
  { float* t = w->out_v; w->out_v = w->alt_v; w->alt_v = t; }
  { float* t = w->out_n; w->out_n = w->alt_n; w->alt_n = t; }
  { float* t = w->out_c; w->out_c = w->alt_c; w->alt_c = t; }
  { unsigned* t = w->out_f; w->out_f = w->alt_f; w->alt_f = t; }
  w->n_v = got[PW_NV]; w->n_f = got[PW_NF];
  w->parts_valid = 0;                                                 // the labels named the old vertex indices
  return 0;
}
