// weld.hip -- the triangle soup of the extraction welded into an indexed mesh on the device (reference: what
// MeshGeneratorMarchingcube::saveMesh runs on one host thread, src/MeshGeneratorMarchingcube.cpp:69-86:
// MeshData::mergeCloseVertices (approx), removeDegeneratedFaces, removeDuplicateFaces, computeVertexNormals --
// src/utils/mesh/meshData.cpp:42-82,179-310, src/utils/mesh/meshData.h:713-753).  Same vertices, indices and normals, bit for bit.
//
// The reference's weld is a sequential greedy over the soup vertices: vertex v lies in cell c(v) (meshData.h:750-753, edge = thresh),
// takes the id of the first occupied cell among the 27 around c(v) in (i, j, k) order, and otherwise becomes a new vertex and
// occupies c(v).  Occupancy only grows, so a cell is ever occupied iff its FIRST vertex (its priority p(c): the smallest soup
// index in it) finds no occupied neighbour: the occupied cells are the greedy maximal independent set of the distinct cells under
// 26-adjacency in priority order.  That set has a deterministic parallel form, and everything after it is scans and gathers:
//   insert  : one lane per soup vertex; an open-addressing table whose slot holds a SOUP-VERTEX INDEX: an empty slot is claimed by
//             compare-and-swap, a slot whose holder lies in the same cell takes atomicMin(index), any other sends the probe on.  The
//             key is recomputed from the holder's position, so when the inserts are done every used slot holds exactly p(c).
//   rounds  : a state byte per slot.  Per round (one launch, previous states read, next states written): an undecided cell is OUT if
//             a neighbour with a smaller p is IN, IN if every neighbour with a smaller p is OUT, and otherwise waits.  The undecided
//             cell of smallest p always decides.  The host reads the number still undecided after each round.
//   ids     : flag "first vertex of an IN cell" per soup vertex -> exclusive scan = output vertex id; vertices (colours) copied.
//   lookup  : per soup vertex the first cell in (i, j, k) order among the 27 that is IN and has p <= v (occupied when v was visited).
//   faces   : remapped through lookup; a face that names a vertex twice goes; a second table of the same kind, holding FACE indices
//             under the sorted index triple, keeps the first of every set of duplicates; flag -> scan -> compaction in face order.
//   normals : no float atomics (their sums would depend on arrival order): faces counted per vertex -> scan -> filled -> every
//             vertex's list ordered by face index -> one lane per vertex adds its faces' unit normals in that order.
// Every output is a function of the soup's order alone, never of slot positions, arrival order or scheduling.
#include "kf_internal.h"
#include "weld_mesh.h"
#include "scan.h"
#include <limits.h>
#include <string.h>
#include <new>

#define WELD_EMPTY 0xFFFFFFFFu
enum { WELD_UNDECIDED = 0, WELD_IN = 1, WELD_OUT = 2 };
// device words: [0] cells still undecided after the round, [1] distinct cells, [2] output vertices, [3] output faces, [4] a lookup found no cell (never)
enum { WW_UNDECIDED = 0, WW_CELLS = 1, WW_NV = 2, WW_NF = 3, WW_ERR = 4, WW_WORDS = 8 };

// ---- device arithmetic -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ const float* weld_pos(const kf_triangle* tris, unsigned v) {
  return reinterpret_cast<const float*>(tris) + (size_t)(v / 3u) * 18u + (size_t)(v % 3u) * 6u;
}
// meshData.h:750-753 toVirtualVoxelPos, one axis: (int)(v * r + (float)(sgn(v) * 0.5)); what no int holds converts as the host's cvttss2si does
__device__ __forceinline__ int weld_axis(float v, float r) {
  const float x = v * r + (float)(((0.f < v) - (v < 0.f)) * 0.5);
  if (!(x > -2147483648.f && x < 2147483648.f)) return INT_MIN;
  return (int)x;
}
__device__ __forceinline__ int3 weld_cell(const kf_triangle* tris, unsigned v, float r) {
  const float* p = weld_pos(tris, v);
  return make_int3(weld_axis(p[0], r), weld_axis(p[1], r), weld_axis(p[2], r));
}
__device__ __forceinline__ unsigned weld_mix(unsigned h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ unsigned weld_hash(int3 c) { return weld_mix(((unsigned)c.x * 73856093u) ^ ((unsigned)c.y * 19349669u) ^ ((unsigned)c.z * 83492791u)); }
__device__ __forceinline__ bool weld_same(int3 a, int3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// slot of cell c once the inserts are done (at most half the slots are used: the probe ends), WELD_EMPTY if no vertex lies in it
__device__ __forceinline__ unsigned weld_find(const unsigned* __restrict__ table, unsigned mask, const kf_triangle* tris, float r, int3 c) {
  unsigned s = weld_hash(c) & mask;
  for (;;) {
    const unsigned h = table[s];
    if (h == WELD_EMPTY) return WELD_EMPTY;
    if (weld_same(weld_cell(tris, h, r), c)) return s;
    s = (s + 1u) & mask;
  }
}

// ---- cells ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_weld_insert(const kf_triangle* __restrict__ tris, unsigned nv, float r, unsigned* table, unsigned mask, unsigned* __restrict__ vslot) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256u) {
    const unsigned v = (unsigned)i;
    const int3 c = weld_cell(tris, v, r);
    unsigned s = weld_hash(c) & mask;
    for (;;) {
      unsigned h = table[s];
      if (h == WELD_EMPTY) {
        h = atomicCAS(&table[s], WELD_EMPTY, v);
        if (h == WELD_EMPTY) break;                                   // claimed
      }
      if (weld_same(weld_cell(tris, h, r), c)) { atomicMin(&table[s], v); break; }
      s = (s + 1u) & mask;
    }
    vslot[v] = s;
  }
}

// one round of the independent set; lonely != null in round 0, where every used slot is visited: the cells are counted there
__global__ void __launch_bounds__(256) k_weld_round(const kf_triangle* __restrict__ tris, float r, const unsigned* __restrict__ table, unsigned cap,
                                                    const unsigned char* __restrict__ prev, unsigned char* __restrict__ next, unsigned char* __restrict__ lonely,
                                                    unsigned* words) {
  __shared__ unsigned s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned mask = cap - 1u;
  unsigned n_und = 0, n_cells = 0;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < cap; i += (size_t)gridDim.x * 256u) {
    const unsigned s = (unsigned)i;
    const unsigned p = table[s];
    if (p == WELD_EMPTY) continue;
    ++n_cells;
    unsigned char st = prev[s];
    if (st == WELD_UNDECIDED) {
      const int3 c = weld_cell(tris, p, r);
      bool any_in = false, wait = false, nbr = false;
      for (int n = 0; n < 27; ++n) {
        if (n == 13) continue;
        const int3 q = make_int3(c.x + n / 9 - 1, c.y + (n / 3) % 3 - 1, c.z + n % 3 - 1);
        const unsigned s2 = weld_find(table, mask, tris, r, q);
        if (s2 == WELD_EMPTY) continue;
        nbr = true;
        if (table[s2] < p) {
          const unsigned char t = prev[s2];
          any_in |= t == WELD_IN;
          wait |= t == WELD_UNDECIDED;
        }
      }
      st = any_in ? WELD_OUT : (wait ? WELD_UNDECIDED : WELD_IN);
      if (lonely) lonely[s] = nbr ? 0 : 1;
      if (st == WELD_UNDECIDED) ++n_und;
    }
    next[s] = st;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { n_und += __shfl_down(n_und, off, 64); n_cells += __shfl_down(n_cells, off, 64); }
  if ((threadIdx.x & 63) == 0) { if (n_und) atomicAdd(&s_cnt[0], n_und); if (n_cells) atomicAdd(&s_cnt[1], n_cells); }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(&words[WW_UNDECIDED], s_cnt[0]);
    if (lonely && s_cnt[1]) atomicAdd(&words[WW_CELLS], s_cnt[1]);
  }
}

// ---- vertices ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_weld_vertex_flags(unsigned nv, const unsigned* __restrict__ table, const unsigned* __restrict__ vslot,
                                                           const unsigned char* __restrict__ state, unsigned* __restrict__ vrank) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256u) {
    const unsigned s = vslot[i];
    vrank[i] = (table[s] == (unsigned)i && state[s] == WELD_IN) ? 1u : 0u;
  }
}
// output vertices (meshData.cpp:256-262: the cell's first vertex, copied) and the lookup (:233-252) of every soup vertex
__global__ void __launch_bounds__(256) k_weld_lookup(const kf_triangle* __restrict__ tris, unsigned nv, float r, const unsigned* __restrict__ table, unsigned mask,
                                                     const unsigned* __restrict__ vslot, const unsigned char* __restrict__ state, const unsigned char* __restrict__ lonely,
                                                     const unsigned* __restrict__ vrank, unsigned n_out, unsigned* __restrict__ lookup,
                                                     float* __restrict__ out_v, float* __restrict__ out_c, unsigned* words) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256u) {
    const unsigned v = (unsigned)i;
    const unsigned s = vslot[v];
    unsigned id = WELD_EMPTY;
    if (table[s] == v && state[s] == WELD_IN) {
      id = vrank[v];
      if (id < n_out) {
        const float* p = weld_pos(tris, v);
        out_v[3 * (size_t)id] = p[0]; out_v[3 * (size_t)id + 1] = p[1]; out_v[3 * (size_t)id + 2] = p[2];
        if (out_c) { float* c = out_c + 4 * (size_t)id; c[0] = p[5]; c[1] = p[4]; c[2] = p[3]; c[3] = 1.0f; }   // MeshGeneratorMarchingcube.cpp:53: x <-> z
      }
    } else if (lonely[s]) {
      id = vrank[table[s]];                                          // no other cell near: the cell is IN and its first vertex came before v
    } else {
      const int3 c = weld_cell(tris, v, r);
      for (int n = 0; n < 27; ++n) {                                  // (i, j, k) order, k fastest
        const unsigned s2 = n == 13 ? s : weld_find(table, mask, tris, r, make_int3(c.x + n / 9 - 1, c.y + (n / 3) % 3 - 1, c.z + n % 3 - 1));
        if (s2 == WELD_EMPTY || state[s2] != WELD_IN) continue;
        const unsigned p = table[s2];
        if (p <= v) { id = vrank[p]; break; }                         // occupied when v was visited
      }
    }
    if (id >= n_out) { words[WW_ERR] = 1u; id = 0; }                  // cannot happen (an OUT cell has an earlier IN neighbour); keeps every later index in range
    lookup[v] = id;
  }
}

// ---- faces ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint3 weld_sorted(uint3 f) {
  if (f.x > f.y) { const unsigned t = f.x; f.x = f.y; f.y = t; }
  if (f.y > f.z) { const unsigned t = f.y; f.y = f.z; f.z = t; }
  if (f.x > f.y) { const unsigned t = f.x; f.x = f.y; f.y = t; }
  return f;
}
__device__ __forceinline__ uint3 weld_face(const unsigned* __restrict__ lookup, unsigned f) {
  return make_uint3(lookup[3 * (size_t)f], lookup[3 * (size_t)f + 1], lookup[3 * (size_t)f + 2]);
}
// meshData.cpp:289-310 and :42-82: the faces that name three different vertices go into a table keyed by their sorted triple
__global__ void __launch_bounds__(256) k_weld_face_insert(const unsigned* __restrict__ lookup, unsigned nf, unsigned* ftable, unsigned mask, unsigned* __restrict__ fslot) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nf; i += (size_t)gridDim.x * 256u) {
    const unsigned f = (unsigned)i;
    const uint3 raw = weld_face(lookup, f);
    if (raw.x == raw.y || raw.x == raw.z || raw.y == raw.z) { fslot[f] = WELD_EMPTY; continue; }
    const uint3 key = weld_sorted(raw);
    unsigned s = weld_mix((key.x * 73856093u) ^ (key.y * 19349669u) ^ (key.z * 83492791u)) & mask;
    for (;;) {
      unsigned h = ftable[s];
      if (h == WELD_EMPTY) {
        h = atomicCAS(&ftable[s], WELD_EMPTY, f);
        if (h == WELD_EMPTY) break;
      }
      const uint3 hk = weld_sorted(weld_face(lookup, h));
      if (hk.x == key.x && hk.y == key.y && hk.z == key.z) { atomicMin(&ftable[s], f); break; }
      s = (s + 1u) & mask;
    }
    fslot[f] = s;
  }
}
__global__ void __launch_bounds__(256) k_weld_face_flags(unsigned nf, const unsigned* __restrict__ ftable, const unsigned* __restrict__ fslot, unsigned* __restrict__ frank) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nf; i += (size_t)gridDim.x * 256u) {
    const unsigned s = fslot[i];
    frank[i] = (s != WELD_EMPTY && ftable[s] == (unsigned)i) ? 1u : 0u;
  }
}
// surviving faces in face order; their unit normals (meshData.h:717-724); faces counted per vertex
__global__ void __launch_bounds__(256) k_weld_face_emit(unsigned nf, const unsigned* __restrict__ lookup, const unsigned* __restrict__ frank, unsigned n_out,
                                                        const float* __restrict__ out_v, unsigned* __restrict__ out_f, float* __restrict__ fnorm, unsigned* vcount) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nf; i += (size_t)gridDim.x * 256u) {
    const unsigned j = frank[i];
    if (frank[i + 1] == j || j >= n_out) continue;
    const uint3 f = weld_face(lookup, (unsigned)i);
    out_f[3 * (size_t)j] = f.x; out_f[3 * (size_t)j + 1] = f.y; out_f[3 * (size_t)j + 2] = f.z;
    const float* a = out_v + 3 * (size_t)f.x; const float* b = out_v + 3 * (size_t)f.y; const float* c = out_v + 3 * (size_t)f.z;
    const float3 pa = kf3(a[0], a[1], a[2]);
    const float3 n = kf_normalize(kf_cross(kf_sub(kf3(b[0], b[1], b[2]), pa), kf_sub(kf3(c[0], c[1], c[2]), pa)));
    fnorm[3 * (size_t)j] = n.x; fnorm[3 * (size_t)j + 1] = n.y; fnorm[3 * (size_t)j + 2] = n.z;
    atomicAdd(&vcount[f.x], 1u); atomicAdd(&vcount[f.y], 1u); atomicAdd(&vcount[f.z], 1u);
  }
}

// ---- normals -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_weld_fill(unsigned n_faces, const unsigned* __restrict__ out_f, const unsigned* __restrict__ vstart, unsigned* cursor,
                                                   unsigned* __restrict__ flist) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < (size_t)n_faces * 3u; i += (size_t)gridDim.x * 256u) {
    const unsigned u = out_f[i];
    flist[vstart[u] + atomicAdd(&cursor[u], 1u)] = (unsigned)(i / 3u);
  }
}
// meshData.h:725-735: the faces' unit normals added per vertex in ascending face order (the filled lists arrive in any order: sorted here,
// whatever their length), then normalised; a vertex that no face names keeps zeros
__global__ void __launch_bounds__(256) k_weld_normals(unsigned n_vertices, const unsigned* __restrict__ vstart, unsigned* __restrict__ flist,
                                                      const float* __restrict__ fnorm, float* __restrict__ out_n) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_vertices; i += (size_t)gridDim.x * 256u) {
    const unsigned b = vstart[i], e = vstart[i + 1];
    for (unsigned k = b + 1; k < e; ++k) {
      const unsigned x = flist[k];
      unsigned m = k;
      while (m > b && flist[m - 1] > x) { flist[m] = flist[m - 1]; --m; }
      flist[m] = x;
    }
    float3 d = kf3(0.f, 0.f, 0.f);
    for (unsigned k = b; k < e; ++k) { const float* n = fnorm + 3 * (size_t)flist[k]; d.x += n[0]; d.y += n[1]; d.z += n[2]; }
    d = kf_normalize(d);
    out_n[3 * i] = d.x; out_n[3 * i + 1] = d.y; out_n[3 * i + 2] = d.z;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static void weld_free_scratch(KfWeld* w) {
  void** p[] = {(void**)&w->table, (void**)&w->vslot, (void**)&w->state[0], (void**)&w->state[1], (void**)&w->lonely, (void**)&w->vrank, (void**)&w->lookup,
                (void**)&w->frank, (void**)&w->partials, (void**)&w->words};
  weld_free_list(p, 10);
  w->cap_tris = 0; w->table_cap = 0;
}
static void weld_free_mesh(KfWeld* w) {
  void** p[] = {(void**)&w->out_v, (void**)&w->out_n, (void**)&w->out_c, (void**)&w->vstart, (void**)&w->cursor, (void**)&w->out_f, (void**)&w->flist, (void**)&w->fnorm};
  weld_free_list(p, 8);
  w->cap_v = w->cap_f = 0; w->cap_color = 0;
}
void kf_weld_free(kf_ctx* c) {
  if (!c->weld) return;
  weld_free_scratch(c->weld); weld_free_mesh(c->weld); kf_mesh_parts_free(c->weld);
  delete c->weld; c->weld = nullptr;
}

extern "C" int kf_write_triangles(kf_ctx* c, const kf_triangle* src, uint32_t first, uint32_t count) {
  if (!c || (!src && count)) return KF_ERR_ARG;
  if ((uint64_t)first + count > c->max_triangles) return KF_ERR_ARG;
  if (!c->triangles) return KF_ERR_STATE;
  if (count) KF_CHECK(hipMemcpyAsync(c->triangles + first, src, (size_t)count * sizeof(kf_triangle), hipMemcpyHostToDevice, c->stream));
  *(unsigned*)c->host_pinned = first + count;
  KF_CHECK(hipMemcpyAsync(&c->counters->n_triangles, c->host_pinned, sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int kf_weld_mesh(kf_ctx* c, int has_color, float thresh) {
  if (!c || !(thresh > 0.f)) return KF_ERR_ARG;
  if (!c->triangles) return KF_ERR_STATE;
  KF_CHECK(hipSetDevice(c->cfg.device));
  unsigned n_tris = 0;
  { const int st = weld_read_words(c, &c->counters->n_triangles, &n_tris, 1); if (st) return st; }
  if (n_tris > 0xFFFFFFFFu / 3u) return KF_ERR_ARG;
  if (!c->weld) { c->weld = new (std::nothrow) KfWeld(); if (!c->weld) return KF_ERR_ALLOC; memset((void*)c->weld, 0, sizeof(KfWeld)); }
  KfWeld* w = c->weld;
  w->valid = 0; w->parts_valid = 0;
  if (n_tris == 0) { w->n_v = w->n_f = w->n_rounds = 0; w->has_color = has_color != 0; w->valid = 1; return 0; }
  const unsigned nv = 3u * n_tris;
  if (n_tris > w->cap_tris) {                                          // scratch: kept for the next weld, grown when a larger soup comes
    uint64_t cap = 1024;
    while (cap < 2ull * nv) cap <<= 1;                                 // at most half the slots are ever used
    if (cap > (1ull << 31)) return KF_ERR_ALLOC;
    void** p[] = {(void**)&w->table, (void**)&w->vslot, (void**)&w->state[0], (void**)&w->state[1], (void**)&w->lonely, (void**)&w->vrank, (void**)&w->lookup,
                  (void**)&w->frank, (void**)&w->partials, (void**)&w->words};
    const size_t sizes[] = {(size_t)cap * 4, (size_t)nv * 4, (size_t)cap, (size_t)cap, (size_t)cap, ((size_t)nv + 1) * 4, (size_t)nv * 4,
                            ((size_t)n_tris + 1) * 4, ((size_t)nv / KF_SCAN_CHUNK + 2) * 4, WW_WORDS * 4};
    w->cap_tris = 0; w->table_cap = 0;
    if (weld_alloc_list(p, sizes, 10)) return KF_ERR_ALLOC;
    w->cap_tris = n_tris; w->table_cap = (unsigned)cap;
  }
  unsigned cap = 1024;
  while ((uint64_t)cap < 2ull * nv) cap <<= 1;                         // this soup's table: a prefix of the scratch (a small soup after a large one probes a small table)
  unsigned fcap = 1024;
  while ((uint64_t)fcap < 2ull * n_tris) fcap <<= 1;
  const float r = (float)(1.0 / (double)thresh);                       // meshData.h:751
  hipStream_t st = c->stream;
  const kf_triangle* tris = c->triangles;

  KF_CHECK(hipMemsetAsync(w->table, 0xFF, (size_t)cap * 4, st));
  KF_CHECK(hipMemsetAsync(w->state[0], 0, cap, st));
  KF_CHECK(hipMemsetAsync(w->state[1], 0, cap, st));
  KF_CHECK(hipMemsetAsync(w->words, 0, WW_WORDS * 4, st));
  hipLaunchKernelGGL(k_weld_insert, dim3(weld_grid(c, nv)), dim3(256), 0, st, tris, nv, r, w->table, cap - 1u, w->vslot);
  unsigned rounds = 0, n_cells = 0;
  for (;;) {
    unsigned char* prev = w->state[rounds & 1u]; unsigned char* next = w->state[(rounds + 1u) & 1u];
    if (rounds) KF_CHECK(hipMemsetAsync(&w->words[WW_UNDECIDED], 0, 4, st));
    hipLaunchKernelGGL(k_weld_round, dim3(weld_grid(c, cap)), dim3(256), 0, st, tris, r, w->table, cap, prev, next, rounds == 0 ? w->lonely : (unsigned char*)nullptr, w->words);
    KF_CHECK(hipGetLastError());
    unsigned got[2];
    { const int e = weld_read_words(c, w->words, got, 2); if (e) return e; }
    if (rounds == 0) n_cells = got[WW_CELLS];
    ++rounds;
    if (got[WW_UNDECIDED] == 0) break;
    if (rounds >= n_cells) return KF_ERR_STATE;                        // every round decides a cell: more rounds than cells cannot be
  }
  const unsigned char* state = w->state[rounds & 1u];
  hipLaunchKernelGGL(k_weld_vertex_flags, dim3(weld_grid(c, nv)), dim3(256), 0, st, nv, w->table, w->vslot, state, w->vrank);
  kf_scan_in_place(w->vrank, nv, w->partials, &w->words[WW_NV], st);
  unsigned n_out = 0;
  { const int e = weld_read_words(c, &w->words[WW_NV], &n_out, 1); if (e) return e; }
  if (n_out == 0 || n_out > n_cells) return KF_ERR_STATE;
  if (n_out > w->cap_v || (has_color && !w->cap_color)) {
    void** p[] = {(void**)&w->out_v, (void**)&w->out_n, (void**)&w->out_c, (void**)&w->vstart, (void**)&w->cursor};
    const size_t sizes[] = {(size_t)n_out * 12, (size_t)n_out * 12, has_color ? (size_t)n_out * 16 : 0, ((size_t)n_out + 1) * 4, (size_t)n_out * 4};
    w->cap_v = 0; w->cap_color = 0;
    if (weld_alloc_list(p, sizes, 5)) return KF_ERR_ALLOC;
    w->cap_v = n_out; w->cap_color = has_color != 0;
  }
  hipLaunchKernelGGL(k_weld_lookup, dim3(weld_grid(c, nv)), dim3(256), 0, st, tris, nv, r, w->table, cap - 1u, w->vslot, state, w->lonely, w->vrank, n_out, w->lookup,
                     w->out_v, has_color ? w->out_c : (float*)nullptr, w->words);
  // faces: the table and the slot array start their second life
  KF_CHECK(hipMemsetAsync(w->table, 0xFF, (size_t)fcap * 4, st));
  hipLaunchKernelGGL(k_weld_face_insert, dim3(weld_grid(c, n_tris)), dim3(256), 0, st, w->lookup, n_tris, w->table, fcap - 1u, w->vslot);
  hipLaunchKernelGGL(k_weld_face_flags, dim3(weld_grid(c, n_tris)), dim3(256), 0, st, n_tris, w->table, w->vslot, w->frank);
  kf_scan_in_place(w->frank, n_tris, w->partials, &w->words[WW_NF], st);
  unsigned got[3];
  { const int e = weld_read_words(c, &w->words[WW_NV], got, 3); if (e) return e; }
  if (got[WW_ERR - WW_NV]) return KF_ERR_STATE;
  const unsigned n_faces = got[WW_NF - WW_NV];
  if (n_faces > w->cap_f) {
    void** p[] = {(void**)&w->out_f, (void**)&w->flist, (void**)&w->fnorm};
    const size_t sizes[] = {(size_t)n_faces * 12, (size_t)n_faces * 12, (size_t)n_faces * 12};
    w->cap_f = 0;
    if (weld_alloc_list(p, sizes, 3)) return KF_ERR_ALLOC;
    w->cap_f = n_faces;
  }
  KF_CHECK(hipMemsetAsync(w->vstart, 0, ((size_t)n_out + 1) * 4, st));
  KF_CHECK(hipMemsetAsync(w->cursor, 0, (size_t)n_out * 4, st));
  if (n_faces) {
    hipLaunchKernelGGL(k_weld_face_emit, dim3(weld_grid(c, n_tris)), dim3(256), 0, st, n_tris, w->lookup, w->frank, n_faces, w->out_v, w->out_f, w->fnorm, w->vstart);
    kf_scan_in_place(w->vstart, n_out, w->partials, (unsigned*)nullptr, st);
    hipLaunchKernelGGL(k_weld_fill, dim3(weld_grid(c, (size_t)n_faces * 3)), dim3(256), 0, st, n_faces, w->out_f, w->vstart, w->cursor, w->flist);
  }
  hipLaunchKernelGGL(k_weld_normals, dim3(weld_grid(c, n_out)), dim3(256), 0, st, n_out, w->vstart, w->flist, w->fnorm, w->out_n);
  KF_CHECK(hipGetLastError());
  w->n_v = n_out; w->n_f = n_faces; w->n_rounds = rounds; w->has_color = has_color != 0; w->valid = 1;
  return 0;
}

extern "C" int kf_mesh_counts(kf_ctx* c, uint32_t* n_vertices, uint32_t* n_faces, uint32_t* n_rounds) {
  if (!c) return KF_ERR_ARG;
  if (!c->weld || !c->weld->valid) return KF_ERR_STATE;
  KF_CHECK(hipStreamSynchronize(c->stream));
  if (n_vertices) *n_vertices = c->weld->n_v;
  if (n_faces) *n_faces = c->weld->n_f;
  if (n_rounds) *n_rounds = c->weld->n_rounds;
  return 0;
}

extern "C" int kf_read_mesh(kf_ctx* c, float* vertices, float* normals, float* colors, uint32_t* faces) {
  if (!c) return KF_ERR_ARG;
  if (!c->weld || !c->weld->valid) return KF_ERR_STATE;
  const KfWeld* w = c->weld;
  if (w->n_v) {
    if (vertices) KF_CHECK(hipMemcpyAsync(vertices, w->out_v, (size_t)w->n_v * 12, hipMemcpyDeviceToHost, c->stream));
    if (normals) KF_CHECK(hipMemcpyAsync(normals, w->out_n, (size_t)w->n_v * 12, hipMemcpyDeviceToHost, c->stream));
    if (colors && w->has_color) KF_CHECK(hipMemcpyAsync(colors, w->out_c, (size_t)w->n_v * 16, hipMemcpyDeviceToHost, c->stream));
  }
  if (faces && w->n_f) KF_CHECK(hipMemcpyAsync(faces, w->out_f, (size_t)w->n_f * 12, hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int kf_weld_release(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!c->weld) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  KF_CHECK(hipStreamSynchronize(c->stream));
  kf_weld_free(c);
  return 0;
}
