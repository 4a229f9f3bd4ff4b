// weld_mesh.h -- the context's indexed mesh: what kf_weld_mesh (weld.hip) makes and kf_mesh_parts / kf_mesh_drop_parts (meshparts.hip)
// label and rewrite.  Host side only: no kernel takes any of this by value.
#pragma once
#include "kf_internal.h"
#include <string.h>

struct KfWeld {
  // scratch, sized by the triangle count
  size_t cap_tris; unsigned table_cap;
  unsigned* table;                 // [table_cap] soup-vertex index per cell; afterwards [face_cap] face index per index triple
  unsigned* vslot;                 // [3 cap_tris] the slot of every soup vertex's cell; afterwards the slot of every face's triple
  unsigned char* state[2];         // [table_cap] WELD_* per slot, double-buffered across rounds
  unsigned char* lonely;           // [table_cap] the cell has no neighbour cell at all (round 0)
  unsigned* vrank;                 // [3 cap_tris + 1] flag, then output vertex id, per soup vertex
  unsigned* lookup;                // [3 cap_tris] output vertex id per soup vertex = the remapped faces
  unsigned* frank;                 // [cap_tris + 1] flag, then output face id, per triangle
  unsigned* partials;              // scan partials
  unsigned* words;                 // [WW_WORDS]
  // the indexed mesh (+ what the normals need), sized by the output counts
  size_t cap_v, cap_f; int cap_color;
  float* out_v; float* out_n; float* out_c; unsigned* vstart; unsigned* cursor;      // [3 cap_v] x 2, [4 cap_v], [cap_v + 1], [cap_v]
  unsigned* out_f; unsigned* flist; float* fnorm;                                   // [3 cap_f] x 3
  unsigned n_v, n_f, n_rounds; int has_color, valid;
  // the mesh's parts (meshparts.hip).  The second mesh buffers have exactly the capacities above: a drop compacts into them and swaps the pointers.
  size_t pcap_v, pcap_f; int pcap_color;
  unsigned* p_label; unsigned* p_parent; unsigned* p_size; unsigned* p_vfaces;      // [pcap_v] label, union-find parent, faces per label, faces of the vertex's part
  unsigned* p_vrank[2];            // [pcap_v + 1] x 2 flag, then scanned, per vertex
  unsigned* p_frank;               // [pcap_f + 1] flag, then output face id, per face
  unsigned* p_partials;            // scan partials of the larger of the two
  unsigned* p_words;               // [PW_WORDS]
  float* alt_v; float* alt_n; float* alt_c; unsigned* alt_f;                          // the second mesh
  unsigned n_parts, largest_faces, largest_label, n_orphans, parts_rounds; int parts_valid;   // of the current mesh, while parts_valid
};

static inline void weld_free_list(void*** ptrs, int n) { for (int i = 0; i < n; ++i) { if (*ptrs[i]) hipFree(*ptrs[i]); *ptrs[i] = nullptr; } }
// all or nothing: what the list held is freed first; on failure every pointer of it is null again
static inline int weld_alloc_list(void*** ptrs, const size_t* sizes, int n) {
  weld_free_list(ptrs, n);
  for (int i = 0; i < n; ++i) {
    if (sizes[i] == 0) continue;
    if (hipMalloc(ptrs[i], sizes[i]) != hipSuccess) { (void)hipGetLastError(); *ptrs[i] = nullptr; weld_free_list(ptrs, n); return KF_ERR_ALLOC; }
  }
  return 0;
}
static inline int weld_read_words(kf_ctx* c, const unsigned* dev, unsigned* out, int n) {
  KF_CHECK(hipMemcpyAsync(c->host_pinned, dev, n * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  memcpy(out, c->host_pinned, n * sizeof(unsigned));
  return 0;
}
static inline unsigned weld_grid(const kf_ctx* c, size_t n) {
  const size_t wgs = (n + 255) / 256, walk = (size_t)(c->num_cus > 0 ? c->num_cus : 256) * 8u;
  return (unsigned)(wgs < 1 ? 1 : (wgs < walk ? wgs : walk));
}
void kf_mesh_parts_free(KfWeld* w);      // (meshparts.hip) the parts' buffers, for kf_weld_free
