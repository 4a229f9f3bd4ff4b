// mesh_parts.hpp -- the connected parts of an indexed mesh and dropping the small ones, on one host thread: the rule of include/hybkf.h
// (kf_mesh_parts / kf_mesh_drop_parts) as a sequential union-find whose root is always the smaller index.  Header-only, plain C++; works on
// any mesh type with MeshData's four vectors (vertices xyz, normals xyz, colors rgba or empty, faces 3 indices).
#pragma once
#include <cstddef>
#include <vector>

namespace mesh_parts_detail {
inline unsigned find_root(std::vector<unsigned>& parent, unsigned x) {
  unsigned r = x;
  while (parent[r] != r) r = parent[r];
  while (parent[x] != r) { const unsigned n = parent[x]; parent[x] = r; x = n; }
  return r;
}
inline void join(std::vector<unsigned>& parent, unsigned a, unsigned b) {
  a = find_root(parent, a); b = find_root(parent, b);
  if (a < b) parent[b] = a; else if (b < a) parent[a] = b;          // the smaller index is the root: a part's label is its smallest vertex
}
}  // namespace mesh_parts_detail

// labels[v]: the smallest vertex index of v's part; part_faces[v]: the faces of v's part (0: an orphan, a vertex that no face names)
template <class Mesh>
inline void meshParts(const Mesh& m, std::vector<unsigned>& labels, std::vector<unsigned>& part_faces) {
  const size_t nv = m.vertices.size() / 3, nf = m.faces.size() / 3;
  std::vector<unsigned> parent(nv);
  for (size_t v = 0; v < nv; ++v) parent[v] = (unsigned)v;
  for (size_t f = 0; f < nf; ++f) {
    mesh_parts_detail::join(parent, m.faces[3 * f], m.faces[3 * f + 1]);
    mesh_parts_detail::join(parent, m.faces[3 * f], m.faces[3 * f + 2]);
  }
  labels.resize(nv);
  for (size_t v = 0; v < nv; ++v) labels[v] = mesh_parts_detail::find_root(parent, (unsigned)v);
  std::vector<unsigned> size(nv, 0u);
  for (size_t f = 0; f < nf; ++f) ++size[labels[m.faces[3 * f]]];
  part_faces.resize(nv);
  for (size_t v = 0; v < nv; ++v) part_faces[v] = size[labels[v]];
}

// Keeps the parts with at least max(min_faces, 1) faces -- with largest_only only the one with the most faces (a tie: the smallest label; none if
// it has fewer than min_faces).  Kept faces keep their order, kept vertices their ascending order and their positions, normals and colours, verbatim.
template <class Mesh>
inline void dropParts(Mesh& m, unsigned min_faces, bool largest_only, unsigned* parts_dropped = nullptr, unsigned* orphans_dropped = nullptr) {
  const size_t nv = m.vertices.size() / 3, nf = m.faces.size() / 3;
  std::vector<unsigned> labels, part_faces;
  meshParts(m, labels, part_faces);
  const unsigned thr = min_faces > 1u ? min_faces : 1u;
  unsigned best_faces = 0, best_label = 0, n_parts = 0, n_orphans = 0, n_kept = 0;
  for (size_t v = 0; v < nv; ++v) {
    if (part_faces[v] == 0) { ++n_orphans; continue; }
    if (labels[v] != v) continue;
    ++n_parts;
    if (part_faces[v] > best_faces) { best_faces = part_faces[v]; best_label = (unsigned)v; }   // ascending v: a tie stays with the smaller label
  }
  std::vector<unsigned> new_id(nv, 0u);
  const bool has_col = m.colors.size() == nv * 4, has_n = m.normals.size() == nv * 3;
  size_t w = 0;
  for (size_t v = 0; v < nv; ++v) {
    const bool keep = part_faces[v] >= thr && (!largest_only || (labels[v] == best_label && best_faces >= thr));
    if (!keep) { new_id[v] = (unsigned)-1; continue; }
    if (labels[v] == v) ++n_kept;
    new_id[v] = (unsigned)w;
    for (int k = 0; k < 3; ++k) m.vertices[3 * w + k] = m.vertices[3 * v + k];
    if (has_n) for (int k = 0; k < 3; ++k) m.normals[3 * w + k] = m.normals[3 * v + k];
    if (has_col) for (int k = 0; k < 4; ++k) m.colors[4 * w + k] = m.colors[4 * v + k];
    ++w;
  }
  m.vertices.resize(3 * w);
  if (has_n) m.normals.resize(3 * w);
  if (has_col) m.colors.resize(4 * w);
  size_t g = 0;
  for (size_t f = 0; f < nf; ++f) {
    if (new_id[m.faces[3 * f]] == (unsigned)-1) continue;
    for (int k = 0; k < 3; ++k) m.faces[3 * g + k] = new_id[m.faces[3 * f + k]];
    ++g;
  }
  m.faces.resize(3 * g);
  if (parts_dropped) *parts_dropped = n_parts - n_kept;
  if (orphans_dropped) *orphans_dropped = n_orphans;
}
