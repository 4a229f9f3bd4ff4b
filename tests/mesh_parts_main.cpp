// Stand-alone driver of hybkinectfu_amd/host/mesh_parts.hpp for the sanitizer run of tests/test_mesh_parts_cpu.py (compiled with
// -fsanitize=address,undefined; MeshData itself comes from libhybkf_host.so).  Reads cases on stdin:
//   n_v n_f min_faces largest_only
//   n_v lines "x y z"   (integers: lattice coordinates, scaled by 0.01)
//   n_f lines "a b c"
// and prints per case: "labels ...", "sizes ...", then after dropParts "dropped P O", "kept ..." (the old indices of the kept vertices, carried
// through the drop in the colours) and "faces ...".  It asserts on the way that the drop copied positions, normals and colours verbatim, and that
// computeVertexNormals() on the cleaned mesh gives every normal the bytes it already had.  The last line is "mesh parts ok <cases>".
#include "hybkf_host.hpp"
#include "mesh_parts.hpp"
#include <stdio.h>
#include <string.h>
#include <vector>

static int fail(const char* what, unsigned n) { printf("FAILED case %u: %s\n", n, what); return 1; }

int main() {
  unsigned n_cases = 0, nv, nf, min_faces; int largest_only;
  while (scanf("%u %u %u %d", &nv, &nf, &min_faces, &largest_only) == 4) {
    MeshData m;
    m.vertices.resize((size_t)nv * 3); m.colors.resize((size_t)nv * 4); m.faces.resize((size_t)nf * 3);
    for (unsigned v = 0; v < nv; ++v) {
      int x, y, z;
      if (scanf("%d %d %d", &x, &y, &z) != 3) return fail("short vertex list", n_cases);
      m.vertices[3 * v] = (float)x * 0.01f; m.vertices[3 * v + 1] = (float)y * 0.01f; m.vertices[3 * v + 2] = (float)z * 0.01f;
      m.colors[4 * v] = (float)v; m.colors[4 * v + 1] = 0.25f; m.colors[4 * v + 2] = 0.5f; m.colors[4 * v + 3] = 1.0f;
    }
    for (unsigned f = 0; f < 3 * nf; ++f) {
      if (scanf("%u", &m.faces[f]) != 1 || m.faces[f] >= nv) return fail("bad face", n_cases);
    }
    m.computeVertexNormals();
    const MeshData before = m;
    std::vector<unsigned> labels, sizes;
    meshParts(m, labels, sizes);
    if (labels.size() != nv || sizes.size() != nv) return fail("sizes of the label arrays", n_cases);
    printf("labels"); for (unsigned v : labels) printf(" %u", v); printf("\n");
    printf("sizes"); for (unsigned v : sizes) printf(" %u", v); printf("\n");
    unsigned pd = 0, od = 0;
    dropParts(m, min_faces, largest_only != 0, &pd, &od);
    const size_t kv = m.vertices.size() / 3, kf = m.faces.size() / 3;
    if (m.normals.size() != kv * 3 || m.colors.size() != kv * 4) return fail("attribute sizes after the drop", n_cases);
    printf("dropped %u %u\n", pd, od);
    printf("kept");
    for (size_t v = 0; v < kv; ++v) {
      const unsigned old = (unsigned)m.colors[4 * v];
      if (old >= nv) return fail("a colour that is no old index", n_cases);
      if (memcmp(&m.vertices[3 * v], &before.vertices[3 * old], 12) || memcmp(&m.normals[3 * v], &before.normals[3 * old], 12) ||
          memcmp(&m.colors[4 * v], &before.colors[4 * old], 16)) return fail("an attribute was not copied verbatim", n_cases);
      printf(" %u", old);
    }
    printf("\nfaces");
    for (size_t f = 0; f < 3 * kf; ++f) { if (m.faces[f] >= kv) return fail("a face index out of range", n_cases); printf(" %u", m.faces[f]); }
    printf("\n");
    const std::vector<float> copied = m.normals;
    m.computeVertexNormals();                                         // every face of a kept vertex is kept, in order: the same sums, the same bits
    if (m.normals.size() != copied.size() || (copied.size() && memcmp(m.normals.data(), copied.data(), copied.size() * 4)))
      return fail("recomputed normals differ from the copied ones", n_cases);
    MeshData again = m;                                                // a second identical drop is the identity
    dropParts(again, min_faces, largest_only != 0, &pd, &od);
    if (pd || od || again.vertices != m.vertices || again.faces != m.faces) return fail("the second drop changed the mesh", n_cases);
    ++n_cases;
  }
  printf("mesh parts ok %u\n", n_cases);
  return 0;
}
