// Stand-alone check of kf_strip_boxes (hybkinectfu_amd/csrc/strip_boxes.h): the one statement of the moving volume's strip rule.  Built with
// -fsanitize=address,undefined and run on the CPU by tests/test_stream_abi_cpu.py.  No device, no library: the header is all there is.
// For n in {1, 2, 5, 8}, both reaches and every move with components in [-n-2, n+2]: the boxes are non-empty, inside [0, n)^3, pairwise disjoint,
// come in the fixed order (x strip in full, y strip without the x strip, z strip without both), and their union is the set stated point by point:
//   reach 1 (cells): a cell belongs if one of its voxels c-1 .. c+1 leaves the window on some axis (the rule hkf_departing_boxes documents);
//   reach 0 (bricks): brick q leaves when q - s lies outside [0, n) on some axis; the bricks that enter (b + s outside) are the call with -s.
#include "strip_boxes.h"
#include <stdio.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// coordinate c of an axis of length n under a move s: does it belong to the axis' strip?
static bool in_strip(int c, int s, int n, int reach) {
  if (reach == 0) return c - s < 0 || c - s >= n;                 // the brick leaves
  for (int v = c - 1; v <= c + 1; ++v) {                          // the cell's stencil meets a voxel that leaves
    if (v < 0 || v >= n) continue;
    if ((s > 0 && v < s) || (s < 0 && v >= n + s)) return true;
  }
  return false;
}

static void check(const int s[3], int n, int reach, bool entering) {
  int32_t lo[3][3], hi[3][3];
  const int sg = entering ? -1 : 1;
  const int boxes = kf_strip_boxes(sg * s[0], sg * s[1], sg * s[2], n, reach, lo, hi);
  EXPECT(boxes >= 0 && boxes <= 3);
  std::vector<unsigned char> hits((size_t)n * n * n, 0);
  int last_axis = -1;
  for (int b = 0; b < boxes; ++b) {
    for (int k = 0; k < 3; ++k) EXPECT(0 <= lo[b][k] && lo[b][k] < hi[b][k] && hi[b][k] <= n);
    // the order: box b is the strip of an axis a beyond the last box's -- all of the axes after a, the strip on a, what the strips leave of the axes before a
    int a = -1;
    for (int k = last_axis + 1; k < 3 && a < 0; ++k) {
      bool is = true;
      for (int j = 0; j < 3 && is; ++j)
        for (int c = 0; c < n && is; ++c) {
          const bool inside = lo[b][j] <= c && c < hi[b][j];
          const bool want = j > k ? true : (j == k ? in_strip(c, sg * s[j], n, reach) : !in_strip(c, sg * s[j], n, reach));
          is = inside == want;
        }
      if (is) a = k;
    }
    EXPECT(a > last_axis);
    last_axis = a;
    for (int z = lo[b][2]; z < hi[b][2]; ++z)
      for (int y = lo[b][1]; y < hi[b][1]; ++y)
        for (int x = lo[b][0]; x < hi[b][0]; ++x) ++hits[((size_t)z * n + y) * n + x];
  }
  size_t bad = 0;
  for (int z = 0; z < n; ++z)
    for (int y = 0; y < n; ++y)
      for (int x = 0; x < n; ++x) {
        bool want;
        if (entering) want = x + s[0] < 0 || x + s[0] >= n || y + s[1] < 0 || y + s[1] >= n || z + s[2] < 0 || z + s[2] >= n;   // (reach 0 only)
        else want = in_strip(x, s[0], n, reach) || in_strip(y, s[1], n, reach) || in_strip(z, s[2], n, reach);
        if (hits[((size_t)z * n + y) * n + x] != (want ? 1 : 0)) ++bad;                                                      // exactly once, or never
      }
  EXPECT(bad == 0);
}

int main() {
  for (int n : {1, 2, 5, 8})
    for (int reach : {0, 1})
      for (int sx = -n - 2; sx <= n + 2; ++sx)
        for (int sy = -n - 2; sy <= n + 2; ++sy)
          for (int sz = -n - 2; sz <= n + 2; ++sz) {
            const int s[3] = {sx, sy, sz};
            check(s, n, reach, false);
            if (reach == 0) check(s, n, reach, true);
          }
  int32_t lo[3][3], hi[3][3];
  EXPECT(kf_strip_boxes(0, 0, 0, 8, 0, lo, hi) == 0 && kf_strip_boxes(0, 0, 0, 8, 1, lo, hi) == 0);
  EXPECT(kf_strip_boxes(2, -1, 3, 8, 0, lo, hi) == 3);
  EXPECT(lo[0][0] == 0 && hi[0][0] == 2 && lo[0][1] == 0 && hi[0][1] == 8 && lo[0][2] == 0 && hi[0][2] == 8);            // the x strip in full
  EXPECT(lo[1][0] == 2 && hi[1][0] == 8 && lo[1][1] == 7 && hi[1][1] == 8 && lo[1][2] == 0 && hi[1][2] == 8);            // the y strip without it
  EXPECT(lo[2][0] == 2 && hi[2][0] == 8 && lo[2][1] == 0 && hi[2][1] == 7 && lo[2][2] == 0 && hi[2][2] == 3);            // the z strip without both
  EXPECT(kf_strip_boxes(INT32_MAX, INT32_MIN, 0, 1 << 30, 1, lo, hi) == 1 && hi[0][0] == 1 << 30);                       // 64-bit inside: everything is the x strip
  if (fails) return 1;
  printf("strip boxes ok\n");
  return 0;
}
