// Stand-alone check of hkf_departing_boxes (hybkinectfu_amd/host/recentre.cpp): which cells a shift of the moving volume makes unextractable for
// good.  Built with -fsanitize=address,undefined and run on the CPU by tests/test_stream_abi_cpu.py.  No device, no library: recentre.cpp is the
// only other translation unit.  Every shift is checked against the rule stated cell by cell: a cell belongs to exactly one box if one of its
// voxels x-1 .. x+1 (each axis) leaves the window, and to none otherwise.
#include "hybkf_host.hpp"
#include <limits.h>
#include <stdio.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// does the stencil of cell c meet a voxel that leaves when the window moves by d along an axis of R voxels?
static bool departs(int c, long long d, int R) {
  for (int v = c - 1; v <= c + 1; ++v) {
    if (v < 0 || v >= R) continue;
    if ((d > 0 && v < d) || (d < 0 && v >= R + d)) return true;
  }
  return false;
}

static void check(const int32_t d[3], int R) {
  int32_t lo[3][3], hi[3][3];
  const int n = hkf_departing_boxes(d, (uint32_t)R, lo, hi);
  EXPECT(n >= 0 && n <= 3);
  std::vector<unsigned char> hits((size_t)R * R * R, 0);
  for (int b = 0; b < n; ++b) {
    for (int k = 0; k < 3; ++k) EXPECT(0 <= lo[b][k] && lo[b][k] < hi[b][k] && hi[b][k] <= R);
    for (int z = lo[b][2]; z < hi[b][2]; ++z)
      for (int y = lo[b][1]; y < hi[b][1]; ++y)
        for (int x = lo[b][0]; x < hi[b][0]; ++x) ++hits[((size_t)z * R + y) * R + x];
  }
  size_t bad = 0;
  for (int z = 0; z < R; ++z)
    for (int y = 0; y < R; ++y)
      for (int x = 0; x < R; ++x) {
        const bool want = departs(x, d[0], R) || departs(y, d[1], R) || departs(z, d[2], R);
        if (hits[((size_t)z * R + y) * R + x] != (want ? 1 : 0)) ++bad;
      }
  EXPECT(bad == 0);
}

int main() {
  const int32_t steps[] = {0, 8, -8, 24, -16, 64, -72, 4096, -4096, INT_MAX, INT_MIN};
  for (int R : {16, 24}) {
    for (int32_t dx : steps) for (int32_t dy : steps) for (int32_t dz : steps) { const int32_t d[3] = {dx, dy, dz}; check(d, R); }
  }
  int32_t lo[3][3], hi[3][3];
  const int32_t one[3] = {8, 0, 0}, none[3] = {0, 0, 0}, three[3] = {16, -8, 24};
  EXPECT(hkf_departing_boxes(none, 64, lo, hi) == 0);
  EXPECT(hkf_departing_boxes(one, 64, lo, hi) == 1 && lo[0][0] == 0 && hi[0][0] == 9 && lo[0][1] == 0 && hi[0][1] == 64 && lo[0][2] == 0 && hi[0][2] == 64);
  EXPECT(hkf_departing_boxes(three, 64, lo, hi) == 3);
  EXPECT(lo[0][0] == 0 && hi[0][0] == 17 && hi[0][1] == 64 && hi[0][2] == 64);                              // the x strip in full
  EXPECT(lo[1][0] == 17 && hi[1][0] == 64 && lo[1][1] == 55 && hi[1][1] == 64 && lo[1][2] == 0 && hi[1][2] == 64);     // the y strip without it
  EXPECT(lo[2][0] == 17 && hi[2][0] == 64 && lo[2][1] == 0 && hi[2][1] == 55 && lo[2][2] == 0 && hi[2][2] == 25);      // the z strip without both
  EXPECT(hkf_departing_boxes(one, 0, lo, hi) == 0);
  if (fails) return 1;
  printf("stream host arithmetic ok\n");
  return 0;
}
