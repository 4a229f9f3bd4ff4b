// map_erase_main.cpp -- a stand-alone program (tests/test_map_erase_cpu.py builds it with AddressSanitizer + UBSan and runs it):
//   1. csrc/erase_box.h: the class of a brick against a box equals a brute-force count of the brick's 512 voxels through the voxel test, for every brick of
//      [-3, 3)^3 against every box with corners in [-20, 20] in steps of 3 (empty and inverted boxes included), in both modes;
//   2. the clamp: INT32_MIN / INT32_MAX corners are legal, overflow nothing and mean "to the end of the key range";
//   3. host/erase_box_voxels.hpp: the voxel box of a box in metres equals the centre rule lo <= (g + 1/2) * cell < hi evaluated voxel by voxel.
#include "erase_box.h"
#include "erase_box_voxels.hpp"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <limits>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static int brute_class(const KfEraseBox& b, int mode, int kx, int ky, int kz) {
  int cleared = 0;
  for (int z = 0; z < 8; ++z) for (int y = 0; y < 8; ++y) for (int x = 0; x < 8; ++x)
    cleared += kf_erase_voxel_cleared(b, mode, 8 * kx + x, 8 * ky + y, 8 * kz + z) ? 1 : 0;
  return cleared == 0 ? KF_BRICK_UNTOUCHED : (cleared == 512 ? KF_BRICK_REMOVED : KF_BRICK_CUT);
}

// how many of the 8 voxels of brick coordinate k pass the voxel test along ONE axis of box [lo, hi): the real voxel test, on a box that spans the key
// range on the other two axes
static int brute_axis(int axis, int lo, int hi, int k) {
  int32_t l[3] = {KF_ERASE_VOX_MIN, KF_ERASE_VOX_MIN, KF_ERASE_VOX_MIN}, h[3] = {KF_ERASE_VOX_MAX, KF_ERASE_VOX_MAX, KF_ERASE_VOX_MAX};
  l[axis] = lo; h[axis] = hi;
  const KfEraseBox b = {l[0], l[1], l[2], h[0], h[1], h[2]};
  int n = 0;
  for (int v = 0; v < 8; ++v) {
    int g[3] = {0, 0, 0};
    g[axis] = 8 * k + v;
    n += kf_erase_voxel_cleared(b, KF_ERASE_BOX_INSIDE, g[0], g[1], g[2]) ? 1 : 0;
  }
  return n;
}

static void test_class() {
  std::vector<int> c;
  for (int v = -20; v <= 20; v += 3) c.push_back(v);
  const int nc = (int)c.size();                              // 14 corner values, 196 (lo, hi) pairs an axis, empty and inverted ones included
  // (a) the 512 voxels one by one through the three-dimensional voxel test: every corner pair on one axis against a short list of pairs on the other two
  const int zs[][2] = {{-14, 19}, {-5, 3}};
  long n = 0, seen[2][3] = {{0, 0, 0}, {0, 0, 0}};
  for (int axis = 0; axis < 3; ++axis) for (int l : c) for (int h : c) for (const auto& p : zs) for (const auto& q : zs) {
    int32_t lo[3], hi[3];
    lo[axis] = l; hi[axis] = h; lo[(axis + 1) % 3] = p[0]; hi[(axis + 1) % 3] = p[1]; lo[(axis + 2) % 3] = q[0]; hi[(axis + 2) % 3] = q[1];
    const KfEraseBox b = kf_erase_box_clamped(lo, hi);
    for (int mode = 0; mode < 2; ++mode)
      for (int kz = -3; kz < 3; ++kz) for (int ky = -3; ky < 3; ++ky) for (int kx = -3; kx < 3; ++kx) {
        const int got = kf_erase_brick_class(b, mode, kx, ky, kz), want = brute_class(b, mode, kx, ky, kz);
        CHECK(got == want, "box (%d %d %d)-(%d %d %d) mode %d brick (%d %d %d): %d, brute force %d", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], mode, kx, ky, kz, got, want);
        ++seen[mode][got]; ++n;
      }
  }
  for (int mode = 0; mode < 2; ++mode) for (int k = 0; k < 3; ++k) CHECK(seen[mode][k] > 1000, "mode %d class %d seen %ld times", mode, k, seen[mode][k]);
  printf("brick classes, voxel by voxel: %ld comparisons\n", n);
  // (b) EVERY box with corners in [-20, 20] in steps of 3 -- 14^6 of them -- against every brick of [-3, 3)^3 in both modes.  The voxel test is a
  // conjunction of three one-axis tests, so the brute-force count of the 512 voxels inside a box that is not empty is the product of three one-axis
  // counts, each taken voxel by voxel through the voxel test (brute_axis); an empty box holds none, and all
  // empty boxes are one box after the clamp.  (a) has checked that statement on 512 voxels.
  std::vector<int> cnt((size_t)3 * nc * nc * 6);
  for (int axis = 0; axis < 3; ++axis) for (int i = 0; i < nc; ++i) for (int j = 0; j < nc; ++j) for (int k = -3; k < 3; ++k)
    cnt[(((size_t)axis * nc + i) * nc + j) * 6 + (k + 3)] = brute_axis(axis, c[i], c[j], k);
  long m = 0, bad = 0, n_empty = 0;
  for (int ix = 0; ix < nc; ++ix) for (int jx = 0; jx < nc; ++jx) for (int iy = 0; iy < nc; ++iy) for (int jy = 0; jy < nc; ++jy)
    for (int iz = 0; iz < nc; ++iz) for (int jz = 0; jz < nc; ++jz) {
      const int32_t lo[3] = {c[ix], c[iy], c[iz]}, hi[3] = {c[jx], c[jy], c[jz]};
      const KfEraseBox b = kf_erase_box_clamped(lo, hi);
      const bool empty = ix >= jx || iy >= jy || iz >= jz;
      if (empty && n_empty++) {                              // every empty box clamps to ONE box, (0 0 0)-(0 0 0): its classes are compared once, below
        bad += !(b.lx == 0 && b.ly == 0 && b.lz == 0 && b.hx == 0 && b.hy == 0 && b.hz == 0);
        m += 432;
        continue;
      }
      const int *px = &cnt[(((size_t)0 * nc + ix) * nc + jx) * 6], *py = &cnt[(((size_t)1 * nc + iy) * nc + jy) * 6], *pz = &cnt[(((size_t)2 * nc + iz) * nc + jz) * 6];
      for (int kz = 0; kz < 6; ++kz) for (int ky = 0; ky < 6; ++ky) for (int kx = 0; kx < 6; ++kx) {
        const int in = empty ? 0 : px[kx] * py[ky] * pz[kz];
        for (int mode = 0; mode < 2; ++mode) {
          const int cleared = mode == KF_ERASE_BOX_INSIDE ? in : 512 - in;
          const int want = cleared == 0 ? KF_BRICK_UNTOUCHED : (cleared == 512 ? KF_BRICK_REMOVED : KF_BRICK_CUT);
          bad += kf_erase_brick_class(b, mode, kx - 3, ky - 3, kz - 3) != want;
          ++m;
        }
      }
    }
  CHECK(bad == 0, "%ld of %ld (box, brick, mode) classes differ from the brute-force count", bad, m);
  printf("brick classes, every box: %ld comparisons\n", m);
}

static void test_clamp() {
  const int32_t mn = std::numeric_limits<int32_t>::min(), mx = std::numeric_limits<int32_t>::max();
  const int32_t lo[3] = {mn, mn, mn}, hi[3] = {mx, mx, mx};
  const KfEraseBox all = kf_erase_box_clamped(lo, hi);
  CHECK(all.lx == KF_ERASE_VOX_MIN && all.ly == KF_ERASE_VOX_MIN && all.lz == KF_ERASE_VOX_MIN && all.hx == KF_ERASE_VOX_MAX && all.hy == KF_ERASE_VOX_MAX &&
        all.hz == KF_ERASE_VOX_MAX, "the whole int32 range clamps to the key range");
  const int edge[] = {-(1 << 20), -(1 << 20) + 1, -1, 0, 1, (1 << 20) - 2, (1 << 20) - 1};     // bricks at both ends of the key range
  for (int kx : edge) for (int ky : edge) for (int kz : edge) {
    CHECK(kf_erase_brick_class(all, KF_ERASE_BOX_INSIDE, kx, ky, kz) == KF_BRICK_REMOVED, "everything, inside: brick (%d %d %d)", kx, ky, kz);
    CHECK(kf_erase_brick_class(all, KF_ERASE_BOX_OUTSIDE, kx, ky, kz) == KF_BRICK_UNTOUCHED, "everything, outside: brick (%d %d %d)", kx, ky, kz);
    CHECK(brute_class(all, KF_ERASE_BOX_INSIDE, kx, ky, kz) == KF_BRICK_REMOVED, "brute force at (%d %d %d)", kx, ky, kz);
  }
  // half spaces: INT32_MIN to 3 on x cuts brick 0 and removes everything below it
  const int32_t hlo[3] = {mn, mn, mn}, hhi[3] = {3, mx, mx};
  const KfEraseBox half = kf_erase_box_clamped(hlo, hhi);
  CHECK(kf_erase_brick_class(half, 0, 0, 5, -7) == KF_BRICK_CUT && kf_erase_brick_class(half, 0, -1, 5, -7) == KF_BRICK_REMOVED &&
        kf_erase_brick_class(half, 0, -(1 << 20), 5, -7) == KF_BRICK_REMOVED && kf_erase_brick_class(half, 0, 1, 5, -7) == KF_BRICK_UNTOUCHED, "a half space");
  CHECK(kf_erase_brick_class(half, 1, 0, 5, -7) == KF_BRICK_CUT && kf_erase_brick_class(half, 1, -1, 5, -7) == KF_BRICK_UNTOUCHED &&
        kf_erase_brick_class(half, 1, (1 << 20) - 1, 5, -7) == KF_BRICK_REMOVED, "a half space, outside");
  // inverted and degenerate int32 boxes are empty
  const int32_t ilo[3] = {mx, 0, 0}, ihi[3] = {mn, 8, 8};
  const KfEraseBox inv = kf_erase_box_clamped(ilo, ihi);
  CHECK(inv.lx == 0 && inv.hx == 0 && inv.ly == 0 && inv.hy == 0 && inv.lz == 0 && inv.hz == 0, "an inverted box is the empty box");
  const int32_t plo[3] = {mx, mx, mx}, phi[3] = {mx, mx, mx};
  const KfEraseBox pt = kf_erase_box_clamped(plo, phi);
  CHECK(kf_erase_brick_class(pt, 0, (1 << 20) - 1, 0, 0) == KF_BRICK_UNTOUCHED && kf_erase_brick_class(pt, 1, 0, 0, 0) == KF_BRICK_REMOVED, "lo == hi is empty");
  for (int32_t v : {mn, mn + 1, -(1 << 23) - 1, -(1 << 23), -1, 0, 1, (1 << 23), (1 << 23) + 1, mx - 1, mx}) {
    const int32_t cl = kf_erase_clamp(v);
    CHECK(cl >= KF_ERASE_VOX_MIN && cl <= KF_ERASE_VOX_MAX && (v < KF_ERASE_VOX_MIN || v > KF_ERASE_VOX_MAX || cl == v), "clamp(%d) = %d", v, cl);
  }
  printf("clamp ok\n");
}

// the centre rule, voxel by voxel, over [g0, g1): the voxel box it gives on one axis (lo: the first voxel in; hi: one past the last voxel in); the
// box must lie inside the scanned range
static void centre_rule(double lo_m, double hi_m, double cell, int g0, int g1, int& lo, int& hi) {
  lo = hi = 0;
  bool any = false;
  for (int g = g0; g < g1; ++g) {
    const double centre = ((double)g + 0.5) * cell;
    if (lo_m <= centre && centre < hi_m) { if (!any) lo = g; hi = g + 1; any = true; }
  }
  if (!any) lo = hi = g0 - 1;                                // (marks "empty")
}

static void test_metres() {
  // cells that are powers of two: x / cell and (g + 1/2) * cell are exact, so the two statements must agree everywhere, ties included
  const float cells[] = {1.f / 32.f, 1.f / 64.f, 0.125f};
  const float xs[] = {-1.75f, -1.f, -0.515625f, -0.5f, -0.484375f, -1.f / 64.f, -1.f / 128.f, 0.f, 1.f / 128.f, 1.f / 64.f, 3.f / 64.f, 0.25f, 0.265625f, 0.984375f, 1.f, 1.5f};
  long n = 0;
  for (float cell : cells) for (float a : xs) for (float b : xs) {
    const float lo_m[3] = {a, a, b}, hi_m[3] = {b, a, a};
    int32_t lo[3], hi[3];
    hkf_erase_box_voxels(lo_m, hi_m, cell, lo, hi);
    for (int k = 0; k < 3; ++k) {
      int wl, wh;
      centre_rule(lo_m[k], hi_m[k], cell, -300, 300, wl, wh);
      if (wl == -301) CHECK(lo[k] >= hi[k], "cell %g [%g, %g): empty by the centre rule, got [%d, %d)", cell, lo_m[k], hi_m[k], lo[k], hi[k]);
      else CHECK(lo[k] == wl && hi[k] == wh, "cell %g [%g, %g): [%d, %d), the centre rule gives [%d, %d)", cell, lo_m[k], hi_m[k], lo[k], hi[k], wl, wh);
      ++n;
    }
  }
  // a corner exactly on a centre: in at lo, out at hi (cell 1 / 32: centre of voxel -3 is -2.5 / 32, of voxel 4 is 4.5 / 32)
  {
    const float cell = 1.f / 32.f;
    const float lo_m[3] = {-2.5f / 32.f, -2.5f / 32.f, 4.5f / 32.f}, hi_m[3] = {4.5f / 32.f, -2.5f / 32.f, 4.5f / 32.f};
    int32_t lo[3], hi[3];
    hkf_erase_box_voxels(lo_m, hi_m, cell, lo, hi);
    CHECK(lo[0] == -3 && hi[0] == 4, "on a centre: [%d, %d)", lo[0], hi[0]);
    CHECK(lo[1] == -3 && hi[1] == -3 && lo[2] == 4 && hi[2] == 4, "lo == hi on a centre is empty");
  }
  // a cell that is no power of two (3 m / 128): corners away from ties agree with the rule evaluated in fp64
  {
    const float cell = 3.0f / 128.0f;
    for (int i = -40; i <= 40; ++i) for (int j = -40; j <= 40; j += 7) {
      const float a = (float)(i * 0.0371), b = (float)(j * 0.0533 + 0.01);
      const float lo_m[3] = {a, a, a}, hi_m[3] = {b, b, b};
      int32_t lo[3], hi[3];
      hkf_erase_box_voxels(lo_m, hi_m, cell, lo, hi);
      const double fa = (double)a / (double)cell - 0.5, fb = (double)b / (double)cell - 0.5;
      if (fabs(fa - round(fa)) < 1e-6 || fabs(fb - round(fb)) < 1e-6) continue;      // a tie within rounding: the two statements may differ by design
      int wl, wh;
      centre_rule(a, b, cell, -200, 200, wl, wh);
      if (wl == -201) CHECK(lo[0] >= hi[0], "cell 3/128 [%g, %g): empty by the rule, got [%d, %d)", a, b, lo[0], hi[0]);
      else CHECK(lo[0] == wl && hi[0] == wh, "cell 3/128 [%g, %g): [%d, %d), the rule gives [%d, %d)", a, b, lo[0], hi[0], wl, wh);
      ++n;
    }
  }
  // not finite, or beyond the key range: clamped; NaN: an empty axis
  {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float lo_m[3] = {-inf, -3.0e38f, nan}, hi_m[3] = {inf, 3.0e38f, 1.f};
    int32_t lo[3], hi[3];
    hkf_erase_box_voxels(lo_m, hi_m, 1.f / 32.f, lo, hi);
    CHECK(lo[0] == KF_ERASE_VOX_MIN && hi[0] == KF_ERASE_VOX_MAX && lo[1] == KF_ERASE_VOX_MIN && hi[1] == KF_ERASE_VOX_MAX, "infinite and huge corners clamp");
    CHECK(lo[2] == KF_ERASE_VOX_MIN && hi[2] == 32, "a NaN lower corner: [%d, %d)", lo[2], hi[2]);
    const float l2[3] = {0.f, nan, inf}, h2[3] = {nan, nan, inf};
    hkf_erase_box_voxels(l2, h2, 1.f / 32.f, lo, hi);
    CHECK(lo[0] >= hi[0] && lo[1] >= hi[1] && lo[2] >= hi[2], "NaN upper corners and (inf, inf) give empty axes");
    const float l3[3] = {1.f, 1.f, 1.f}, h3[3] = {2.f, 2.f, 2.f};
    hkf_erase_box_voxels(l3, h3, 0.f, lo, hi);               // a zero cell divides to infinity: clamped, no undefined conversion
    CHECK(lo[0] == KF_ERASE_VOX_MAX && hi[0] == KF_ERASE_VOX_MAX, "cell 0");
    hkf_erase_box_voxels(l3, h3, nan, lo, hi);
    CHECK(lo[0] == KF_ERASE_VOX_MIN && hi[0] == KF_ERASE_VOX_MIN, "cell NaN");
  }
  printf("metres to voxels: %ld comparisons\n", n);
}

int main() {
  test_class();
  test_clamp();
  test_metres();
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("map erase ok\n");
  return 0;
}
