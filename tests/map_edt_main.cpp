// map_edt_main.cpp -- a stand-alone program (tests/test_map_edt_cpu.py builds it with AddressSanitizer + UBSan and runs it) for host/edt_box_voxels.hpp:
//   1. the box in metres: the centre rule lo <= (g + 1/2) * cell < hi voxel by voxel; a corner exactly on a centre goes in at lo and out at hi; an empty or
//      NaN box is refused;
//   2. the radius: floor(maxDist / cell) clamped to 1 .. 255;
//   3. the tile plan: the tiles of an axis cover it once, in order, none longer than 128; the voxel count of a box, refused above 2^31 without overflow.
#include "edt_box_voxels.hpp"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <limits>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void test_box() {
  const float cell = 1.f / 32.f;                              // a power of two: x / cell and (g + 1/2) * cell are exact
  const float xs[] = {-1.75f, -0.515625f, -0.5f, -2.5f / 32.f, -1.f / 64.f, 0.f, 1.f / 64.f, 3.f / 64.f, 4.5f / 32.f, 0.265625f, 1.f};
  long n = 0;
  for (float a : xs) for (float b : xs) {
    const float lo_m[3] = {a, a, a}, hi_m[3] = {b, b, b};
    int32_t lo[3]; uint32_t dims[3];
    const bool ok = hkf_edt_box_voxels(lo_m, hi_m, cell, lo, dims);
    int first = 0, count = 0;
    for (int g = -100; g < 100; ++g) {
      const double centre = ((double)g + 0.5) * (double)cell;
      if ((double)a <= centre && centre < (double)b) { if (!count) first = g; ++count; }
    }
    CHECK(ok == (count > 0), "[%g, %g): %d voxels by the rule, ok = %d", a, b, count, (int)ok);
    if (ok) for (int k = 0; k < 3; ++k) CHECK(lo[k] == first && dims[k] == (uint32_t)count, "[%g, %g): lo %d dims %u, the rule gives %d, %d", a, b, lo[k], dims[k], first, count);
    ++n;
  }
  {                                                            // corners exactly on the centres of voxels -3 and 4: -3 is in, 4 is out
    const float lo_m[3] = {-2.5f / 32.f, -2.5f / 32.f, -2.5f / 32.f}, hi_m[3] = {4.5f / 32.f, 4.5f / 32.f, 4.5f / 32.f};
    int32_t lo[3]; uint32_t dims[3];
    CHECK(hkf_edt_box_voxels(lo_m, hi_m, cell, lo, dims) && lo[0] == -3 && dims[0] == 7u && lo[2] == -3 && dims[2] == 7u, "on a centre: lo %d dims %u", lo[0], dims[0]);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float l2[3] = {0.f, nan, 0.f}, h2[3] = {1.f, 1.f, 1.f};
    CHECK(!hkf_edt_box_voxels(l2, h2, cell, lo, dims), "a NaN lower corner is refused");     // (hkf_erase_voxel_of clamps it to the low end: the axis would not be empty)
    const float l3[3] = {0.f, 0.f, 0.f}, h3[3] = {1.f, nan, 1.f};
    CHECK(!hkf_edt_box_voxels(l3, h3, cell, lo, dims), "a NaN upper corner is empty");
    const float l4[3] = {1.f, 0.f, 0.f}, h4[3] = {0.f, 1.f, 1.f};
    CHECK(!hkf_edt_box_voxels(l4, h4, cell, lo, dims) && dims[0] == 0u, "an inverted axis is empty");
    const float inf = std::numeric_limits<float>::infinity();
    const float l5[3] = {-inf, 0.f, 0.f}, h5[3] = {inf, 1.f, 1.f};
    CHECK(hkf_edt_box_voxels(l5, h5, cell, lo, dims) && lo[0] == -(1 << 23) && dims[0] == (1u << 24), "the whole key range: lo %d dims %u", lo[0], dims[0]);
  }
  printf("box: %ld comparisons\n", n);
}

static void test_radius() {
  const float cell = 3.0f / 128.0f;
  CHECK(hkf_edt_radius(0.f, cell) == 1u && hkf_edt_radius(-1.f, cell) == 1u && hkf_edt_radius(cell * 0.5f, cell) == 1u, "the clamp at 1");
  CHECK(hkf_edt_radius(std::numeric_limits<float>::quiet_NaN(), cell) == 1u, "NaN");
  CHECK(hkf_edt_radius(1.f, 1.f / 32.f) == 32u && hkf_edt_radius(1.f - 1.f / 1024.f, 1.f / 32.f) == 31u, "floor");
  CHECK(hkf_edt_radius(255.f / 32.f, 1.f / 32.f) == 255u && hkf_edt_radius(256.f / 32.f, 1.f / 32.f) == 255u, "the clamp at 255");
  CHECK(hkf_edt_radius(std::numeric_limits<float>::infinity(), cell) == 255u && hkf_edt_radius(1.f, 0.f) == 255u, "infinity");
  for (int r = 1; r <= 255; ++r) CHECK(hkf_edt_radius((float)((r + 0.5) * (double)cell), cell) == (uint32_t)r, "radius %d", r);
  printf("radius ok\n");
}

static void test_tiles() {
  const uint32_t ns[] = {1u, 2u, 127u, 128u, 129u, 255u, 256u, 257u, 1000u, 1u << 24};
  for (uint32_t n : ns) {
    const uint32_t t = hkf_edt_tile_count(n);
    uint64_t next = 0;
    for (uint32_t i = 0; i < t; ++i) {
      uint32_t off, len;
      hkf_edt_tile(n, i, &off, &len);
      CHECK(off == next && len >= 1u && len <= HKF_EDT_TILE, "n %u tile %u: off %u len %u", n, i, off, len);
      next = (uint64_t)off + len;
    }
    CHECK(next == n && t == (n + 127u) / 128u, "n %u: %u tiles end at %llu", n, t, (unsigned long long)next);
  }
  // the voxel count: exact below the bound, refused above it and for a zero dimension, with no overflow on the way (2^24 per axis is 2^72 voxels)
  {
    uint64_t n = 7;
    const uint32_t ok1[3] = {130u, 20u, 10u}, ok2[3] = {1u << 11, 1u << 10, 1u << 10}, big1[3] = {1u << 24, 1u << 24, 1u << 24}, big2[3] = {1u << 16, 1u << 16, 1u},
                   big3[3] = {(1u << 11) + 1u, 1u << 10, 1u << 10}, big4[3] = {1u, 1u << 24, 1u << 24}, zero[3] = {5u, 0u, 5u}, wrap[3] = {1u << 22, 1u << 21, 1u << 21};
    CHECK(hkf_edt_voxel_count(ok1, &n) && n == 26000ull, "130 x 20 x 10: %llu", (unsigned long long)n);
    CHECK(hkf_edt_voxel_count(ok2, &n) && n == HKF_EDT_MAX_VOXELS, "exactly the bound: %llu", (unsigned long long)n);
    CHECK(!hkf_edt_voxel_count(big1, &n) && n == 0ull, "2^72 voxels");
    CHECK(!hkf_edt_voxel_count(big2, &n) && !hkf_edt_voxel_count(big3, &n) && !hkf_edt_voxel_count(big4, &n), "above the bound");
    CHECK(!hkf_edt_voxel_count(wrap, &n) && n == 0ull, "2^64 voxels: the product would wrap to 0");
    CHECK(!hkf_edt_voxel_count(zero, &n), "a zero dimension");
  }
  // a tile passes the call's cap at every radius
  CHECK((uint64_t)HKF_EDT_TILE * (HKF_EDT_TILE + 2u * HKF_EDT_MAX_RADIUS) * (HKF_EDT_TILE + 2u * HKF_EDT_MAX_RADIUS) <= (1ull << 29), "a tile fits the cap");
  printf("tiles ok\n");
}

int main() {
  test_box();
  test_radius();
  test_tiles();
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("map edt ok\n");
  return 0;
}
