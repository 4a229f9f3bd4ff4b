// Stand-alone check of the moving volume's host arithmetic (hybkinectfu_amd/host/recentre.cpp): built with -fsanitize=address,undefined and run on
// the CPU by tests/test_shift_abi_cpu.py.  No device, no library: recentre.cpp is the only other translation unit.
#include "hybkf_host.hpp"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void pose_at(float p[16], float x, float y, float z) {
  for (int i = 0; i < 16; ++i) p[i] = (i % 5 == 0) ? 1.f : 0.f;
  p[3] = x; p[7] = y; p[11] = z;
}

int main() {
  float p[16]; int32_t d[3];
  const float size = 2.0f; const uint32_t res = 64;                       // cell 1 / 32, a brick 0.25 m
  pose_at(p, 1.f, 1.f, -0.3f);
  hkf_recentre_shift(p, size, res, 0.5f, d); EXPECT(d[0] == 0 && d[1] == 0 && d[2] == 0);
  hkf_recentre_shift(p, size, res, 0.f, d); EXPECT(d[0] == 0 && d[1] == 0 && d[2] == 0);        // off
  pose_at(p, 1.51f, 1.f, -0.3f);
  hkf_recentre_shift(p, size, res, 0.5f, d); EXPECT(d[0] == 16 && d[1] == 0 && d[2] == -8);
  pose_at(p, 0.3f, 1.f, -1.f);
  hkf_recentre_shift(p, size, res, 0.5f, d); EXPECT(d[0] == -16 && d[1] == 0 && d[2] == -32);   // toward zero: -2.8 bricks -> -2
  // values no volume reaches: the conversion stays defined and the result a multiple of 8
  const float wild[] = {1.0e30f, -1.0e30f, 3.0e38f, INFINITY, -INFINITY, NAN, 1.0e-40f};
  for (float w : wild) {
    pose_at(p, w, 1.f, -0.3f);
    hkf_recentre_shift(p, size, res, 0.5f, d);
    EXPECT(d[0] % 8 == 0 && d[1] % 8 == 0 && d[2] % 8 == 0);
    p[2] = w;                                                             // ... and in the rotation column
    hkf_recentre_shift(p, size, res, 0.5f, d);
    EXPECT(d[0] % 8 == 0 && d[1] % 8 == 0 && d[2] % 8 == 0);
  }
  hkf_recentre_shift(p, -1.f, res, 0.5f, d); EXPECT(d[0] == 0);
  hkf_recentre_shift(p, size, 0, 0.5f, d); EXPECT(d[0] == 0);
  // the origin offset: zero leaves every bit, otherwise one fp32 add per coordinate
  const int32_t zero[3] = {0, 0, 0}, org[3] = {16, -8, INT32_MIN};
  pose_at(p, -0.0f, 1.f, 2.f);
  hkf_world_pose(p, zero, 1.f / 32.f); EXPECT(signbit(p[3]) && p[7] == 1.f);
  hkf_world_pose(p, org, 1.f / 32.f); EXPECT(p[3] == 0.5f && p[7] == 0.75f && p[11] == 2.f + (float)INT32_MIN / 32.f);
  std::vector<float> v = {0.f, 0.f, 0.f, 1.f, 2.f, 3.f};
  hkf_world_positions(v.data(), 2, zero, 0.5f); EXPECT(v[3] == 1.f);
  hkf_world_positions(v.data(), 2, org, 1.f / 32.f); EXPECT(v[0] == 0.5f && v[1] == -0.25f && v[3] == 1.5f && v[4] == 1.75f);
  hkf_world_positions(v.data(), 0, org, 1.f / 32.f);
  hkf_world_positions(nullptr, 0, org, 1.f / 32.f);
  if (fails) return 1;
  printf("shift host arithmetic ok\n");
  return 0;
}
