// Stand-alone check of the map viewer's host arithmetic (hkf_view_frame, hybkinectfu_amd/host/recentre.cpp): built with -fsanitize=address,undefined and
// run on the CPU by tests/test_view_at_abi_cpu.py.  No device, no library: recentre.cpp is the only other translation unit.
#include "hybkf_host.hpp"
#include <math.h>
#include <stdio.h>
#include <string.h>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void pose_at(float p[16], float x, float y, float z) {
  for (int i = 0; i < 16; ++i) p[i] = (i % 5 == 0) ? 1.f : 0.f;
  p[3] = x; p[7] = y; p[11] = z;
}

int main() {
  float p[16], q[16]; int32_t f[3], d[3];
  const float size = 2.0f; const uint32_t res = 64;                       // cell 1 / 32, a brick 0.25 m
  pose_at(p, 1.f, 1.f, -0.3f);                                            // the focus (1, 1, 0.7) lies 0.3 m from the centre: closer than two bricks, frame -8 on z
  hkf_view_frame(p, size, res, f, q); EXPECT(f[0] == 0 && f[1] == 0 && f[2] == -8 && q[3] == 1.f && q[11] == -0.3f + 0.25f);
  pose_at(p, 1.2f, 0.9f, 0.1f);                                           // within one brick of the centre on every axis: frame 0, the pose as it came
  hkf_view_frame(p, size, res, f, q); EXPECT(f[0] == 0 && f[1] == 0 && f[2] == 0 && memcmp(p, q, sizeof(p)) == 0);
  pose_at(p, 1.51f, 1.f, -0.3f);                                          // where hkf_recentre_shift moves, the frame is its shift
  hkf_view_frame(p, size, res, f, q); hkf_recentre_shift(p, size, res, 0.5f, d);
  EXPECT(f[0] == 16 && f[1] == 0 && f[2] == -8 && d[0] == f[0] && d[1] == f[1] && d[2] == f[2]);
  EXPECT(q[3] == 1.51f - 16.f / 32.f && q[7] == 1.f && q[11] == -0.3f + 8.f / 32.f && q[0] == 1.f && q[15] == 1.f);
  pose_at(p, 5.3f, 1.f, -2.f);
  hkf_view_frame(p, size, res, f, q); EXPECT(f[0] == 136 && f[1] == 0 && f[2] == -64);
  // values no map reaches: the conversion stays defined; beyond the clamp the frame is +-8e6 voxels, a pose that is not finite gives frame 0 and the pose back
  const float wild[] = {1.0e30f, -1.0e30f, 3.0e38f, INFINITY, -INFINITY, NAN, 1.0e-40f};
  for (float w : wild) {
    for (int where = 0; where < 2; ++where) {
      pose_at(p, 1.f, 1.f, -0.3f);
      p[where ? 2 : 3] = w;                                               // in the translation, then in the rotation column
      hkf_view_frame(p, size, res, f, q);
      EXPECT(f[0] % 8 == 0 && f[1] % 8 == 0 && f[2] % 8 == 0 && f[0] >= -8000000 && f[0] <= 8000000);
      if (!(fabsf(w) <= 3.0e38f)) EXPECT(f[0] == 0 && f[1] == 0 && f[2] == 0 && memcmp(p, q, sizeof(p)) == 0);
    }
  }
  pose_at(p, 1.0e30f, 1.f, -0.3f);
  hkf_view_frame(p, size, res, f, q); EXPECT(f[0] == 8000000 && f[2] == -8);
  pose_at(p, 5.3f, 1.f, -2.f);
  hkf_view_frame(p, -1.f, res, f, q); EXPECT(f[0] == 0 && memcmp(p, q, sizeof(p)) == 0);
  hkf_view_frame(p, size, 0, f, q); EXPECT(f[0] == 0 && memcmp(p, q, sizeof(p)) == 0);
  hkf_view_frame(p, size, res, f, p);                                     // in place
  EXPECT(f[0] == 136 && p[3] == 5.3f - 136.f / 32.f);
  if (fails) return 1;
  printf("view frame arithmetic ok\n");
  return 0;
}
