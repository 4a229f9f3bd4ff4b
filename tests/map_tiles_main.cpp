// A main of its own around csrc/map_tiles.h, for a sanitizer run on the CPU (tests/test_mapmesh_abi_cpu.py): reads cases
// "res  slo_x slo_y slo_z  shi_x shi_y shi_z  ox oy oz" (store box in bricks, half-open; window origin in voxels), one per line, and prints for each
// "tiles n" followed by n lines "fx fy fz" -- the frames kf_marching_cubes_map would visit, in order.  The list is asked for twice, once for its
// length and once into a buffer of exactly that length, as the library does.
#include "map_tiles.h"
#include <cstdio>
#include <vector>

int main() {
  int res, n_cases = 0;
  int32_t slo[3], shi[3], o[3];
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d", &res, &slo[0], &slo[1], &slo[2], &shi[0], &shi[1], &shi[2], &o[0], &o[1], &o[2]) == 10) {
    const int64_t n = kf_map_tiles(slo, shi, o, res, nullptr, 0);
    std::printf("tiles %lld\n", (long long)n);
    if (n < 0) { ++n_cases; continue; }
    std::vector<int32_t> frames((size_t)n * 3);
    if (kf_map_tiles(slo, shi, o, res, frames.data(), n) != n) { std::printf("second pass disagrees\n"); return 2; }
    for (int64_t t = 0; t < n; ++t) std::printf("%d %d %d\n", frames[3 * t], frames[3 * t + 1], frames[3 * t + 2]);
    if (n > 1) {                                             // a short buffer takes the first tiles only and still reports them all
      std::vector<int32_t> head(3);
      if (kf_map_tiles(slo, shi, o, res, head.data(), 1) != n || head[0] != frames[0] || head[1] != frames[1] || head[2] != frames[2]) { std::printf("short buffer wrong\n"); return 3; }
    }
    ++n_cases;
  }
  // the floor division at its sign changes
  if (kf_floor_div(-1, 48) != -1 || kf_floor_div(-48, 48) != -1 || kf_floor_div(-49, 48) != -2 || kf_floor_div(0, 48) != 0 || kf_floor_div(47, 48) != 0 || kf_floor_div(48, 48) != 1) {
    std::printf("floor division wrong\n"); return 4;
  }
  std::printf("map tiles ok %d\n", n_cases);
  return 0;
}
