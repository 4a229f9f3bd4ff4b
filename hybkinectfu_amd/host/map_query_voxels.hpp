// map_query_voxels.hpp -- positions in WORLD metres as the fp64 world-voxel positions kf_map_sample and kf_map_cast_rays take (HybKinectfu::sampleMap,
// castMapRays).  Plain host C++, fp64; no device.
#pragma once
#include <stddef.h>

// World metres are the first cube's coordinates: those of the map mesh's vertices and of worldPose.  Voxel g covers [g, g + 1) * cell, its centre at
// (g + 1/2) * cell -- the frame eraseMapBox uses -- so the position in voxels is x / cell: one fp64 division by the fp32 cell widened, nothing else.
static inline void hkf_query_voxels(const double* world_m, size_t count3, float cell, double* vox) {
  const double c = (double)cell;
  for (size_t i = 0; i < count3; ++i) vox[i] = world_m[i] / c;
}
