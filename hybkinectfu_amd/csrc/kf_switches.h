// kf_switches.h -- every environment variable libhybkf.so reads, in one table (DESIGN.md "Switches" lists the same names).
// X(identifier, name, value when unset, cached, meaning): a switch is atoi() of its variable, or the "unset" value; a cached one is read on its first use in the
// process, an uncached one at every use.  What a value MEANS stays with the switch's user.  None is needed for normal use: every form gives the same bits.
#pragma once
#include <stdlib.h>
#ifdef KF_EXPERIMENTS            // the result-changing timing experiments: their names exist only in the variant built with -DKF_EXPERIMENTS (kf_internal.h: KF_EXP_ENV)
#define KF_SWITCH_EXP(X, ...) X(__VA_ARGS__)
#else
#define KF_SWITCH_EXP(X, ...)
#endif
#define KF_SWITCH_LIST(X) \
  X(INTEGRATE_SAT,         "KF_INTEGRATE_SAT",         1, 1, "deferred free-space weights: 0 never, 1 from 768^3, 2 always (kf_set_defer overrides per context)") \
  X(INTEGRATE_PAIRS,       "KF_INTEGRATE_PAIRS",       1, 1, "0: the scalar fusion kernel (k_integrate_bricks) without colour; no deferral") \
  X(INTEGRATE_COLOR_PAIRS, "KF_INTEGRATE_COLOR_PAIRS", 1, 1, "0: the scalar fusion kernel with colour") \
  X(INTEGRATE_BR,          "KF_INTEGRATE_BR",          0, 1, "1 | 2 | 4 bricks in flight per workgroup; anything else: 2 with colour, the size rule without") \
  X(INTEGRATE_PIPE,        "KF_INTEGRATE_PIPE",       -2, 1, "0 | 1: the plain one-brick loop / the two-stage pipeline; negative: the pipeline where the pass defers") \
  X(INTEGRATE_GRID,        "KF_INTEGRATE_GRID",        1, 1, "64..65536 workgroups of the fusion pass; anything else: the residency rule") \
  X(INTEGRATE_FREESPACE,   "KF_INTEGRATE_FREESPACE",   1, 1, "0: free-space voxels form their quotients too") \
  X(CULL_SIFT,             "KF_CULL_SIFT",            -1, 1, "0 | 1: macro cells one per wave / sifted one per lane first; negative: sifted from 100000 cells") \
  X(CULL_FINE,             "KF_CULL_FINE",            -1, 1, "0 | 1: the 8-pixel tile table off / on; negative: by the bricks' size on screen") \
  X(CULL_MACRO_DEPTH,      "KF_CULL_MACRO_DEPTH",      1, 1, "0: no depth test of whole macro cells") \
  X(CULL_IN_TRACK,         "KF_CULL_IN_TRACK",         1, 1, "0: the cull always in a launch of its own, never as the tail of the tracking launch") \
  X(OBSERVED_COUNT,        "KF_OBSERVED_COUNT",       -1, 1, "0: kf_get_volume_stats always sweeps; 1: counted from the first question; negative: after two questions in 8 frames") \
  X(PREFETCH_FUSED,        "KF_PREFETCH_FUSED",        1, 1, "0: kf_prefetch_frame on a side stream instead of riding in the raycast launch") \
  X(PREFETCH_IN_TRACK,     "KF_PREFETCH_IN_TRACK",     1, 1, "0: the next frame's filter never rides in the tracking launch") \
  X(RAYCAST_SHARED_GRAD,   "KF_RAYCAST_SHARED_GRAD",   1, 0, "0: six separate gradient lookups; 2: shared, every other wave forced down the fallback (tests)") \
  X(RAYCAST_VIEW_HALF,     "KF_RAYCAST_VIEW_HALF",     0, 0, "1..4095 brick layers of the gathers' view on either side (tests); anything else: most") \
  X(RAYCAST_PYRAMID,       "KF_RAYCAST_PYRAMID",       1, 1, "0: the model maps' pyramid levels are left to the tracker's launch") \
  X(RAYCAST_BOUNDS,        "KF_RAYCAST_BOUNDS",        1, 1, "0: no tile bounds; 2: through the super-cell list at any size (tests)") \
  X(RAYCAST_BOUNDS_MESO,   "KF_RAYCAST_BOUNDS_MESO",   1, 1, "0: small volumes' tile bounds from the macro table") \
  X(RAYCAST_MESO,          "KF_RAYCAST_MESO",          1, 1, "0: the meso table stays out of LDS") \
  X(RAYCAST_NEG_LDS,       "KF_RAYCAST_NEG_LDS",       1, 1, "0: brick flags from global memory at any size (tests)") \
  X(ICP_PERSISTENT,        "KF_ICP_PERSISTENT",        1, 1, "0: one launch per Gauss-Newton step, both trackers") \
  X(ICP_COOPERATIVE,       "KF_ICP_COOPERATIVE",       0, 1, "1: the persistent ICP loop as a cooperative launch") \
  X(ICP_BATCHED,           "KF_ICP_BATCHED",           1, 1, "0: images beyond one resident grid track per step") \
  X(ICP_BATCHED_ROOM,      "KF_ICP_BATCHED_ROOM",      0, 1, "resident workgroups of the batched loop, from 16; anything else: four fifths of the CUs") \
  X(SDF_PERSISTENT,        "KF_SDF_PERSISTENT",        1, 1, "0: the SDF tracker one launch per iteration") \
  X(SDF_LOOP_WG,           "KF_SDF_LOOP_WG",           0, 1, "workgroups of k_sdf_loop; 0 or less: one per CU") \
  KF_SWITCH_EXP(X, INTEGRATE_EXP, "KF_INTEGRATE_EXP",  0, 1, "experiments build: fusion-pass timing modes") \
  KF_SWITCH_EXP(X, ICP_EXP,       "KF_ICP_EXP",        0, 1, "experiments build: tracking-loop timing modes") \
  KF_SWITCH_EXP(X, RAYCAST_EXP,   "KF_RAYCAST_EXP",    0, 1, "experiments build: raycast timing modes")
enum kf_switch_id {
#define KF_SWITCH_ID(id, name, unset, cached, meaning) KF_SW_##id,
  KF_SWITCH_LIST(KF_SWITCH_ID) KF_SW_COUNT
#undef KF_SWITCH_ID
};
// the switch's value: the only place that consults the environment.  Hidden: one instance per library, never shared with a variant whose table has other rows
__attribute__((visibility("hidden"))) inline int kf_switch(kf_switch_id id) {
  static const struct { const char* name; int unset; int cached; } table[KF_SW_COUNT] = {
#define KF_SWITCH_ROW(id, name, unset, cached, meaning) {name, unset, cached},
    KF_SWITCH_LIST(KF_SWITCH_ROW)
#undef KF_SWITCH_ROW
  };
  static int value[KF_SW_COUNT]; static bool known[KF_SW_COUNT];
  if (known[id]) return value[id];
  const char* e = getenv(table[id].name);
  const int v = e ? atoi(e) : table[id].unset;
  if (table[id].cached) { value[id] = v; known[id] = true; }
  return v;
}
