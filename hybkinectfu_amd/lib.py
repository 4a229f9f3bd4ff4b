"""ctypes binding of the C ABI in include/hybkf.h (libhybkf.so).

Python here is plumbing for tests and bench.py; the product is the shared library and the C++ host classes in
hybkinectfu_amd/host/.  There is NO CPU fallback: if the HIP library is missing, loading raises.
"""
import ctypes as C
import os
import weakref
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# KF_LIB: tools/ may point at the experiments variant (libhybkf_exp.so, `make -C csrc experiments`); default = the product library
LIB_PATH = os.environ.get("KF_LIB") or os.path.join(PKG_DIR, "libhybkf.so")


class CameraParams(C.Structure):
    _fields_ = [("cols", C.c_uint32), ("rows", C.c_uint32), ("cx", C.c_float), ("cy", C.c_float), ("fx", C.c_float), ("fy", C.c_float)]


class Mat44(C.Structure):
    _fields_ = [("m", C.c_float * 16)]

    @staticmethod
    def of(a):
        a = np.asarray(a, dtype=np.float32).reshape(16)
        return Mat44((C.c_float * 16)(*a.tolist()))

    def numpy(self):
        return np.array(list(self.m), dtype=np.float32).reshape(4, 4)


class IntegrateParams(C.Structure):
    _fields_ = [("sdf_truncation", C.c_float), ("max_integrate_dist", C.c_float)]


class RaycastParams(C.Structure):
    _fields_ = [("ray_increment", C.c_float)]


class VolumeParams(C.Structure):
    _fields_ = [("resolution", C.c_uint32), ("size_m", C.c_float), ("max_weight", C.c_float)]


class IcpParams(C.Structure):
    _fields_ = [("pyramid_levels", C.c_uint32), ("norm_sin_thres", C.c_float), ("dist_thres", C.c_float),
                ("dist_shake", C.c_float), ("angle_shake", C.c_float)]


class SdfTrackerParams(C.Structure):
    _fields_ = [("max_iter_nums", C.c_uint32), ("dist_shake", C.c_float), ("angle_shake", C.c_float)]


class Config(C.Structure):
    _fields_ = [("depth_camera", CameraParams), ("rgb_camera", CameraParams), ("volume", VolumeParams),
                ("pyramid_levels", C.c_uint32), ("max_triangles", C.c_uint32), ("has_color", C.c_int32), ("device", C.c_int32),
                ("slab_z_begin", C.c_uint32), ("slab_z_end", C.c_uint32), ("slab_halo", C.c_uint32)]


class TrackResult(C.Structure):
    _fields_ = [("pose", Mat44), ("tracked", C.c_int32), ("status", C.c_int32), ("iterations", C.c_int32), ("launch_form", C.c_int32)]


class VolumeStats(C.Structure):
    _fields_ = [("updated_last", C.c_uint64), ("weight_gt0", C.c_uint64), ("bricks_active", C.c_uint64), ("bricks_total", C.c_uint64),
                ("updated_total", C.c_uint64), ("frames_fused", C.c_uint64), ("frames_lost", C.c_uint64)]


class FusionForm(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("bricks", C.c_int32), ("defer", C.c_int32), ("color", C.c_int32), ("layers", C.c_int32),
                ("count", C.c_int32), ("cull", C.c_int32), ("cull_defer", C.c_int32), ("grid", C.c_uint32), ("calls", C.c_uint32)]


FUSE_NONE, FUSE_PAIRS, FUSE_PIPE, FUSE_BRICKS = 0, 1, 2, 3           # kf_fusion_form::kernel
CULL_NONE, CULL_TAIL, CULL_MACRO, CULL_SIFT = 0, 1, 2, 3             # kf_fusion_form::cull


class RaycastForm(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("fast", C.c_int32), ("output", C.c_int32), ("tile_bounds", C.c_int32), ("bounds_path", C.c_int32),
                ("meso_lds", C.c_int32), ("neg_lds", C.c_int32), ("shared_grad", C.c_int32), ("view_half", C.c_int32), ("pyramid", C.c_int32),
                ("grid", C.c_uint32), ("calls", C.c_uint32)]


RC_NONE, RC_PLAIN, RC_FILTER, RC_BEHIND = 0, 1, 2, 3                  # kf_raycast_form::kernel
RC_BOUNDS_NONE, RC_BOUNDS_MESO, RC_BOUNDS_MACRO, RC_BOUNDS_LIST = 0, 1, 2, 3    # kf_raycast_form::bounds_path
RC_OUT_MAPS, RC_OUT_T, RC_OUT_TA, RC_OUT_TA_SPEC = 0, 1, 2, 3          # kf_raycast_form::output


VERTEX_DTYPE = np.dtype([("pos", "<f4", (3,)), ("color", "<f4", (3,))])
TRI_DTYPE = np.dtype([("v", VERTEX_DTYPE, (3,))])

MC_WORLD, MC_TO_WORLD_SOUP = 1, 2                                     # kf_marching_cubes_region: flags

MAP_RAW_DEPTH, MAP_TRUNCED_DEPTH, MAP_FILTERED_DEPTH = 0, 1, 2
MAP_NEW_VERTICES, MAP_NEW_NORMALS, MAP_MODEL_VERTICES, MAP_MODEL_NORMALS = 3, 4, 5, 6
MAP_RAW_RGB, MAP_RAYCAST_RGB = 7, 8
VIEW_NORMALS, VIEW_SHADED, VIEW_COLOR = 0, 1, 2                      # kf_render_view / kf_view_model_maps: mode

# every symbol include/hybkf.h declares (tests check that the library exports each of them)
SYMBOLS = [
    "kf_error_string", "kf_version", "kf_create", "kf_destroy", "kf_synchronize", "kf_stream", "kf_reset_volume",
    "kf_upload_depth_mm", "kf_set_depth_mm_device", "kf_upload_rgb", "kf_trunc_depth", "kf_bilateral_filter_depth",
    "kf_calculate_new_vertices", "kf_calculate_new_normals", "kf_preprocess", "kf_prefetch_frame", "kf_downsample_new_vertices",
    "kf_downsample_new_normals", "kf_downsample_model_vertices", "kf_downsample_model_normals",
    "kf_cal_point_to_plane_solver_params", "kf_cal_sdf_solver_params", "kf_read_solver_params", "kf_set_pose",
    "kf_icp_track", "kf_sdf_track", "kf_read_track_result", "kf_request_track_result", "kf_wait_track_result", "kf_integrate_volume", "kf_raycast_volume",
    "kf_marching_cubes", "kf_clear_triangles", "kf_triangle_count", "kf_read_triangles", "kf_download_map",
    "kf_upload_map", "kf_download_volume", "kf_upload_volume", "kf_get_volume_stats", "kf_stored_z_range",
    "kf_stage_timers", "kf_read_stage_ms", "kf_read_work_counters", "kf_set_stream", "kf_raycast_volume_slab", "kf_slab_mask_candidates", "kf_set_model_maps_device", "kf_raycast_volume_slab_cross", "kf_slab_ray_normals", "kf_raycast_volume_slab_cross_spec", "kf_slab_ray_normals_spec", "kf_set_model_maps_rays", "kf_selftest_div",
    "kf_icp_partition_begin", "kf_icp_partition_steps", "kf_icp_partition_step", "kf_icp_partition_finish",
    "kf_sdf_partition_begin", "kf_sdf_partition_step", "kf_sdf_partition_finish", "kf_set_defer", "kf_inject_track_stall",
    "kf_download_volume_device", "kf_upload_volume_device", "kf_resize_slab", "kf_count_layer_work", "kf_read_layer_work",
    "kf_upload_depth_mm_next", "kf_take_next_depth", "kf_cull_tail_counts", "kf_count_observed_voxels", "kf_get_fusion_counters",
    "kf_get_fusion_form", "kf_get_raycast_form",
    "kf_write_triangles", "kf_weld_mesh", "kf_mesh_counts", "kf_read_mesh", "kf_weld_release",
    "kf_mesh_parts", "kf_read_mesh_parts", "kf_mesh_drop_parts",
    "kf_set_rgb_device", "kf_raycast_volume_slab_cross_spec_color", "kf_slab_ray_normals_color", "kf_set_model_maps_rays_color",
    "kf_render_view", "kf_render_view_at", "kf_view_model_maps", "kf_view_size", "kf_view_device", "kf_read_view",
    "kf_view_slab_cross", "kf_view_slab_normals", "kf_view_from_rays",
    "kf_shift_volume", "kf_volume_origin",
    "kf_marching_cubes_region", "kf_region_work", "kf_world_soup_reserve", "kf_world_soup_count", "kf_read_world_soup", "kf_clear_world_soup",
    "kf_append_world_soup", "kf_set_stream_out",
    "kf_brick_store_reserve", "kf_brick_store_count", "kf_brick_store_clear", "kf_read_brick_store", "kf_brick_store_bounds",
    "kf_write_brick_store", "kf_brick_store_capture", "kf_place_window",
    "kf_merge_brick_store", "kf_refill_window", "kf_merge_brick_store_rigid", "kf_rigid_brick_keys",
    "kf_align_brick_store", "kf_align_step",
    "kf_merge_brick_store_halved", "kf_halved_brick_keys",
    "kf_brick_store_erase_box", "kf_brick_store_erase_weak",
    "kf_map_sample", "kf_map_sample_device", "kf_map_cast_rays", "kf_map_cast_rays_device",
    "kf_map_distance_field", "kf_map_distance_field_device",
    "kf_map_score_poses", "kf_map_score_poses_device", "kf_map_pose_sums", "kf_map_refine_poses",
    "kf_marching_cubes_at", "kf_marching_cubes_map", "kf_map_tile_frames",
    "kf_slab_layer_bytes", "kf_slab_shift_needs", "kf_slab_needs", "kf_slab_pack_layers", "kf_shift_slab",
]


def build(force=False):
    """Compile the HIP sources in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(PKG_DIR, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j6"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def load():
    """dlopen libhybkf.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libhybkf.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.kf_error_string.restype = C.c_char_p
        _lib.kf_version.restype = C.c_char_p
        _lib.kf_stream.restype = C.c_void_p
        _lib.kf_view_device.restype = C.c_void_p
        _lib.kf_shift_volume.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        _lib.kf_volume_origin.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        _lib.kf_marching_cubes_region.argtypes = [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
        _lib.kf_region_work.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _lib.kf_world_soup_reserve.argtypes = [C.c_void_p, C.c_uint32]
        _lib.kf_world_soup_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.kf_read_world_soup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _lib.kf_clear_world_soup.argtypes = [C.c_void_p]
        _lib.kf_append_world_soup.argtypes = [C.c_void_p]
        _lib.kf_set_stream_out.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
        _lib.kf_brick_store_reserve.argtypes = [C.c_void_p, C.c_uint32]
        _lib.kf_brick_store_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib.kf_brick_store_clear.argtypes = [C.c_void_p]
        _lib.kf_read_brick_store.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.kf_brick_store_bounds.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _lib.kf_write_brick_store.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.kf_brick_store_capture.argtypes = [C.c_void_p]
        _lib.kf_place_window.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        _lib.kf_merge_brick_store.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        _lib.kf_refill_window.argtypes = [C.c_void_p]
        _lib.kf_merge_brick_store_rigid.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        _lib.kf_rigid_brick_keys.argtypes = [C.c_uint32, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_int64]
        _lib.kf_rigid_brick_keys.restype = C.c_int64
        _lib.kf_align_brick_store.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(AlignParams),
                                              C.POINTER(AlignReport)]
        _lib.kf_align_step.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.kf_merge_brick_store_halved.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.kf_halved_brick_keys.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int64]
        _lib.kf_halved_brick_keys.restype = C.c_int64
        _lib.kf_brick_store_erase_box.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        _lib.kf_brick_store_erase_weak.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_uint32)]
        for f in (_lib.kf_map_sample, _lib.kf_map_sample_device):
            f.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        for f in (_lib.kf_map_cast_rays, _lib.kf_map_cast_rays_device):
            f.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_float, C.c_uint32] + [C.c_void_p] * 5
        for f in (_lib.kf_map_score_poses, _lib.kf_map_score_poses_device):
            f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p]
        _lib.kf_map_pose_sums.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        _lib.kf_map_refine_poses.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RefineParams), C.c_void_p]
        for f in (_lib.kf_map_distance_field, _lib.kf_map_distance_field_device):
            f.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib.kf_marching_cubes_at.argtypes = [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
        _lib.kf_render_view_at.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        _lib.kf_marching_cubes_map.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_uint32)]
        _lib.kf_map_tile_frames.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int64]
        _lib.kf_map_tile_frames.restype = C.c_int64
        _lib.kf_slab_layer_bytes.argtypes = [C.c_void_p]
        _lib.kf_slab_layer_bytes.restype = C.c_size_t
        _lib.kf_slab_shift_needs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.kf_slab_pack_layers.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib.kf_shift_slab.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32]
    return _lib


def map_tiles(store_lo, store_hi, origin_vox, res):
    """the frames (n, 3) kf_marching_cubes_map visits, in order, for a store box (bricks, half-open), a window origin and a resolution (kf_map_tile_frames)"""
    lib = load()
    a, b, o = ((C.c_int32 * 3)(*[int(x) for x in v]) for v in (store_lo, store_hi, origin_vox))
    n = lib.kf_map_tile_frames(a, b, o, int(res), None, 0)
    if n < 0:
        raise KfError("kf_map_tile_frames: resolution %d" % res)
    out = np.zeros((n, 3), np.int32)
    if n:
        lib.kf_map_tile_frames(a, b, o, int(res), out.ctypes.data_as(C.c_void_p), n)
    return out


class KfError(RuntimeError):
    pass


def rigid_xf(xf):
    """a 3x4 [R | t] as the double[12] the C ABI takes"""
    return (C.c_double * 12)(*np.asarray(xf, np.float64).reshape(12).tolist())


def rigid_brick_keys(keys, xf):
    """the candidate destination bricks (n, 3), sorted by (z, y, x), of a source map with brick keys `keys` under xf = [R | t], source -> destination, t in
    voxels (kf_rigid_brick_keys)"""
    lib = load()
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
    x = rigid_xf(xf)
    n = lib.kf_rigid_brick_keys(len(keys), _p(keys), x, None, 0)
    if n < 0:
        raise KfError("kf_rigid_brick_keys: no rigid transform, or a candidate brick outside the key range")
    out = np.zeros((n, 3), np.int32)
    if n:
        lib.kf_rigid_brick_keys(len(keys), _p(keys), x, _p(out), n)
    return out


def halved_brick_keys(keys):
    """the coarse bricks (n, 3), unique and sorted by (z, y, x), of a map with brick keys `keys` at half its resolution: key >> 1 per component
    (kf_halved_brick_keys)"""
    lib = load()
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
    n = lib.kf_halved_brick_keys(len(keys), _p(keys), None, 0)
    if n < 0:
        raise KfError("kf_halved_brick_keys: a key component outside the key range")
    out = np.zeros((n, 3), np.int32)
    if n:
        lib.kf_halved_brick_keys(len(keys), _p(keys), _p(out), n)
    return out


ERASE_INSIDE, ERASE_OUTSIDE = 0, 1                                    # kf_brick_store_erase_box: mode
RAY_MISS, RAY_HIT, RAY_BROKEN = 0, 1, 2                               # kf_map_cast_rays: status
VOX_UNKNOWN, VOX_FREE, VOX_OCCUPIED = 0, 1, 2                         # kf_map_distance_field: the class byte; bit c of site_mask = class c
EDT_FAR = 0xFFFF                                                      # kf_map_distance_field: no site within the radius

ALIGN_CONVERGED, ALIGN_ITER_LIMIT, ALIGN_FEW_PAIRS, ALIGN_SINGULAR = 0, 1, 2, 3   # kf_align_report.verdict


class AlignParams(C.Structure):
    _fields_ = [("max_iter", C.c_uint32), ("min_pairs", C.c_uint32), ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("centre", C.c_double * 3)]


class AlignReport(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("verdict", C.c_uint32), ("sums", C.c_double * 29), ("rms", C.c_double), ("step", C.c_double * 6)]


class RefineParams(C.Structure):
    _fields_ = [("max_iter", C.c_uint32), ("min_pairs", C.c_uint32), ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("gate", C.c_float)]


# kf_pose_score: 24 bytes per pose
POSE_SCORE_DTYPE = np.dtype([("n_obs", "<u4"), ("n_in", "<u4"), ("n_behind", "<u4"), ("n_free", "<u4"), ("sum_q", "<u8")])


def align_params(centre, max_iter=25, min_pairs=1000, eps_rot=1e-9, eps_trans=1e-9):
    return AlignParams(int(max_iter), int(min_pairs), float(eps_rot), float(eps_trans), (C.c_double * 3)(*[float(x) for x in centre]))


def align_step(sums, centre, xf):
    """one Gauss-Newton step from the 29 sums: (the updated 3x4 transform, the step (omega, v)), or None when the solve refuses (kf_align_step)"""
    lib = load()
    s = (C.c_double * 29)(*np.asarray(sums, np.float64).reshape(29).tolist())
    c = (C.c_double * 3)(*np.asarray(centre, np.float64).reshape(3).tolist())
    x, step = rigid_xf(xf), (C.c_double * 6)()
    if lib.kf_align_step(s, c, x, step) != 0:
        return None
    return np.array(x[:], np.float64).reshape(3, 4), np.array(step[:], np.float64)


def _chk(st, what):
    if st != 0:
        raise KfError("%s failed: %d (%s)" % (what, st, load().kf_error_string(st).decode()))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def camera(cols, rows, cx, cy, fx, fy):
    return CameraParams(int(cols), int(rows), cx, cy, fx, fy)


def half_camera(c):
    """src/CameraPoseFinderICP.cpp:39-45 in fp32"""
    f = np.float32
    return CameraParams(c.cols // 2, c.rows // 2, f(c.cx) / f(2), f(c.cy) / f(2), f(c.fx) / f(2), f(c.fy) / f(2))


_LIVE = weakref.WeakSet()


def live_contexts():
    """Contexts created through this module and not yet closed (a second live kf_ctx switches the persistent loops off, so a
    leaked one changes launch forms: test harnesses close what a failed test left open)."""
    return [c for c in list(_LIVE) if c.h]


class Context:
    """One kf_ctx (one GPU / one z-slab)."""

    def __init__(self, depth_cam, volume_res, volume_size, max_weight=128.0, levels=3, max_triangles=0, has_color=False,
                 rgb_cam=None, device=0, slab=None, halo=0):
        self.lib = load()
        self.cam = depth_cam
        self.rgb_cam = rgb_cam if rgb_cam is not None else depth_cam
        self.res, self.size, self.levels = int(volume_res), float(volume_size), int(levels)
        self.has_color = bool(has_color)
        z0, z1 = slab if slab is not None else (0, volume_res)
        cfg = Config(depth_cam, self.rgb_cam, VolumeParams(volume_res, volume_size, max_weight), levels, max_triangles,
                     int(has_color), device, z0, z1, halo)
        self.h = C.c_void_p()
        _chk(self.lib.kf_create(C.byref(cfg), C.byref(self.h)), "kf_create")
        _LIVE.add(self)
        z0s, z1s = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_stored_z_range(self.h, C.byref(z0s), C.byref(z1s)), "kf_stored_z_range")
        self.stored = (z0s.value, z1s.value)
        self.owned = (z0, z1)

    @classmethod
    def borrow(cls, handle, depth_cam, volume_res, volume_size, levels=3):
        """Wrap a kf_ctx owned by someone else (the C++ host application): same methods, close() leaves it alone."""
        self = cls.__new__(cls)
        self.lib = load()
        self.cam = self.rgb_cam = depth_cam
        self.res, self.size, self.levels = int(volume_res), float(volume_size), int(levels)
        self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self.borrowed = True
        z0s, z1s = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_stored_z_range(self.h, C.byref(z0s), C.byref(z1s)), "kf_stored_z_range")
        self.stored = (z0s.value, z1s.value)
        self.owned = self.stored
        return self

    def close(self):
        if self.h:
            if not getattr(self, "borrowed", False):
                self.lib.kf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- uploads ----
    def upload_depth_mm(self, mm):
        mm = np.ascontiguousarray(mm, np.uint16)
        _chk(self.lib.kf_upload_depth_mm(self.h, _p(mm), mm.shape[1], mm.shape[0]), "kf_upload_depth_mm")
        self.sync()

    def upload_depth_mm_next(self, mm):
        """stage the NEXT frame while the current one is processed; returns its device address (for prefetch_frame)"""
        mm = np.ascontiguousarray(mm, np.uint16)
        dev = C.c_void_p()
        _chk(self.lib.kf_upload_depth_mm_next(self.h, _p(mm), mm.shape[1], mm.shape[0], C.byref(dev)), "kf_upload_depth_mm_next")
        return dev.value

    def take_next_depth(self):
        _chk(self.lib.kf_take_next_depth(self.h), "kf_take_next_depth")

    def set_depth_mm_device(self, dev_ptr):
        _chk(self.lib.kf_set_depth_mm_device(self.h, C.c_void_p(dev_ptr), self.cam.cols, self.cam.rows), "kf_set_depth_mm_device")

    def upload_rgb(self, bgr):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        _chk(self.lib.kf_upload_rgb(self.h, _p(bgr), bgr.shape[1], bgr.shape[0]), "kf_upload_rgb")

    def set_rgb_device(self, dev_ptr):
        """a BGR frame (rows x cols x 3 bytes) that is already on the device"""
        _chk(self.lib.kf_set_rgb_device(self.h, C.c_void_p(dev_ptr), self.rgb_cam.cols, self.rgb_cam.rows), "kf_set_rgb_device")

    def upload_map(self, map_id, level, arr):
        arr = np.ascontiguousarray(arr)
        _chk(self.lib.kf_upload_map(self.h, map_id, level, _p(arr), C.c_size_t(arr.nbytes)), "kf_upload_map")

    def download_map(self, map_id, level=0):
        cols, rows = self.cam.cols >> level, self.cam.rows >> level
        if map_id in (MAP_RAW_DEPTH, MAP_TRUNCED_DEPTH, MAP_FILTERED_DEPTH):
            out = np.empty((self.cam.rows, self.cam.cols), np.float32)
        elif map_id == MAP_RAW_RGB:
            out = np.empty((self.rgb_cam.rows, self.rgb_cam.cols, 3), np.uint8)
        elif map_id == MAP_RAYCAST_RGB:
            out = np.empty((self.cam.rows, self.cam.cols, 3), np.uint8)
        else:
            out = np.empty((rows, cols, 4), np.float32)
        _chk(self.lib.kf_download_map(self.h, map_id, level, _p(out), C.c_size_t(out.nbytes)), "kf_download_map")
        return out

    # ---- per-stage wrappers (1:1 with src/cuda/CudaWrappers.h) ----
    def trunc_depth(self, tmin, tmax):
        _chk(self.lib.kf_trunc_depth(self.h, C.c_float(tmin), C.c_float(tmax)), "kf_trunc_depth")

    def bilateral(self, sigma_pixel, sigma_depth):
        _chk(self.lib.kf_bilateral_filter_depth(self.h, C.c_float(sigma_pixel), C.c_float(sigma_depth)), "kf_bilateral_filter_depth")

    def calculate_new_vertices(self):
        _chk(self.lib.kf_calculate_new_vertices(self.h, C.byref(self.cam)), "kf_calculate_new_vertices")

    def calculate_new_normals(self):
        _chk(self.lib.kf_calculate_new_normals(self.h), "kf_calculate_new_normals")

    def preprocess(self, tmin, tmax, sigma_pixel, sigma_depth):
        _chk(self.lib.kf_preprocess(self.h, C.c_float(tmin), C.c_float(tmax), C.c_float(sigma_pixel), C.c_float(sigma_depth),
                                    C.byref(self.cam)), "kf_preprocess")

    def prefetch_frame(self, dev_ptr, tmin, tmax, sigma_pixel, sigma_depth):
        _chk(self.lib.kf_prefetch_frame(self.h, C.c_void_p(dev_ptr), self.cam.cols, self.cam.rows, C.c_float(tmin), C.c_float(tmax),
                                        C.c_float(sigma_pixel), C.c_float(sigma_depth), C.byref(self.cam)), "kf_prefetch_frame")

    def downsample(self, model):
        if model:
            _chk(self.lib.kf_downsample_model_vertices(self.h), "kf_downsample_model_vertices")
            _chk(self.lib.kf_downsample_model_normals(self.h), "kf_downsample_model_normals")
        else:
            _chk(self.lib.kf_downsample_new_vertices(self.h), "kf_downsample_new_vertices")
            _chk(self.lib.kf_downsample_new_normals(self.h), "kf_downsample_new_normals")

    def icp_system(self, level, cur, last_inv, cam, dist, sin):
        _chk(self.lib.kf_cal_point_to_plane_solver_params(self.h, level, C.byref(Mat44.of(cur)), C.byref(Mat44.of(last_inv)),
                                                          C.byref(cam), C.c_float(dist), C.c_float(sin)), "kf_cal_point_to_plane_solver_params")
        return self.read_solver_params()

    def sdf_system(self, cur):
        _chk(self.lib.kf_cal_sdf_solver_params(self.h, C.byref(self.cam), C.byref(Mat44.of(cur))), "kf_cal_sdf_solver_params")
        return self.read_solver_params()

    def read_solver_params(self):
        out = np.zeros(27, np.float32)
        _chk(self.lib.kf_read_solver_params(self.h, _p(out)), "kf_read_solver_params")
        return out

    # ---- device-resident tracking ----
    def set_pose(self, pose):
        _chk(self.lib.kf_set_pose(self.h, C.byref(Mat44.of(pose))), "kf_set_pose")

    def icp_track(self, frame_id, dist, sin, dist_shake, angle_shake):
        p = IcpParams(self.levels, sin, dist, dist_shake, angle_shake)
        _chk(self.lib.kf_icp_track(self.h, frame_id, C.byref(p), C.byref(self.cam)), "kf_icp_track")

    def icp_partition_track(self, frame_id, dist, sin, dist_shake, angle_shake, part, parts, dev_sums_ptr, all_reduce):
        """ICP with the pixels split over `parts` ranks; `all_reduce()` must sum the 32-float buffer at dev_sums_ptr over the ranks."""
        p = IcpParams(self.levels, sin, dist, dist_shake, angle_shake)
        _chk(self.lib.kf_icp_partition_begin(self.h, frame_id), "kf_icp_partition_begin")
        if frame_id == 0:
            return
        for step in range(self.lib.kf_icp_partition_steps(self.h)):
            _chk(self.lib.kf_icp_partition_step(self.h, step, C.byref(p), C.byref(self.cam), part, parts, C.c_void_p(dev_sums_ptr)),
                 "kf_icp_partition_step")
            all_reduce()
        _chk(self.lib.kf_icp_partition_finish(self.h, C.byref(p), C.c_void_p(dev_sums_ptr)), "kf_icp_partition_finish")

    def sdf_partition_track(self, frame_id, max_iter, dist_shake, angle_shake, dev_sums_ptr, all_reduce):
        """CameraPoseFinderSDF on a z-slab: this context sums the pixels whose world point it owns; `all_reduce()` must sum the 32-float
        buffer at dev_sums_ptr over the ranks (called max_iter times on every rank, whatever the convergence)."""
        p = SdfTrackerParams(max_iter, dist_shake, angle_shake)
        _chk(self.lib.kf_sdf_partition_begin(self.h, frame_id), "kf_sdf_partition_begin")
        if frame_id == 0:
            return
        for step in range(max_iter):
            _chk(self.lib.kf_sdf_partition_step(self.h, step, C.byref(p), C.byref(self.cam), C.c_void_p(dev_sums_ptr)), "kf_sdf_partition_step")
            all_reduce()
        _chk(self.lib.kf_sdf_partition_finish(self.h, C.byref(p), C.byref(self.cam), C.c_void_p(dev_sums_ptr)), "kf_sdf_partition_finish")

    def sdf_track(self, frame_id, max_iter, dist_shake, angle_shake):
        p = SdfTrackerParams(max_iter, dist_shake, angle_shake)
        _chk(self.lib.kf_sdf_track(self.h, frame_id, C.byref(p), C.byref(self.cam)), "kf_sdf_track")

    def inject_track_stall(self, launches=1):
        """fault injection: the next `launches` persistent-loop launches run with one workgroup playing dead (the frame is finished solo)"""
        _chk(self.lib.kf_inject_track_stall(self.h, int(launches)), "kf_inject_track_stall")

    def cull_tail_counts(self):
        """(consumed, undone): culls that ran as the tail of a tracking launch and were used by / discarded before the fusion pass"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_cull_tail_counts(self.h, C.byref(a), C.byref(b)), "kf_cull_tail_counts")
        return a.value, b.value

    def track_result(self):
        r = TrackResult()
        _chk(self.lib.kf_read_track_result(self.h, C.byref(r)), "kf_read_track_result")
        self.last_form = r.launch_form       # 1: persistent device loop, 2: one launch per Gauss-Newton step, 3: loop finished by one workgroup after a time-out (same pose bits), 0: none
        return bool(r.tracked), r.pose.numpy(), r.status, r.iterations

    # ---- volume ----
    def integrate(self, pose, sdf_trunc, max_dist, has_color=False, angle_weight=False):
        ip = IntegrateParams(sdf_trunc, max_dist)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_integrate_volume(self.h, int(has_color), int(angle_weight), tp, C.byref(ip), C.byref(self.cam),
                                          C.byref(self.rgb_cam)), "kf_integrate_volume")

    def fusion_form(self):
        """what the last integrate launched (kf_get_fusion_form): a dict of the kf_fusion_form fields"""
        f = FusionForm()
        _chk(self.lib.kf_get_fusion_form(self.h, C.byref(f)), "kf_get_fusion_form")
        return {name: int(getattr(f, name)) for name, _ in FusionForm._fields_}

    def set_defer(self, mode):
        """deferred free-space weights: 1 on, 0 off (the plain fusion kernel on every frame), -1 follow the environment"""
        _chk(self.lib.kf_set_defer(self.h, int(mode)), "kf_set_defer")

    def raycast(self, pose, inc, near, far, has_color=False):
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_raycast_volume(self.h, int(has_color), tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far)),
             "kf_raycast_volume")

    # ---- viewer frames ----
    def render_view(self, mode, pose, cam, inc, near, far, dev_v=None, dev_n=None):
        """a free viewpoint: march `cam` (lib.camera, any size) from `pose` (None: the device-resident pose) into the context's BGRA view image;
        dev_v / dev_n: optional device addresses of float4 maps of cam's size.  Asynchronous; tracking state is left alone (kf_render_view)"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_render_view(self.h, int(mode), tp, C.byref(cam), C.byref(rp), C.c_float(near), C.c_float(far),
                                     C.c_void_p(dev_v), C.c_void_p(dev_n)), "kf_render_view")

    def render_view_at(self, mode, frame_origin, pose, cam, inc, near, far, dev_v=None, dev_n=None):
        """render_view of a window that stands elsewhere: the bytes render_view would give after shift_volume(frame_origin - origin), store included,
        without moving anything.  `pose` in that frame's coordinates (None: the device-resident pose as that shift would leave it) (kf_render_view_at)"""
        rp = RaycastParams(inc) if inc is not None else None       # (frame_origin, cam, inc None: NULL -- refused, for the tests of the refusals)
        m = Mat44.of(pose) if pose is not None else None
        f = (C.c_int32 * 3)(*[int(x) for x in frame_origin]) if frame_origin is not None else None
        _chk(self.lib.kf_render_view_at(self.h, int(mode), f, C.byref(m) if m is not None else None, C.byref(cam) if cam is not None else None,
                                        C.byref(rp) if rp is not None else None, C.c_float(near), C.c_float(far), C.c_void_p(dev_v), C.c_void_p(dev_n)),
             "kf_render_view_at")

    def view_model_maps(self, mode):
        """the tracking camera's view from the current model maps, KF_MAP_RAYCAST_RGB and the device pose: no march (kf_view_model_maps)"""
        _chk(self.lib.kf_view_model_maps(self.h, int(mode)), "kf_view_model_maps")

    def view_size(self):
        """(cols, rows) of the last view"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_view_size(self.h, C.byref(a), C.byref(b)), "kf_view_size")
        return a.value, b.value

    def view_device(self):
        """device address of the last view's image (rows x cols x 4 bytes: b, g, r, a), valid in stream order; None before a view"""
        return self.lib.kf_view_device(self.h)

    def read_view(self):
        """the last view as a (rows, cols, 4) uint8 array (b, g, r, a); blocking"""
        cols, rows = self.view_size()
        out = np.empty((rows, cols, 4), np.uint8)
        _chk(self.lib.kf_read_view(self.h, _p(out), C.c_size_t(out.nbytes)), "kf_read_view")
        return out

    # the per-member steps of a merged view over z-slabs (group.Group.render_view runs them with the two all-reduces between)
    def view_slab_cross(self, color, pose, cam, inc, near, far, dev_ta, dev_ta_own, dev_spec):
        """raycast_slab_cross_spec (color: ..._spec_color, 4 words per pixel) for `cam`, any size; a bystander like render_view (kf_view_slab_cross)"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_view_slab_cross(self.h, int(bool(color)), tp, C.byref(cam), C.byref(rp), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta),
                                         C.c_void_p(dev_ta_own), C.c_void_p(dev_spec)), "kf_view_slab_cross")

    def view_slab_normals(self, color, pose, cam, inc, near, far, dev_ta_min, dev_ta_own, dev_spec, dev_cand):
        """slab_ray_normals_spec / _color for `cam`; dev_ta_own and dev_spec both None: every owned vertex is evaluated (kf_view_slab_normals)"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_view_slab_normals(self.h, int(bool(color)), tp, C.byref(cam), C.byref(rp), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta_min),
                                           C.c_void_p(dev_ta_own), C.c_void_p(dev_spec), C.c_void_p(dev_cand)), "kf_view_slab_normals")

    def view_from_rays(self, mode, pose, cam, dev_ta_min, dev_cand, words=3, dev_v=None, dev_n=None):
        """the merged crossing words and candidates (`words` per pixel) into the context's BGRA view image, optionally the float4 maps (kf_view_from_rays)"""
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_view_from_rays(self.h, int(mode), tp, C.byref(cam), C.c_void_p(dev_ta_min), C.c_void_p(dev_cand), int(words),
                                        C.c_void_p(dev_v), C.c_void_p(dev_n)), "kf_view_from_rays")

    def raycast_form(self):
        """what the last raycast launch took (kf_get_raycast_form): a dict of the kf_raycast_form fields"""
        f = RaycastForm()
        _chk(self.lib.kf_get_raycast_form(self.h, C.byref(f)), "kf_get_raycast_form")
        return {name: int(getattr(f, name)) for name, _ in RaycastForm._fields_}

    def raycast_slab(self, pose, inc, near, far, dev_t, dev_v, dev_n):
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_raycast_volume_slab(self.h, 0, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far),
                                             C.c_void_p(dev_t), C.c_void_p(dev_v), C.c_void_p(dev_n)), "kf_raycast_volume_slab")

    def slab_mask_candidates(self, dev_t, dev_tmin, dev_v, dev_n):
        _chk(self.lib.kf_slab_mask_candidates(self.h, C.c_void_p(dev_t), C.c_void_p(dev_tmin), C.c_void_p(dev_v), C.c_void_p(dev_n)),
             "kf_slab_mask_candidates")

    def raycast_slab_cross(self, pose, inc, near, far, dev_ta):
        """every ray's first crossing in the owned layers as one 64-bit word per pixel (crossing parameter << 32 | vertex parameter alpha)"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_raycast_volume_slab_cross(self.h, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta)),
             "kf_raycast_volume_slab_cross")

    def slab_ray_normals(self, pose, inc, near, far, dev_ta_min, dev_cand):
        """after the MIN all-reduce of the words: (normal, 1) for the winners whose vertex this context owns, zeros elsewhere"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_slab_ray_normals(self.h, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta_min),
                                          C.c_void_p(dev_cand)), "kf_slab_ray_normals")

    def raycast_slab_cross_spec(self, pose, inc, near, far, dev_ta, dev_ta_own, dev_spec):
        """raycast_slab_cross + a second copy of the words and the speculative normals of this context's own crossings (kf_raycast_volume_slab_cross_spec)"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_raycast_volume_slab_cross_spec(self.h, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta),
                                                        C.c_void_p(dev_ta_own), C.c_void_p(dev_spec)), "kf_raycast_volume_slab_cross_spec")

    def slab_ray_normals_spec(self, pose, inc, near, far, dev_ta_min, dev_ta_own, dev_spec, dev_cand):
        """slab_ray_normals that copies the speculative normal where this context's own crossing won and evaluates the rest"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_slab_ray_normals_spec(self.h, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta_min),
                                               C.c_void_p(dev_ta_own), C.c_void_p(dev_spec), C.c_void_p(dev_cand)), "kf_slab_ray_normals_spec")

    def set_model_maps_rays(self, pose, dev_ta_min, dev_cand):
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_set_model_maps_rays(self.h, tp, C.byref(self.cam), C.c_void_p(dev_ta_min), C.c_void_p(dev_cand)), "kf_set_model_maps_rays")

    # the colour forms: dev_spec / dev_cand hold 4 words per pixel (normal, colour word)
    def raycast_slab_cross_spec_color(self, pose, inc, near, far, dev_ta, dev_ta_own, dev_spec):
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_raycast_volume_slab_cross_spec_color(self.h, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta),
                                                              C.c_void_p(dev_ta_own), C.c_void_p(dev_spec)), "kf_raycast_volume_slab_cross_spec_color")

    def slab_ray_normals_color(self, pose, inc, near, far, dev_ta_min, dev_ta_own, dev_spec, dev_cand):
        """dev_ta_own / dev_spec None: every vertex this context owns is evaluated here (gradient and colour)"""
        rp = RaycastParams(inc)
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_slab_ray_normals_color(self.h, tp, C.byref(rp), C.byref(self.cam), C.c_float(near), C.c_float(far), C.c_void_p(dev_ta_min),
                                                C.c_void_p(dev_ta_own), C.c_void_p(dev_spec), C.c_void_p(dev_cand)), "kf_slab_ray_normals_color")

    def set_model_maps_rays_color(self, pose, dev_ta_min, dev_cand):
        tp = C.byref(Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_set_model_maps_rays_color(self.h, tp, C.byref(self.cam), C.c_void_p(dev_ta_min), C.c_void_p(dev_cand)), "kf_set_model_maps_rays_color")

    def set_model_maps_device(self, dev_v, dev_n):
        _chk(self.lib.kf_set_model_maps_device(self.h, C.c_void_p(dev_v), C.c_void_p(dev_n)), "kf_set_model_maps_device")

    def set_stream(self, hip_stream):
        _chk(self.lib.kf_set_stream(self.h, C.c_void_p(hip_stream)), "kf_set_stream")

    def marching_cubes(self, thr, has_color=False):
        _chk(self.lib.kf_marching_cubes(self.h, int(has_color), C.c_float(thr)), "kf_marching_cubes")

    def clear_triangles(self):
        _chk(self.lib.kf_clear_triangles(self.h), "kf_clear_triangles")

    def triangles(self):
        n = C.c_uint32()
        _chk(self.lib.kf_triangle_count(self.h, C.byref(n)), "kf_triangle_count")
        out = np.zeros(n.value, dtype=TRI_DTYPE)
        if n.value:
            _chk(self.lib.kf_read_triangles(self.h, _p(out), 0, n.value), "kf_read_triangles")
        return out

    def write_triangles(self, tris, first=0):
        """host triangles (lib.TRI_DTYPE) into the buffer at `first`; the triangle count becomes first + len(tris)"""
        tris = np.ascontiguousarray(tris)
        assert tris.dtype.itemsize == 72
        _chk(self.lib.kf_write_triangles(self.h, _p(tris), int(first), len(tris)), "kf_write_triangles")

    def weld_mesh(self, has_color=False, thresh=1e-4):
        """the buffer's triangles welded into an indexed mesh on the device (what saveMesh's host weld makes of them, bit for bit)"""
        _chk(self.lib.kf_weld_mesh(self.h, int(has_color), C.c_float(thresh)), "kf_weld_mesh")

    def mesh_counts(self):
        """(vertices, faces, rounds of the cell selection) of the last weld_mesh"""
        nv, nf, nr = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_mesh_counts(self.h, C.byref(nv), C.byref(nf), C.byref(nr)), "kf_mesh_counts")
        return nv.value, nf.value, nr.value

    def read_mesh(self, with_color=False):
        """the last weld_mesh's mesh: dict of vertices / normals (n, 3) f32, colors (n, 4) f32 -- (0, 4) without colour --, faces (m, 3) u32"""
        nv, nf, _ = self.mesh_counts()
        v, n = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32)
        c = np.empty((nv if with_color else 0, 4), np.float32)
        f = np.empty((nf, 3), np.uint32)
        _chk(self.lib.kf_read_mesh(self.h, _p(v), _p(n), _p(c) if with_color else None, _p(f)), "kf_read_mesh")
        return dict(vertices=v, normals=n, colors=c, faces=f)

    def mesh_parts(self):
        """(parts with a face, faces of the largest, orphans, labelling rounds) of the current mesh; include/hybkf.h has the rule"""
        n, big, orph, nr = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_mesh_parts(self.h, C.byref(n), C.byref(big), C.byref(orph), C.byref(nr)), "kf_mesh_parts")
        return n.value, big.value, orph.value, nr.value

    def read_mesh_parts(self):
        """per vertex of the current mesh: (label = smallest vertex index of its part, faces of its part), two (n_v,) u32 arrays"""
        nv = self.mesh_counts()[0]
        lab, cnt = np.empty(nv, np.uint32), np.empty(nv, np.uint32)
        _chk(self.lib.kf_read_mesh_parts(self.h, _p(lab), _p(cnt)), "kf_read_mesh_parts")
        return lab, cnt

    def mesh_drop_parts(self, min_faces=0, largest_only=False):
        """drops the parts with fewer than max(min_faces, 1) faces (largest_only: all but the largest) from the mesh on the device;
        returns (parts dropped, orphans dropped); mesh_counts / read_mesh report the cleaned mesh"""
        pd, od = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_mesh_drop_parts(self.h, C.c_uint32(int(min_faces)), int(bool(largest_only)), C.byref(pd), C.byref(od)), "kf_mesh_drop_parts")
        return pd.value, od.value

    def weld_release(self):
        _chk(self.lib.kf_weld_release(self.h), "kf_weld_release")

    def download_volume(self, z0=None, z1=None, color=False):
        z0 = self.stored[0] if z0 is None else z0
        z1 = self.stored[1] if z1 is None else z1
        shape = (z1 - z0, self.res, self.res)
        t, w = np.empty(shape, np.float32), np.empty(shape, np.float32)
        c = np.empty(shape + (3,), np.uint8) if color else None
        _chk(self.lib.kf_download_volume(self.h, z0, z1, _p(t), _p(w), _p(c) if color else None), "kf_download_volume")
        return (t, w, c) if color else (t, w)

    def upload_volume(self, tsdf, weight, color=None, z0=None):
        z0 = self.stored[0] if z0 is None else z0
        tsdf, weight = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
        z1 = z0 + tsdf.shape[0]
        cc = np.ascontiguousarray(color, np.uint8) if color is not None else None
        _chk(self.lib.kf_upload_volume(self.h, z0, z1, _p(tsdf), _p(weight), _p(cc) if cc is not None else None), "kf_upload_volume")

    def download_volume_device(self, z0, z1, dev_tsdf, dev_weight):
        _chk(self.lib.kf_download_volume_device(self.h, z0, z1, C.c_void_p(dev_tsdf), C.c_void_p(dev_weight), None), "kf_download_volume_device")

    def upload_volume_device(self, z0, z1, dev_tsdf, dev_weight):
        _chk(self.lib.kf_upload_volume_device(self.h, z0, z1, C.c_void_p(dev_tsdf), C.c_void_p(dev_weight), None), "kf_upload_volume_device")

    def resize_slab(self, z0, z1, halo):
        """own [z0, z1) (+ halo) from now on: layers stored before and after keep their voxels, new ones read as never observed"""
        _chk(self.lib.kf_resize_slab(self.h, z0, z1, halo), "kf_resize_slab")
        z0s, z1s = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_stored_z_range(self.h, C.byref(z0s), C.byref(z1s)), "kf_stored_z_range")
        self.stored, self.owned = (z0s.value, z1s.value), (z0, z1)

    def count_layer_work(self, frames):
        _chk(self.lib.kf_count_layer_work(self.h, int(frames)), "kf_count_layer_work")

    def read_layer_work(self, reset=True):
        out = np.zeros(self.res // 8, np.uint64)
        _chk(self.lib.kf_read_layer_work(self.h, _p(out), int(reset)), "kf_read_layer_work")
        return out

    def reset_volume(self):
        _chk(self.lib.kf_reset_volume(self.h), "kf_reset_volume")

    def shift_volume(self, dx, dy, dz):
        """the window moves by (dx, dy, dz) voxels, multiples of 8: contents, deferred weights and the device-resident pose move with it, in place
        and asynchronously; the model maps are stale until the next raycast (kf_shift_volume)"""
        _chk(self.lib.kf_shift_volume(self.h, int(dx), int(dy), int(dz)), "kf_shift_volume")

    def marching_cubes_region(self, thr, lo, hi, has_color=False, flags=0):
        """kf_marching_cubes for the cells lo <= (x, y, z) < hi only, appended to the triangle buffer (flags: MC_WORLD world coordinates,
        MC_TO_WORLD_SOUP into the world soup instead); its cost follows the box (kf_marching_cubes_region)"""
        l, h = (C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in hi])
        _chk(self.lib.kf_marching_cubes_region(self.h, int(has_color), thr, l, h, int(flags)), "kf_marching_cubes_region")

    def region_work(self):
        """(bricks whose voxels the class pass read, 256-cell blocks listed) of the last region extraction (kf_region_work)"""
        out = (C.c_uint64 * 2)()
        _chk(self.lib.kf_region_work(self.h, out), "kf_region_work")
        return int(out[0]), int(out[1])

    def world_soup_reserve(self, max_triangles):
        """(re)allocate and clear the world soup; 0 frees it (kf_world_soup_reserve)"""
        _chk(self.lib.kf_world_soup_reserve(self.h, int(max_triangles)), "kf_world_soup_reserve")

    def world_soup_count(self):
        """(triangles held, triangles that did not fit since the last clear)"""
        n, d = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_world_soup_count(self.h, C.byref(n), C.byref(d)), "kf_world_soup_count")
        return n.value, d.value

    def world_soup(self):
        """the world soup's triangles (lib.TRI_DTYPE), in world coordinates"""
        n, _ = self.world_soup_count()
        out = np.zeros(n, dtype=TRI_DTYPE)
        if n:
            _chk(self.lib.kf_read_world_soup(self.h, _p(out), 0, n), "kf_read_world_soup")
        return out

    def clear_world_soup(self):
        _chk(self.lib.kf_clear_world_soup(self.h), "kf_clear_world_soup")

    def append_world_soup(self):
        """device to device: the world soup behind what the triangle buffer holds, clamped (kf_append_world_soup)"""
        _chk(self.lib.kf_append_world_soup(self.h), "kf_append_world_soup")

    def slab_layer_bytes(self):
        """bytes of one brick layer in transit between two members (kf_slab_layer_bytes)"""
        return int(self.lib.kf_slab_layer_bytes(self.h))

    def slab_shift_needs(self, dz):
        """(bz_begin, bz_end): the global brick layers this context must be fed for a z shift of dz; (0, 0) when none (kf_slab_shift_needs)"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_slab_shift_needs(self.h, int(dz), C.byref(a), C.byref(b)), "kf_slab_shift_needs")
        return a.value, b.value

    def pack_layers(self, bz_begin, bz_end, dev_dst):
        """stored brick layers [bz_begin, bz_end) into the device buffer at address dev_dst, in the transit layout; asynchronous (kf_slab_pack_layers)"""
        _chk(self.lib.kf_slab_pack_layers(self.h, int(bz_begin), int(bz_end), C.c_void_p(int(dev_dst))), "kf_slab_pack_layers")

    def shift_slab(self, dx, dy, dz, dev_feed=None, feed=(0, 0)):
        """shift_volume for a context that stores only some brick layers: dev_feed (a device address) holds the brick layers `feed` = slab_shift_needs(dz)
        as their owners packed them; asynchronous, the model maps are stale afterwards (kf_shift_slab)"""
        _chk(self.lib.kf_shift_slab(self.h, int(dx), int(dy), int(dz), C.c_void_p(int(dev_feed)) if dev_feed else None, int(feed[0]), int(feed[1])),
             "kf_shift_slab")

    def set_stream_out(self, on, thr=0.0, has_color=False):
        """on: every shift_volume first extracts the surface that is about to leave into the world soup (kf_set_stream_out)"""
        _chk(self.lib.kf_set_stream_out(self.h, int(bool(on)), int(has_color), thr), "kf_set_stream_out")

    def brick_store_reserve(self, max_bricks):
        """(re)allocate and clear the brick store: from now on shift_volume keeps every observed brick that leaves and restores every brick that
        enters and is found; 0 frees it (kf_brick_store_reserve)"""
        _chk(self.lib.kf_brick_store_reserve(self.h, int(max_bricks)), "kf_brick_store_reserve")

    def brick_store_count(self):
        """(bricks held, bricks dropped for want of room, bricks restored) since the last clear (kf_brick_store_count)"""
        h, d, r = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _chk(self.lib.kf_brick_store_count(self.h, C.byref(h), C.byref(d), C.byref(r)), "kf_brick_store_count")
        return h.value, d.value, r.value

    def brick_store_clear(self):
        _chk(self.lib.kf_brick_store_clear(self.h), "kf_brick_store_clear")

    def brick_store(self, color=None):
        """(keys, tsdf, weight, color): everything the store holds -- keys[i] the world brick coordinate (x, y, z), tsdf[i] / weight[i] the brick as
        (8, 8, 8) in (z, y, x) order with the true weights, color[i] as (8, 8, 8, 3), None without a colour plane (kf_read_brick_store)"""
        color = getattr(self, "has_color", False) if color is None else color
        n = self.brick_store_count()[0]
        keys = np.zeros((n, 3), np.int32)
        t, w = np.zeros((n, 8, 8, 8), np.float32), np.zeros((n, 8, 8, 8), np.float32)
        c = np.zeros((n, 8, 8, 8, 3), np.uint8) if color else None
        if n:
            _chk(self.lib.kf_read_brick_store(self.h, 0, n, _p(keys), _p(t), _p(w), _p(c) if color else None), "kf_read_brick_store")
        return keys, t, w, c

    def write_brick_store(self, keys, tsdf, weight, color=None):
        """brick_store()'s inverse: every entry with a weight > 0 into the store under its key, a held key overwritten; keys (n, 3) world brick
        coordinates, each once; tsdf / weight (n, 8, 8, 8) in (z, y, x) order, true weights; color (n, 8, 8, 8, 3) or None (kf_write_brick_store)"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        n = len(keys)
        t, w = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
        c = np.ascontiguousarray(color, np.uint8) if color is not None else None
        assert t.size == n * 512 and w.size == n * 512 and (c is None or c.size == n * 1536)
        _chk(self.lib.kf_write_brick_store(self.h, n, _p(keys), _p(t), _p(w), _p(c) if c is not None else None), "kf_write_brick_store")

    def brick_store_capture(self):
        """every observed brick of the current window into the store, without a shift; nothing moves (kf_brick_store_capture)"""
        _chk(self.lib.kf_brick_store_capture(self.h), "kf_brick_store_capture")

    def place_window(self, x, y, z):
        """the window at origin (x, y, z) voxels, multiples of 8, filled from the store: what capture, a shift far away and a shift to there leave; the
        model maps are stale until the next raycast (kf_place_window)"""
        _chk(self.lib.kf_place_window(self.h, int(x), int(y), int(z)), "kf_place_window")

    def merge_brick_store(self, keys, tsdf, weight, color=None, offset=(0, 0, 0)):
        """write_brick_store's arguments, but a key the store holds is merged with the entry voxel by voxel -- the weighted running average, exact in
        fp32 -- instead of overwritten; offset: whole bricks added to every key first.  The store only: follow with refill_window() to see the result in
        the window (kf_merge_brick_store)"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        n = len(keys)
        t, w = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
        c = np.ascontiguousarray(color, np.uint8) if color is not None else None
        assert t.size == n * 512 and w.size == n * 512 and (c is None or c.size == n * 1536)
        off = (C.c_int32 * 3)(*(int(x) for x in offset)) if offset is not None else None
        _chk(self.lib.kf_merge_brick_store(self.h, n, _p(keys), _p(t), _p(w), _p(c) if c is not None else None, off), "kf_merge_brick_store")

    def merge_brick_store_rigid(self, keys, tsdf, weight, color, xf):
        """merge_brick_store's arrays, but the map is first resampled under xf = [R | t] (3x4, source world -> this store's world, t in voxels): trilinear
        in tsdf and colour, the least weight of the corners, unobserved where a corner is; then merged by the same rule (kf_merge_brick_store_rigid)"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        n = len(keys)
        t, w = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
        c = np.ascontiguousarray(color, np.uint8) if color is not None else None
        assert t.size == n * 512 and w.size == n * 512 and (c is None or c.size == n * 1536)
        _chk(self.lib.kf_merge_brick_store_rigid(self.h, n, _p(keys), _p(t), _p(w), _p(c) if c is not None else None, rigid_xf(xf)), "kf_merge_brick_store_rigid")

    def merge_brick_store_halved(self, keys, tsdf, weight, color=None):
        """merge_brick_store's arrays, read as a map of HALF this store's voxel size: every coarse voxel is formed from its eight children -- the mean
        tsdf of the observed ones, their least weight, their mean colour, unobserved where none is observed --; then merged by the same rule
        (kf_merge_brick_store_halved)"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        n = len(keys)
        t, w = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
        c = np.ascontiguousarray(color, np.uint8) if color is not None else None
        assert t.size == n * 512 and w.size == n * 512 and (c is None or c.size == n * 1536)
        _chk(self.lib.kf_merge_brick_store_halved(self.h, n, _p(keys), _p(t), _p(w), _p(c) if c is not None else None), "kf_merge_brick_store_halved")

    def align_brick_store(self, keys, tsdf, weight, xf, centre, max_iter=25, min_pairs=1000, eps_rot=1e-9, eps_trans=1e-9):
        """the rigid transform that lays the map (keys, tsdf, weight) onto this store, refined from the guess xf = [R | t] (3x4, source world -> this
        store's world, t in voxels) by Gauss-Newton on the SDF-to-SDF error; rotations are taken about `centre` (voxels).  Returns (the transform found,
        the AlignReport); max_iter = 0 only evaluates the sums at xf.  Nothing is merged and nothing changes (kf_align_brick_store)"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        n = len(keys)
        t, w = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
        assert t.size == n * 512 and w.size == n * 512
        x, rep = rigid_xf(xf), AlignReport()
        _chk(self.lib.kf_align_brick_store(self.h, n, _p(keys), _p(t), _p(w), x, C.byref(align_params(centre, max_iter, min_pairs, eps_rot, eps_trans)),
                                           C.byref(rep)), "kf_align_brick_store")
        return np.array(x[:], np.float64).reshape(3, 4), rep

    def brick_store_erase_box(self, lo, hi, mode=ERASE_INSIDE):
        """clears the voxels of the store inside the half-open box lo <= g < hi of world voxel indices (ERASE_OUTSIDE: outside it); bricks left with
        nothing observed are removed and their slots are free again.  The store only: capture first and refill_window() afterwards to erase from the
        map.  Returns (bricks removed, observed voxels cleared) (kf_brick_store_erase_box)"""
        l, h = (C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in hi])
        removed, cleared = C.c_uint32(), C.c_uint64()
        _chk(self.lib.kf_brick_store_erase_box(self.h, l, h, int(mode), C.byref(removed), C.byref(cleared)), "kf_brick_store_erase_box")
        return removed.value, cleared.value

    def brick_store_erase_weak(self, min_weight):
        """removes every brick of the store whose greatest true weight is below min_weight; the others stay bit for bit.  Returns the bricks removed
        (kf_brick_store_erase_weak)"""
        removed = C.c_uint32()
        _chk(self.lib.kf_brick_store_erase_weak(self.h, float(min_weight), C.byref(removed)), "kf_brick_store_erase_weak")
        return removed.value

    def map_sample(self, pos, want=("tsdf", "weight", "grad", "color")):
        """the map at points pos (n, 3), fp64, WORLD VOXEL units (voxel g's centre at g + 0.5), read where it lies -- window first, then the store: a dict
        of tsdf (n,), weight (n,), grad (n, 3) in tsdf units per voxel and color (n, 4); an unobserved point (one of its eight corners has weight 0) is 0
        everywhere.  want: which outputs to ask for, the others are passed as NULL (kf_map_sample)"""
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        n = len(pos)
        out = dict(tsdf=np.zeros(n, np.float32), weight=np.zeros(n, np.float32), grad=np.zeros((n, 3), np.float32), color=np.zeros((n, 4), np.uint8))
        out = {k: v for k, v in out.items() if k in want}
        a = [_p(out[k]) if k in out else None for k in ("tsdf", "weight", "grad", "color")]
        _chk(self.lib.kf_map_sample(self.h, n, _p(pos), *a), "kf_map_sample")
        return out

    def map_sample_device(self, n, dev_pos, dev_tsdf=None, dev_weight=None, dev_grad=None, dev_color=None):
        """map_sample with device pointers (integers or None), on the context's stream, non-blocking (kf_map_sample_device)"""
        _chk(self.lib.kf_map_sample_device(self.h, int(n), *[C.c_void_p(x) if x else None for x in (dev_pos, dev_tsdf, dev_weight, dev_grad, dev_color)]),
             "kf_map_sample_device")

    def map_cast_rays(self, origin, dirs, t_min, t_max, step, max_steps=1 << 24, want=("status", "t", "normal", "color", "weight")):
        """the first surface crossing of n rays through the map: origin (n, 3) fp64 in world voxels, dirs (n, 3) fp32 used as given, t_min / t_max (n,) or
        scalars, samples every `step`, at most max_steps of them.  A dict of status (n,) u8 (RAY_MISS, RAY_HIT, RAY_BROKEN), t (n,), normal (n, 3), color
        (n, 4), weight (n,); zeros where status is not RAY_HIT (kf_map_cast_rays)"""
        origin = np.ascontiguousarray(origin, np.float64).reshape(-1, 3)
        n = len(origin)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, np.float32), (n,)))
        t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float32), (n,)))
        assert len(dirs) == n
        out = dict(status=np.zeros(n, np.uint8), t=np.zeros(n, np.float32), normal=np.zeros((n, 3), np.float32), color=np.zeros((n, 4), np.uint8),
                   weight=np.zeros(n, np.float32))
        out = {k: v for k, v in out.items() if k in want}
        a = [_p(out[k]) if k in out else None for k in ("status", "t", "normal", "color", "weight")]
        _chk(self.lib.kf_map_cast_rays(self.h, n, _p(origin), _p(dirs), _p(t0), _p(t1), C.c_float(step), int(max_steps), *a), "kf_map_cast_rays")
        return out

    def map_cast_rays_device(self, n, dev_origin, dev_dir, dev_tmin, dev_tmax, step, max_steps, dev_status=None, dev_t=None, dev_normal=None,
                             dev_color=None, dev_weight=None):
        """map_cast_rays with device pointers (integers or None), on the context's stream, non-blocking (kf_map_cast_rays_device)"""
        ptr = [C.c_void_p(x) if x else None for x in (dev_origin, dev_dir, dev_tmin, dev_tmax, dev_status, dev_t, dev_normal, dev_color, dev_weight)]
        _chk(self.lib.kf_map_cast_rays_device(self.h, int(n), ptr[0], ptr[1], ptr[2], ptr[3], C.c_float(step), int(max_steps), *ptr[4:]),
             "kf_map_cast_rays_device")

    def map_score_poses(self, points, poses, band):
        """candidate camera poses scored against the map: points (n, 3) fp32 in the camera frame, voxel units; poses (k, 3, 4) fp64 [R | t], camera -> world
        voxels; band in (0, 1], tsdf units.  A (k,) array of POSE_SCORE_DTYPE: points observed, in the band, behind a surface, in free space, and the sum of
        the quantised |tsdf| (kf_map_score_poses)"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        out = np.zeros(len(poses), POSE_SCORE_DTYPE)
        _chk(self.lib.kf_map_score_poses(self.h, len(points), _p(points), len(poses), _p(poses), C.c_float(band), _p(out)), "kf_map_score_poses")
        return out

    def map_score_poses_device(self, n_points, dev_points, n_poses, dev_poses, band, dev_scores):
        """map_score_poses with device pointers (integers), on the context's stream, non-blocking (kf_map_score_poses_device)"""
        _chk(self.lib.kf_map_score_poses_device(self.h, int(n_points), C.c_void_p(dev_points), int(n_poses), C.c_void_p(dev_poses), C.c_float(band),
                                                C.c_void_p(dev_scores)), "kf_map_score_poses_device")

    def map_pose_sums(self, points, poses, centres, gate):
        """the 29 Gauss-Newton sums (kf_align_brick_store's layout) of each pose, (k, 29) fp64: points and poses as map_score_poses takes them, centres
        (k, 3) fp64 in world voxels, gate in (0, 1] (kf_map_pose_sums)"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        centres = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
        assert len(centres) == len(poses)
        out = np.zeros((len(poses), 29), np.float64)
        _chk(self.lib.kf_map_pose_sums(self.h, len(points), _p(points), len(poses), _p(poses), _p(centres), C.c_float(gate), _p(out)), "kf_map_pose_sums")
        return out

    def map_refine_poses(self, points, poses, centres, gate, max_iter=25, min_pairs=100, eps_rot=1e-9, eps_trans=1e-9):
        """Gauss-Newton from each pose on the map's distance at the points, all poses in one launch per iteration: (the refined poses (k, 3, 4), a list of
        k dicts of iterations, verdict (ALIGN_*), sums (29,), rms, step (6,)) (kf_map_refine_poses)"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        poses = np.array(poses, np.float64).reshape(-1, 12)
        centres = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
        assert len(centres) == len(poses)
        par = RefineParams(int(max_iter), int(min_pairs), float(eps_rot), float(eps_trans), float(gate))
        reps = (AlignReport * len(poses))()
        _chk(self.lib.kf_map_refine_poses(self.h, len(points), _p(points), len(poses), _p(poses), _p(centres), C.byref(par), reps), "kf_map_refine_poses")
        return poses.reshape(-1, 3, 4), [dict(iterations=r.iterations, verdict=r.verdict, sums=np.array(r.sums[:]), rms=r.rms, step=np.array(r.step[:])) for r in reps]

    def map_distance_field(self, lo_vox, dims, radius, level=0.0, site_mask=1 << VOX_OCCUPIED, want=("dist2", "cls")):
        """the map's distance field over the box of world voxels lo_vox (x, y, z), dims (nx, ny, nz): a dict of dist2 (nz, ny, nx) uint16 -- the squared
        distance in voxels to the nearest site of the map within `radius` (1 .. 255) voxels, EDT_FAR beyond -- and cls (nz, ny, nx) uint8 (VOX_UNKNOWN,
        VOX_FREE: tsdf > level, VOX_OCCUPIED).  The sites are the voxels whose class has its bit set in site_mask.  want: which outputs to ask for, the
        other is passed as NULL (kf_map_distance_field)"""
        lo, n = (C.c_int32 * 3)(*[int(x) for x in lo_vox]), (C.c_uint32 * 3)(*[int(x) for x in dims])
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        out = {k: v for k, v in dict(dist2=np.zeros(shape, np.uint16), cls=np.zeros(shape, np.uint8)).items() if k in want}
        a = [_p(out[k]) if k in out else None for k in ("dist2", "cls")]
        _chk(self.lib.kf_map_distance_field(self.h, lo, n, int(radius), C.c_float(level), int(site_mask), *a), "kf_map_distance_field")
        return out

    def map_distance_field_device(self, lo_vox, dims, radius, level=0.0, site_mask=1 << VOX_OCCUPIED, dev_dist2=None, dev_cls=None):
        """map_distance_field with device output pointers (integers or None), on the context's stream, non-blocking (kf_map_distance_field_device)"""
        lo, n = (C.c_int32 * 3)(*[int(x) for x in lo_vox]), (C.c_uint32 * 3)(*[int(x) for x in dims])
        _chk(self.lib.kf_map_distance_field_device(self.h, lo, n, int(radius), C.c_float(level), int(site_mask),
                                                   *[C.c_void_p(x) if x else None for x in (dev_dist2, dev_cls)]), "kf_map_distance_field_device")

    def refill_window(self):
        """the window re-read from the store under its current origin, without capturing it first: a window brick the store does not hold reads as never
        observed afterwards; pose and origin stay, the model maps are stale until the next raycast (kf_refill_window)"""
        _chk(self.lib.kf_refill_window(self.h), "kf_refill_window")

    def brick_store_bounds(self):
        """(lo, hi): the half-open box of the world brick coordinates the store holds; lo == hi for an empty or absent store (kf_brick_store_bounds)"""
        lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        _chk(self.lib.kf_brick_store_bounds(self.h, lo, hi), "kf_brick_store_bounds")
        return tuple(int(x) for x in lo), tuple(int(x) for x in hi)

    def marching_cubes_at(self, thr, frame_origin, lo, hi, has_color=False, flags=0):
        """marching_cubes_region in a virtual window at frame_origin (voxels, multiples of 8): the triangles the region call would give after
        shift_volume(frame_origin - origin), store included, without moving anything (kf_marching_cubes_at)"""
        f = (C.c_int32 * 3)(*[int(x) for x in frame_origin])
        l, h = (C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in hi])
        _chk(self.lib.kf_marching_cubes_at(self.h, int(has_color), thr, f, l, h, int(flags)), "kf_marching_cubes_at")

    def marching_cubes_map(self, thr, has_color=False, flags=MC_WORLD):
        """one mesh of everything ever fused -- brick store and window -- in world coordinates, appended to the triangle buffer tile by tile of a
        lattice fixed in the world; returns the number of tiles visited (kf_marching_cubes_map)"""
        n = C.c_uint32()
        _chk(self.lib.kf_marching_cubes_map(self.h, int(has_color), thr, int(flags), C.byref(n)), "kf_marching_cubes_map")
        return n.value

    def volume_origin(self):
        """(x, y, z): the sum of all shifts since the context was created / reset, in voxels (kf_volume_origin)"""
        o = (C.c_int32 * 3)()
        _chk(self.lib.kf_volume_origin(self.h, o), "kf_volume_origin")
        return tuple(int(x) for x in o)

    def stats(self, observed=True):
        """observed=False: kf_get_fusion_counters -- the update counters only (weight_gt0 = 0), no sweep, no effect on the observed-voxel count's bookkeeping"""
        s = VolumeStats()
        if not observed:
            _chk(self.lib.kf_get_fusion_counters(self.h, C.byref(s)), "kf_get_fusion_counters")
            return dict(updated_last=s.updated_last, weight_gt0=0, bricks_active=s.bricks_active, bricks_total=s.bricks_total,
                        updated_total=s.updated_total, frames_fused=s.frames_fused, frames_lost=s.frames_lost)
        _chk(self.lib.kf_get_volume_stats(self.h, C.byref(s)), "kf_get_volume_stats")
        if os.environ.get("KF_STATS_CROSSCHECK") == "1":       # tests/conftest.py: every stats() call checks the running count against a sweep of the volume
            swept = self.count_observed_voxels()
            if swept != s.weight_gt0:
                raise AssertionError("kf_get_volume_stats: running count of observed voxels %d != swept count %d" % (s.weight_gt0, swept))
        return dict(updated_last=s.updated_last, weight_gt0=s.weight_gt0, bricks_active=s.bricks_active, bricks_total=s.bricks_total,
                    updated_total=s.updated_total, frames_fused=s.frames_fused, frames_lost=s.frames_lost)

    def count_observed_voxels(self):
        """voxels of the owned layers with weight > 0, by a sweep of the volume (kf_get_volume_stats keeps the same number as a running count)"""
        n = C.c_uint64()
        _chk(self.lib.kf_count_observed_voxels(self.h, C.byref(n)), "kf_count_observed_voxels")
        return int(n.value)

    def stage_timers(self, mask):
        _chk(self.lib.kf_stage_timers(self.h, int(mask)), "kf_stage_timers")

    def read_stage_ms(self):
        ms = np.zeros(8, np.float32)
        cnt = np.zeros(8, np.uint32)
        _chk(self.lib.kf_read_stage_ms(self.h, _p(ms), _p(cnt)), "kf_read_stage_ms")
        return ms, cnt

    def work_counters(self):
        """(raycast reference samples, rays evaluated, bricks read by marching cubes, triangles) since stage_timers(mask | 1 << 16)"""
        out = (C.c_uint64 * 4)()
        _chk(self.lib.kf_read_work_counters(self.h, out), "kf_read_work_counters")
        return tuple(int(v) for v in out)

    def selftest_div(self, n, seed, mode):
        m = C.c_uint32(0)
        _chk(self.lib.kf_selftest_div(self.h, n, seed, mode, C.byref(m)), "kf_selftest_div")
        return m.value

    def sync(self):
        _chk(self.lib.kf_synchronize(self.h), "kf_synchronize")

    @property
    def stream(self):
        return self.lib.kf_stream(self.h)
