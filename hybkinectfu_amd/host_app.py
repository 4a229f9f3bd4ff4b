"""ctypes binding of libhybkf_host.so: the C++ host classes (HybKinectfu, CameraPoseFinder*, MeshGeneratorMarchingcube)
driven the way src/MainController.cpp drives the reference.  One application per process (the reference uses singletons)."""
import ctypes as C
import os

import numpy as np

from . import lib as K

HOST_LIB = os.environ.get("KF_HOST_LIB") or os.path.join(K.PKG_DIR, "libhybkf_host.so")     # KF_HOST_LIB: the sanitizer build (CPU tests)
_h = None


def load():
    global _h
    if _h is None:
        K.load()
        if not os.path.exists(HOST_LIB):
            raise RuntimeError("libhybkf_host.so is missing: run __graft_entry__.build()")
        _h = C.CDLL(HOST_LIB)
        _h.hkf_app_ctx.restype = C.c_void_p
    return _h


class App:
    def __init__(self, res, size, cam, sdf_tracker=False, host_loop=False, max_triangles=0, sdf_trunc=0.0, integrate_dist=0.0,
                 trunc_max=0.0, device=0, slab=(0, 0), halo=0, dataset_dir="", traj_read="", traj_write="", use_rgb=False):
        """dataset_dir: TUM RGB-D directory (with trailing slash) read by process_dataset_frame; traj_read: trajectory file used
        INSTEAD of a tracker (CameraPoseFinderFromFile); traj_write: record the tracked poses there (TrajectoryRecorder)."""
        self.h = load()
        self.h.hkf_app_configure_io(dataset_dir.encode(), traj_read.encode(), traj_write.encode(), int(use_rgb))
        st = self.h.hkf_app_init(res, C.c_float(size), cam[0], cam[1], C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                 int(sdf_tracker), int(host_loop), max_triangles, C.c_float(sdf_trunc), C.c_float(integrate_dist),
                                 C.c_float(trunc_max), device, slab[0], slab[1], halo)
        if st:
            raise K.KfError("hkf_app_init failed: %d" % st)
        self.cam = cam

    def process_frame(self, mm, frame_id, stamp=0.0):
        mm = np.ascontiguousarray(mm, np.uint16)
        r = self.h.hkf_app_process_frame(mm.ctypes.data_as(C.c_void_p), 0, frame_id, C.c_double(stamp))
        if r < 0:
            raise K.KfError("processNewFrame failed: %d" % r)
        return bool(r)

    def process_dataset_frame(self, frame_id):
        """Next frame of the dataset directory through processNewFrame.  Returns (tracked, depth time stamp) or None at the end."""
        stamp = C.c_double(0.0)
        r = self.h.hkf_app_process_dataset_frame(frame_id, C.byref(stamp))
        if r == -3:
            return None
        if r < 0:
            raise K.KfError("dataset frame failed: %d" % r)
        return bool(r), stamp.value

    def enqueue_frame_device(self, dev_ptr, frame_id):
        r = self.h.hkf_app_enqueue_frame(C.c_void_p(dev_ptr), 1, frame_id)
        if r < 0:
            raise K.KfError("enqueueFrame failed: %d" % r)

    def pose(self):
        out = np.zeros(16, np.float32)
        tracked = self.h.hkf_app_get_pose(out.ctypes.data_as(C.c_void_p))
        return bool(tracked), out.reshape(4, 4)

    def ctx_handle(self):
        return C.c_void_p(self.h.hkf_app_ctx())

    def generate_mesh(self):
        return self.h.hkf_app_generate_mesh()

    def save_mesh(self, filename):
        nv, nf = C.c_uint32(), C.c_uint32()
        ok = self.h.hkf_app_save_mesh(filename.encode(), C.byref(nv), C.byref(nf))
        return bool(ok), nv.value, nf.value

    def set_device_weld(self, on=True):
        """save_mesh welds on the device (kf_weld_mesh) instead of on one host thread; same mesh, same files.  Default off."""
        if self.h.hkf_app_set_device_weld(int(bool(on))) != 0:
            raise K.KfError("hkf_app_set_device_weld: no application")

    def set_min_part_faces(self, n, largest_only=False):
        """save_mesh drops, after the weld, the mesh's connected parts with fewer than n faces (largest_only: all but the largest); on the device
        under set_device_weld, on the host otherwise, same file.  (0, False), the default, is off."""
        if self.h.hkf_app_set_min_part_faces(C.c_uint32(int(n)), int(bool(largest_only))) != 0:
            raise K.KfError("hkf_app_set_min_part_faces: no application")

    def render_view(self, mode, pose, cam):
        """HybKinectfu::renderView: `cam` = (cols, rows, cx, cy, fx, fy) from `pose` (None: the current camera pose), mode = lib.VIEW_*;
        returns (rows, cols, 4) uint8 (b, g, r, a).  Increment and planes are the application's."""
        out = np.empty((cam[1], cam[0], 4), np.uint8)
        p = np.ascontiguousarray(pose, np.float32).reshape(16) if pose is not None else None
        r = self.h.hkf_app_render_view(int(mode), p.ctypes.data_as(C.c_void_p) if p is not None else None, int(cam[0]), int(cam[1]),
                                       C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                       out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
        if r != 0:
            raise K.KfError("renderView failed: %d" % r)
        return out

    def render_view_at(self, mode, frame, pose, cam):
        """HybKinectfu::renderViewAt: render_view of the window as it would stand at `frame` (voxels of the first cube, multiples of 8), the brick
        store's bricks restored, without moving anything; `pose` in that frame's coordinates (None: the current camera pose, translated)"""
        out = np.empty((cam[1], cam[0], 4), np.uint8)
        p = np.ascontiguousarray(pose, np.float32).reshape(16) if pose is not None else None
        f = (C.c_int * 3)(*[int(x) for x in frame])
        r = self.h.hkf_app_render_view_at(int(mode), f, p.ctypes.data_as(C.c_void_p) if p is not None else None, int(cam[0]), int(cam[1]),
                                          C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                          out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
        if r != 0:
            raise K.KfError("renderViewAt failed: %d" % r)
        return out

    def render_map_view(self, mode, world_pose, cam):
        """HybKinectfu::renderMapView: a view of the MAP from `world_pose` (camera -> world in the first cube's coordinates): the window is placed
        around the view's focus (view_frame) and rendered there (render_view_at)"""
        out = np.empty((cam[1], cam[0], 4), np.uint8)
        p = np.ascontiguousarray(world_pose, np.float32).reshape(16)
        r = self.h.hkf_app_render_map_view(int(mode), p.ctypes.data_as(C.c_void_p), int(cam[0]), int(cam[1]),
                                           C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                           out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
        if r != 0:
            raise K.KfError("renderMapView failed: %d" % r)
        return out

    def view_model_maps(self, mode):
        """HybKinectfu::viewModelMaps: the tracking camera's view from the current model maps, (rows, cols, 4) uint8"""
        out = np.empty((self.cam[1], self.cam[0], 4), np.uint8)
        r = self.h.hkf_app_view_model_maps(int(mode), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
        if r != 0:
            raise K.KfError("viewModelMaps failed: %d" % r)
        return out

    def shift_volume(self, dx, dy, dz):
        """HybKinectfu::shiftVolume: the window moves by (dx, dy, dz) voxels (multiples of 8), the model maps are raycast anew; False: refused"""
        r = self.h.hkf_app_shift_volume(int(dx), int(dy), int(dz))
        if r < 0:
            raise K.KfError("hkf_app_shift_volume: no application")
        return bool(r)

    def volume_origin(self):
        """HybKinectfu::volumeOrigin: the sum of all shifts, in voxels"""
        o = (C.c_int * 3)()
        if self.h.hkf_app_volume_origin(o) != 0:
            raise K.KfError("hkf_app_volume_origin: no application")
        return tuple(int(x) for x in o)

    def set_recentre(self, dist):
        """AppParams::_volume_params.fRecentreDist: process_frame recentres the window after a tracked frame whose focus point lies farther
        than `dist` metres from the volume's centre (0: off, the default)"""
        if self.h.hkf_app_set_recentre(C.c_float(dist)) != 0:
            raise K.KfError("hkf_app_set_recentre: no application")

    def set_stream_mesh(self, max_triangles):
        """AppParams::_volume_params.nStreamMeshTriangles: reserve a world soup of that many triangles and stream the departing surface into it at
        every shift; generate_mesh then hands out [world soup, current window] in world coordinates (0: off, the default)"""
        r = self.h.hkf_app_set_stream_mesh(C.c_uint(int(max_triangles)))
        if r != 0:
            raise K.KfError("hkf_app_set_stream_mesh failed: %d" % r)

    def world_soup_count(self):
        """HybKinectfu::worldSoupCount: triangles streamed out so far"""
        r = self.h.hkf_app_world_soup_count()
        if r < 0:
            raise K.KfError("hkf_app_world_soup_count: no application")
        return r

    def set_brick_store(self, max_bricks):
        """AppParams::_volume_params.nBrickStoreBricks: reserve a brick store of that many bricks; every shift then keeps the observed bricks that
        leave the window and restores what it finds when the window returns (0: off, the default)"""
        r = self.h.hkf_app_set_brick_store(C.c_uint(int(max_bricks)))
        if r != 0:
            raise K.KfError("hkf_app_set_brick_store failed: %d" % r)

    def set_map_mesh(self, on=True):
        """MeshGeneratorMarchingcube::setMapMesh: with a brick store reserved, generate_mesh builds the map mesh -- store and window, world coordinates,
        every cell once (kf_marching_cubes_map) -- instead of [world soup, current window].  Default off."""
        if self.h.hkf_app_set_map_mesh(int(bool(on))) != 0:
            raise K.KfError("hkf_app_set_map_mesh: no application")

    def brick_store_count(self):
        """HybKinectfu::brickStoreCounts: (bricks held, bricks dropped for want of room, bricks restored)"""
        out = (C.c_uint64 * 3)()
        r = self.h.hkf_app_brick_store_count(out)
        if r != 0:
            raise K.KfError("hkf_app_brick_store_count failed: %d" % r)
        return int(out[0]), int(out[1]), int(out[2])

    def save_map(self, path):
        """HybKinectfu::saveMap: capture the window into the brick store (nothing moves) and write store, pose, origin and frame id to `path`;
        False: no store, a brick did not fit during the capture, or an I/O error"""
        r = self.h.hkf_app_save_map(os.fsencode(path))
        if r < 0:
            raise K.KfError("hkf_app_save_map: no application")
        return bool(r)

    def load_map(self, path):
        """HybKinectfu::loadMap: the file's map into the store, the window placed at the saved origin, pose and frame id set, the model maps raycast:
        the next process_frame is tracked against the loaded model.  False, with nothing touched: an unreadable, truncated or foreign file, or one
        of another resolution, size, max weight or colour"""
        r = self.h.hkf_app_load_map(os.fsencode(path))
        if r < 0:
            raise K.KfError("hkf_app_load_map: no application")
        return bool(r)

    def load_map_coarser(self, path):
        """HybKinectfu::loadMapCoarser: load_map for a file of 2, 4 or 8 times this application's resolution (same size, max weight and colour): the map is
        halved on the device, once per factor of two, the window placed at 8 * floor(origin / factor / 8) and the pose moved into its coordinates.  A file of
        this application's resolution is loaded as load_map loads it.  False, with nothing touched: any other file"""
        r = self.h.hkf_app_load_map_coarser(os.fsencode(path))
        if r < 0:
            raise K.KfError("hkf_app_load_map_coarser: no application")
        return bool(r)

    def merge_map(self, path, offset=(0, 0, 0)):
        """HybKinectfu::mergeMap: the file's map fused into this session's voxel by voxel (the weighted running average), its keys translated by
        `offset` whole bricks; the window shows the result and the next process_frame is tracked against it.  Pose and frame id stay.  False, with
        nothing touched: a file load_map would refuse, or a translated key outside the key range"""
        r = self.h.hkf_app_merge_map(os.fsencode(path), int(offset[0]), int(offset[1]), int(offset[2]))
        if r < 0:
            raise K.KfError("hkf_app_merge_map: no application")
        return bool(r)

    def merge_map_rigid(self, path, mat):
        """HybKinectfu::mergeMap under a rigid transform: `mat` (4x4, metres, as poses are) maps the file's world frame to this session's; the file's map is
        resampled at this session's voxel centres and merged.  False, with nothing touched: a file load_map would refuse, a matrix that is no rigid
        transform, a brick moved out of the key range"""
        m = np.ascontiguousarray(mat, np.float32).reshape(16)
        r = self.h.hkf_app_merge_map_rigid(os.fsencode(path), m.ctypes.data_as(C.c_void_p))
        if r < 0:
            raise K.KfError("hkf_app_merge_map_rigid: no application")
        return bool(r)

    def align_map(self, path, guess):
        """HybKinectfu::alignMap: the 4x4 (metres, as poses are) that lays the file's map onto this session's, refined from `guess`; a refinement, not a
        search.  Captures the window, merges nothing.  Returns (converged, the matrix found, the lib.AlignReport): pass the matrix to merge_map_rigid"""
        g = np.ascontiguousarray(guess, np.float32).reshape(16)
        found, rep = np.zeros(16, np.float32), K.AlignReport()
        r = self.h.hkf_app_align_map(os.fsencode(path), g.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p), C.byref(rep))
        if r < 0:
            raise K.KfError("hkf_app_align_map: no application")
        return bool(r), found.reshape(4, 4), rep

    def erase_map_box(self, lo, hi, keep_inside=False):
        """HybKinectfu::eraseMapBox: the voxels of this session's map whose centres lie in the box lo <= centre < hi (WORLD metres: the map mesh's
        coordinates) are cleared -- with keep_inside those outside it, which crops the map --, emptied bricks leave the store; the window shows the
        result and the next process_frame is tracked against it.  False, with nothing erased: a NaN corner, or a brick did not fit during the capture.
        The counts of the last call: erase_counts"""
        l, h = (C.c_float * 3)(*[float(x) for x in lo]), (C.c_float * 3)(*[float(x) for x in hi])
        out = (C.c_uint64 * 2)()
        r = self.h.hkf_app_erase_map_box(l, h, int(bool(keep_inside)), out)
        if r < 0:
            raise K.KfError("hkf_app_erase_map_box: no application")
        self.erase_counts = (int(out[0]), int(out[1]))
        return bool(r)

    def erase_map_weak(self, min_weight):
        """HybKinectfu::eraseMapWeak: every brick of this session's map whose greatest weight is below min_weight is removed, the others stay bit for bit;
        capture, window and raycast as erase_map_box.  erase_counts: (bricks removed, 0)"""
        out = (C.c_uint64 * 1)()
        r = self.h.hkf_app_erase_map_weak(C.c_float(min_weight), out)
        if r < 0:
            raise K.KfError("hkf_app_erase_map_weak: no application")
        self.erase_counts = (int(out[0]), 0)
        return bool(r)

    def sample_map(self, points):
        """HybKinectfu::sampleMap: this session's map at points (n, 3) in WORLD metres (the map mesh's coordinates), read where it lies -- window and
        store.  A dict of numpy arrays: distance (n,) in metres (tsdf * truncation), weight (n,), gradient (n, 3) of the distance per metre, color (n, 4);
        zeros where one of the point's eight corners was never observed"""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = len(pts)
        out = dict(distance=np.zeros(n, np.float32), weight=np.zeros(n, np.float32), gradient=np.zeros((n, 3), np.float32), color=np.zeros((n, 4), np.uint8))
        r = self.h.hkf_app_sample_map(K._p(pts), C.c_uint32(n), K._p(out["distance"]), K._p(out["weight"]), K._p(out["gradient"]), K._p(out["color"]))
        if r < 0:
            raise K.KfError("hkf_app_sample_map: no application")
        if r == 0:
            raise K.KfError("hkf_app_sample_map failed")
        return out

    def relocalise(self, mm, frame_id, params=None):
        """HybKinectfu::relocalise: finds the camera again in this session's map from the depth frame mm -- a lattice of candidate poses around params.guess
        (or the current pose) scored against the map, the best refined.  params: reloc_params(...), None for the defaults.  Returns (accepted, the report as
        a dict); accepted: the pose is set and the next process_frame tracks from it; otherwise nothing of the session changed"""
        mm = np.ascontiguousarray(mm, np.uint16)
        rep = RelocReport()
        r = self.h.hkf_app_relocalise(mm.ctypes.data_as(C.c_void_p), C.c_uint(int(frame_id)), C.byref(params) if params is not None else None, C.byref(rep))
        if r < 0:
            raise K.KfError("hkf_app_relocalise: no application")
        return bool(r), _report_dict(rep)

    def cast_map_rays(self, origins, dirs, t_min, t_max):
        """HybKinectfu::castMapRays: the first surface crossing of rays through this session's map: origins (n, 3) in WORLD metres, dirs (n, 3) used as
        given (unit vectors: t is metres), t_min / t_max (n,) or scalars in metres; the march steps by the raycaster's increment.  A dict of numpy arrays:
        status (n,) (K.RAY_MISS, K.RAY_HIT, K.RAY_BROKEN), t (n,) in metres, normal (n, 3), color (n, 4), weight (n,); zeros where status is not K.RAY_HIT"""
        org = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        n = len(org)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        assert len(d) == n
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, np.float32), (n,)))
        t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float32), (n,)))
        out = dict(status=np.zeros(n, np.uint8), t=np.zeros(n, np.float32), normal=np.zeros((n, 3), np.float32), color=np.zeros((n, 4), np.uint8),
                   weight=np.zeros(n, np.float32))
        r = self.h.hkf_app_cast_map_rays(K._p(org), K._p(d), K._p(t0), K._p(t1), C.c_uint32(n), K._p(out["status"]), K._p(out["t"]), K._p(out["normal"]),
                                         K._p(out["color"]), K._p(out["weight"]))
        if r < 0:
            raise K.KfError("hkf_app_cast_map_rays: no application")
        if r == 0:
            raise K.KfError("hkf_app_cast_map_rays failed")
        return out

    def distance_field_box(self, lo_m, hi_m, max_dist_m):
        """the box distance_field computes for these corners, without computing it: (lo_vox (x, y, z), dims (nx, ny, nz), the radius in voxels) -- voxel g is in
        the box iff lo_m <= (g + 1/2) * cell < hi_m, the radius is floor(max_dist_m / cell) clamped to 1 .. 255.  KfError for an empty box, a NaN corner or a
        box of more than 2^31 voxels"""
        l, h = (C.c_float * 3)(*[float(x) for x in lo_m]), (C.c_float * 3)(*[float(x) for x in hi_m])
        lo, dims, radius = (C.c_int32 * 3)(), (C.c_uint32 * 3)(), C.c_uint32()
        r = self.h.hkf_app_distance_field_box(l, h, C.c_float(max_dist_m), lo, dims, C.byref(radius))
        if r < 0:
            raise K.KfError("hkf_app_distance_field_box: no application")
        if r == 0:
            raise K.KfError("hkf_app_distance_field_box: an empty box, or one too large")
        return tuple(int(v) for v in lo), tuple(int(v) for v in dims), int(radius.value)

    def distance_field(self, lo_m, hi_m, max_dist_m, level=0.0, site_mask=1 << K.VOX_OCCUPIED):
        """HybKinectfu::distanceField: the clearance in this session's map over the box lo_m <= voxel centre < hi_m (WORLD metres, erase_map_box's rule): the
        distance in metres from every voxel of the box to the nearest site -- a voxel whose class (K.VOX_UNKNOWN, K.VOX_FREE: tsdf > level, K.VOX_OCCUPIED) has
        its bit set in site_mask -- up to floor(max_dist_m / cell) voxels, clamped to 1 .. 255.  Returns (dist float32 (nz, ny, nx): sqrt(d2) * cell, inf
        where no site lies within the radius; cls uint8 (nz, ny, nx); the radius used, voxels).  Where the box lies in voxels: distance_field_box"""
        _, dims, _ = self.distance_field_box(lo_m, hi_m, max_dist_m)
        l, h = (C.c_float * 3)(*[float(x) for x in lo_m]), (C.c_float * 3)(*[float(x) for x in hi_m])
        shape = (dims[2], dims[1], dims[0])
        dist, cls = np.zeros(shape, np.float32), np.zeros(shape, np.uint8)
        radius = C.c_uint32()
        r = self.h.hkf_app_distance_field(l, h, C.c_float(max_dist_m), C.c_float(level), C.c_uint32(site_mask), C.c_uint64(dist.size), K._p(dist), K._p(cls),
                                          None, None, C.byref(radius))
        if r <= 0:
            raise K.KfError("hkf_app_distance_field failed")
        return dist, cls, int(radius.value)

    def frame_id(self):
        """HybKinectfu::frameId: the id of the last frame processed, or the one load_map set"""
        r = self.h.hkf_app_frame_id()
        if r < 0:
            raise K.KfError("hkf_app_frame_id: no application")
        return r

    def close(self):
        self.h.hkf_app_shutdown()


def map_file_info(path):
    """hkf_map_file_info: the header of a map file after every check of the reader (magic, version, brick edge, length, keys ascending, unique and in
    range), as a dict; raises KfError with the reader's code for a file it refuses.  Needs no GPU."""
    h = load()
    u, f, o, fid = (C.c_uint32 * 4)(), (C.c_float * 2)(), (C.c_int32 * 3)(), C.c_uint32()
    pose, q = np.zeros(16, np.float32), (C.c_uint64 * 2)()
    h.hkf_map_file_info.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    r = h.hkf_map_file_info(os.fsencode(path), u, f, o, C.byref(fid), pose.ctypes.data_as(C.c_void_p), q)
    if r != 0:
        raise K.KfError("map file refused: %d" % r)
    return dict(version=int(u[0]), resolution=int(u[1]), brick_edge=int(u[2]), has_color=bool(u[3]), size=float(f[0]), max_weight=float(f[1]),
                origin_vox=tuple(int(x) for x in o), frame_id=int(fid.value), pose=pose.reshape(4, 4), n_bricks=int(q[0]), dropped=int(q[1]))


SLABS_LIB = os.path.join(K.PKG_DIR, "libhybkf_slabs.so")
_s = None


class RelocParams(C.Structure):
    """host/reloc_search.hpp: RelocParams"""
    _fields_ = [("has_guess", C.c_int32), ("guess", C.c_float * 16), ("trans_step", C.c_float), ("rot_step", C.c_float), ("n", C.c_int32 * 6),
                ("top", C.c_uint32), ("max_points", C.c_uint32), ("level", C.c_int32), ("min_obs", C.c_uint32), ("band", C.c_float), ("gate", C.c_float),
                ("accept_inliers", C.c_float), ("max_iter", C.c_uint32), ("min_pairs", C.c_uint32), ("eps_rot", C.c_double), ("eps_trans", C.c_double)]


class PoseScore(C.Structure):
    _fields_ = [("n_obs", C.c_uint32), ("n_in", C.c_uint32), ("n_behind", C.c_uint32), ("n_free", C.c_uint32), ("sum_q", C.c_uint64)]


class RelocReport(C.Structure):
    """host/reloc_search.hpp: RelocReport"""
    _fields_ = [("candidates", C.c_uint32), ("points", C.c_uint32), ("best_index", C.c_uint32), ("verdict", C.c_uint32), ("iterations", C.c_uint32),
                ("accepted", C.c_int32), ("best_score", PoseScore), ("refined_score", PoseScore), ("best_pose", C.c_double * 12), ("refined_pose", C.c_double * 12),
                ("median_depth", C.c_float), ("trans_step", C.c_float), ("rot_step", C.c_float)]


def reloc_params(guess=None, **kw):
    """the defaults of HybKinectfu::relocalise (hkf_reloc_defaults_get) with the given fields replaced; guess: a 4x4 camera -> WORLD metres pose; n: six ints"""
    par = RelocParams()
    load().hkf_reloc_defaults_get(C.byref(par))
    if guess is not None:
        par.has_guess = 1
        par.guess = (C.c_float * 16)(*np.asarray(guess, np.float32).reshape(16).tolist())
    for k, v in kw.items():
        if k == "n":
            par.n = (C.c_int32 * 6)(*[int(x) for x in v])
        else:
            assert hasattr(par, k), k
            setattr(par, k, v)
    return par


def _report_dict(rep):
    sc = lambda s: {k: int(getattr(s, k)) for k in ("n_obs", "n_in", "n_behind", "n_free", "sum_q")}
    return dict(candidates=rep.candidates, points=rep.points, best_index=rep.best_index, verdict=rep.verdict, iterations=rep.iterations, accepted=bool(rep.accepted),
                best_score=sc(rep.best_score), refined_score=sc(rep.refined_score), best_pose=np.array(rep.best_pose[:]).reshape(3, 4),
                refined_pose=np.array(rep.refined_pose[:]).reshape(3, 4), median_depth=rep.median_depth, trans_step=rep.trans_step, rot_step=rep.rot_step)


def reloc_points(verts, cell, max_points):
    """hkf_reloc_points: (the points (n, 3) float32 in voxels, the median depth in metres) of a float4 vertex map in metres"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 4)
    out, med = np.zeros((max(int(max_points), 1), 3), np.float32), C.c_float(0)
    h = load()
    h.hkf_reloc_points.restype = C.c_uint32
    n = h.hkf_reloc_points(K._p(v), C.c_uint32(len(v)), C.c_float(cell), C.c_uint32(int(max_points)), K._p(out), C.byref(med))
    return out[:n].copy(), med.value


def reloc_lattice(centre, n, trans_step, rot_step):
    """hkf_reloc_lattice: the candidate poses (K, 3, 4) around centre [R | t] (3, 4), or None when refused"""
    c = np.ascontiguousarray(centre, np.float64).reshape(12)
    nn = (C.c_int32 * 6)(*[int(x) for x in n])
    h = load()
    h.hkf_reloc_lattice.restype = C.c_int64
    k = h.hkf_reloc_lattice(K._p(c), nn, C.c_double(trans_step), C.c_double(rot_step), None, C.c_int64(0))
    if k < 0:
        return None
    out = np.zeros((k, 3, 4), np.float64)
    h.hkf_reloc_lattice(K._p(c), nn, C.c_double(trans_step), C.c_double(rot_step), K._p(out), C.c_int64(k))
    return out


def reloc_rank(scores, min_obs, m):
    """hkf_reloc_rank: (the best min(m, eligible) indices, how many poses were eligible) of a K.POSE_SCORE_DTYPE array"""
    sc = np.ascontiguousarray(scores, K.POSE_SCORE_DTYPE)
    best = np.zeros(max(int(m), 1), np.uint32)
    h = load()
    h.hkf_reloc_rank.restype = C.c_uint32
    e = h.hkf_reloc_rank(K._p(sc), C.c_uint32(len(sc)), C.c_uint32(int(min_obs)), C.c_uint32(int(m)), K._p(best))
    return best[:min(int(m), e)].copy(), int(e)


def load_slabs():
    global _s
    if _s is None:
        load()
        if not os.path.exists(SLABS_LIB):
            raise RuntimeError("libhybkf_slabs.so is missing: run __graft_entry__.build()")
        _s = C.CDLL(SLABS_LIB)
        _s.hkf_slabs_group.restype = C.c_void_p
    return _s


class SlabsApp:
    """HybKinectfuSlabs through hkf_slabs_*: the application over a slab group (one per process).  backend / cuts: hybkf_group.h"""

    def __init__(self, res, size, cam, cuts, backend=0, max_triangles=0, sdf_trunc=0.0, integrate_dist=0.0, trunc_max=0.0, device=0, halo=0,
                 traj_write=""):
        """traj_write: record the tracked poses there (TrajectoryRecorder), in world coordinates"""
        self.h = load_slabs()
        self.h.hkf_slabs_configure_traj(traj_write.encode())
        cuts_a = (C.c_uint32 * len(cuts))(*cuts)
        st = self.h.hkf_slabs_init(res, C.c_float(size), cam[0], cam[1], C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                   max_triangles, C.c_float(sdf_trunc), C.c_float(integrate_dist), C.c_float(trunc_max), device, backend,
                                   len(cuts) - 1, cuts_a, None, halo)
        if st:
            raise K.KfError("hkf_slabs_init failed: %d" % st)
        self.cam = cam

    def process_frame(self, mm, frame_id, stamp=0.0):
        mm = np.ascontiguousarray(mm, np.uint16)
        r = self.h.hkf_slabs_process_frame_stamped(mm.ctypes.data_as(C.c_void_p), 0, frame_id, C.c_double(stamp))
        if r < 0:
            raise K.KfError("processNewFrame failed: %d" % r)
        return bool(r)

    def shift_volume(self, dx, dy, dz):
        """HybKinectfuSlabs::shiftVolume: the group's window moves by (dx, dy, dz) voxels (multiples of 8), then the merged raycast; False: refused"""
        r = self.h.hkf_slabs_shift_volume(int(dx), int(dy), int(dz))
        if r < 0:
            raise K.KfError("hkf_slabs_shift_volume: no group")
        return bool(r)

    def volume_origin(self):
        """HybKinectfuSlabs::volumeOrigin: the sum of all shifts, in voxels"""
        o = (C.c_int * 3)()
        if self.h.hkf_slabs_volume_origin(o) != 0:
            raise K.KfError("hkf_slabs_volume_origin: no group")
        return tuple(int(x) for x in o)

    def set_recentre(self, dist):
        """AppParams::_volume_params.fRecentreDist for the slab class, as App.set_recentre (0: off, the default)"""
        if self.h.hkf_slabs_set_recentre(C.c_float(dist)) != 0:
            raise K.KfError("hkf_slabs_set_recentre: no group")

    def generate_mesh(self):
        return self.h.hkf_slabs_generate_mesh()

    def save_mesh(self, filename):
        nv, nf = C.c_uint32(), C.c_uint32()
        ok = self.h.hkf_slabs_save_mesh(filename.encode(), C.byref(nv), C.byref(nf))
        return bool(ok), nv.value, nf.value

    def pose(self):
        out = np.zeros(16, np.float32)
        tracked = self.h.hkf_slabs_get_pose(out.ctypes.data_as(C.c_void_p))
        return bool(tracked), out.reshape(4, 4)

    def group_handle(self):
        return C.c_void_p(self.h.hkf_slabs_group())

    def render_view(self, mode, pose, cam):
        """HybKinectfuSlabs::renderView: App.render_view over the group -- the whole volume's picture from any camera"""
        out = np.empty((cam[1], cam[0], 4), np.uint8)
        p = np.ascontiguousarray(pose, np.float32).reshape(16) if pose is not None else None
        r = self.h.hkf_slabs_render_view(int(mode), p.ctypes.data_as(C.c_void_p) if p is not None else None, int(cam[0]), int(cam[1]),
                                         C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                         out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
        if r != 0:
            raise K.KfError("renderView failed: %d (%d)" % (r, self.h.hkf_slabs_last_error()))
        return out

    def view_model_maps(self, mode):
        out = np.empty((self.cam[1], self.cam[0], 4), np.uint8)
        r = self.h.hkf_slabs_view_model_maps(int(mode), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
        if r != 0:
            raise K.KfError("viewModelMaps failed: %d" % r)
        return out

    def save_map(self, path):
        """HybKinectfuSlabs::saveMap: always False -- the map file is built on the brick store, which a slab group does not have"""
        return self.h.hkf_slabs_save_map(os.fsencode(path)) > 0

    def load_map(self, path):
        """HybKinectfuSlabs::loadMap: always False, nothing touched"""
        return self.h.hkf_slabs_load_map(os.fsencode(path)) > 0

    def load_map_coarser(self, path):
        """always False, nothing touched, as load_map"""
        return self.h.hkf_slabs_load_map_coarser(os.fsencode(path)) > 0

    def merge_map(self, path, offset=(0, 0, 0)):
        """always False, nothing touched: merging maps is built on the brick store, which a slab group does not have"""
        return self.h.hkf_slabs_merge_map(os.fsencode(path), int(offset[0]), int(offset[1]), int(offset[2])) > 0

    def merge_map_rigid(self, path, mat):
        """always False, nothing touched, as merge_map"""
        m = np.ascontiguousarray(mat, np.float32).reshape(16)
        return self.h.hkf_slabs_merge_map_rigid(os.fsencode(path), m.ctypes.data_as(C.c_void_p)) > 0

    def align_map(self, path, guess):
        """always (False, the guess, None), nothing touched, as merge_map"""
        g = np.ascontiguousarray(guess, np.float32).reshape(16)
        found = g.copy()
        self.h.hkf_slabs_align_map(os.fsencode(path), g.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p), None)
        return False, found.reshape(4, 4), None

    def erase_map_box(self, lo, hi, keep_inside=False):
        """always False, nothing touched: erasing from the map is built on the brick store, which a slab group does not have"""
        l, h = (C.c_float * 3)(*[float(x) for x in lo]), (C.c_float * 3)(*[float(x) for x in hi])
        return self.h.hkf_slabs_erase_map_box(l, h, int(bool(keep_inside)), None) > 0

    def erase_map_weak(self, min_weight):
        """always False, nothing touched, as erase_map_box"""
        return self.h.hkf_slabs_erase_map_weak(C.c_float(min_weight), None) > 0

    def sample_map(self, points):
        """always refused (K.KfError), nothing read: the map queries read window and brick store, which a slab group does not have"""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        r = self.h.hkf_slabs_sample_map(K._p(pts), C.c_uint32(len(pts)), None, None, None, None)
        raise K.KfError("hkf_slabs_sample_map: slab groups have no map queries (%d)" % r)

    def relocalise(self, mm, frame_id, params=None):
        """always refused (K.KfError), nothing touched: relocalisation reads window and brick store, which a slab group does not have"""
        r = self.h.hkf_slabs_relocalise(None, C.c_uint(int(frame_id)), None, None)
        raise K.KfError("hkf_slabs_relocalise: slab groups cannot relocalise (%d)" % r)

    def cast_map_rays(self, origins, dirs, t_min, t_max):
        """always refused (K.KfError), as sample_map"""
        org = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        r = self.h.hkf_slabs_cast_map_rays(K._p(org), None, None, None, C.c_uint32(len(org)), None, None, None, None, None)
        raise K.KfError("hkf_slabs_cast_map_rays: slab groups have no map queries (%d)" % r)

    def distance_field(self, lo_m, hi_m, max_dist_m, level=0.0, site_mask=1 << K.VOX_OCCUPIED):
        """always refused (K.KfError), as sample_map"""
        l, h = (C.c_float * 3)(*[float(x) for x in lo_m]), (C.c_float * 3)(*[float(x) for x in hi_m])
        r = self.h.hkf_slabs_distance_field(l, h, C.c_float(max_dist_m), C.c_float(level), C.c_uint32(site_mask), C.c_uint64(0), None, None, None, None, None)
        raise K.KfError("hkf_slabs_distance_field: slab groups have no map queries (%d)" % r)

    def close(self):
        self.h.hkf_slabs_shutdown()
        self.h.hkf_slabs_configure_traj(b"")


# ---- GPU-free helpers of the dataset / trajectory code -------------------------------------------------------------------------
def dataset_read(directory, cols, rows, n, with_color=False):
    h = load()
    depth = np.zeros((n, rows, cols), np.uint16)
    bgr = np.zeros((n, rows, cols, 3), np.uint8) if with_color else None
    ds, cs = np.zeros(n, np.float64), np.zeros(n, np.float64)
    got = h.hkf_dataset_read(directory.encode(), cols, rows, int(with_color), n, depth.ctypes.data_as(C.c_void_p),
                             bgr.ctypes.data_as(C.c_void_p) if with_color else None, ds.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(C.c_void_p))
    if got < 0:
        raise K.KfError("hkf_dataset_read failed: %d" % got)
    return depth[:got], (bgr[:got] if with_color else None), ds[:got], cs[:got]


def png_read(path):
    h = load()
    h.hkf_png_read.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    w, hh, ch, bits = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    if not h.hkf_png_read(path.encode(), C.byref(w), C.byref(hh), C.byref(ch), C.byref(bits), None, 0):
        return None
    out = np.zeros((hh.value, w.value, ch.value), np.uint16 if bits.value == 16 else np.uint8)
    h.hkf_png_read(path.encode(), C.byref(w), C.byref(hh), C.byref(ch), C.byref(bits), out.ctypes.data_as(C.c_void_p), out.nbytes)
    return out


def pyrdown16(img):
    h = load()
    img = np.ascontiguousarray(img, np.uint16)
    out = np.zeros(((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2), np.uint16)
    h.hkf_pyrdown16(img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], out.ctypes.data_as(C.c_void_p))
    return out


def quat_from_pose(pose):
    h = load()
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    q = np.zeros(4, np.float32)
    h.hkf_quat_from_pose(p.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p))
    return q


def pose_from_quat(t, q_xyzw):
    h = load()
    t = np.ascontiguousarray(t, np.float32); q = np.ascontiguousarray(q_xyzw, np.float32)
    out = np.zeros(16, np.float32)
    h.hkf_pose_from_quat(t.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.reshape(4, 4)


def trajectory_write(path, poses, stamps):
    h = load()
    p = np.ascontiguousarray(poses, np.float32).reshape(-1, 16); s = np.ascontiguousarray(stamps, np.float64)
    return h.hkf_trajectory_write(path.encode(), p.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), len(s))


def table_nearest(path, header_lines, targets):
    h = load()
    t = np.ascontiguousarray(targets, np.float64); out = np.zeros(len(t), np.float64)
    n = h.hkf_table_nearest(path.encode(), header_lines, t.ctypes.data_as(C.c_void_p), len(t), out.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise K.KfError("cannot read " + path)
    return out


# ---- mesh post-processing (MeshGeneratorMarchingcube::saveMesh's weld / dedupe / normals / writers) ------------------------------
def _mesh_read(which):
    h = load()
    nv, nf, nc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if h.hkf_mesh_sizes(which, C.byref(nv), C.byref(nf), C.byref(nc)) != 0:
        raise K.KfError("no mesh")
    v = np.empty((nv.value, 3), np.float32)
    n = np.empty((nv.value, 3), np.float32)
    c = np.empty((nc.value, 4), np.float32)
    f = np.empty((nf.value, 3), np.uint32)
    h.hkf_mesh_read(which, v.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p) if nc.value else None,
                    f.ctypes.data_as(C.c_void_p))
    return dict(vertices=v, normals=n, colors=c, faces=f)


def mesh_from_soup(triangles, with_color=False):
    """GPU-free: weld / dedupe / normals of a triangle soup (numpy array of lib.TRI_DTYPE), as saveMesh does after the copy."""
    h = load()
    tris = np.ascontiguousarray(triangles)
    assert tris.dtype.itemsize == 72
    h.hkf_mesh_from_soup(tris.ctypes.data_as(C.c_void_p), len(tris), int(with_color), None, None)
    return _mesh_read(0)


def mesh_save(which, filename):
    """which: 0 = the mesh of mesh_from_soup, 1 = the application's mesh (after App.save_mesh)"""
    return bool(load().hkf_mesh_save(which, filename.encode()))


def mesh_parts(which):
    """GPU-free: per vertex of the mesh `which` (label = smallest vertex index of its part, faces of its part), two (n_v,) u32 arrays"""
    h = load()
    nv, nf, nc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if h.hkf_mesh_sizes(which, C.byref(nv), C.byref(nf), C.byref(nc)) != 0:
        raise K.KfError("no mesh")
    lab, cnt = np.empty(nv.value, np.uint32), np.empty(nv.value, np.uint32)
    h.hkf_mesh_parts(which, lab.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
    return lab, cnt


def mesh_drop_parts(which, min_faces=0, largest_only=False):
    """GPU-free: drops the small parts of the mesh `which` on one host thread (the rule of kf_mesh_drop_parts) and returns the cleaned mesh"""
    if load().hkf_mesh_drop_parts(which, C.c_uint32(int(min_faces)), int(bool(largest_only))) != 0:
        raise K.KfError("no mesh")
    return _mesh_read(which)


def app_mesh():
    return _mesh_read(1)


def departing_boxes(d, res):
    """hkf_departing_boxes: the disjoint cell boxes [(lo, hi), ...] (x, y, z; half-open) that a shift by d voxels makes unextractable, in the order
    the stream-out emits them; GPU-free"""
    h = load()
    dd = (C.c_int32 * 3)(*[int(x) for x in d])
    lo, hi = ((C.c_int32 * 3) * 3)(), ((C.c_int32 * 3) * 3)()
    h.hkf_departing_boxes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    n = h.hkf_departing_boxes(dd, C.c_uint32(res), lo, hi)
    return [(tuple(int(x) for x in lo[b]), tuple(int(x) for x in hi[b])) for b in range(n)]


def recentre_shift(pose, size, res, dist):
    """hkf_recentre_shift: the shift (voxels, multiples of 8) HybKinectfu::processNewFrame applies for `pose` with fRecentreDist = dist; GPU-free"""
    h = load()
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    out = (C.c_int32 * 3)()
    h.hkf_recentre_shift(p.ctypes.data_as(C.c_void_p), C.c_float(size), C.c_uint32(res), C.c_float(dist), out)
    return tuple(int(x) for x in out)


def view_frame(world_pose, size, res):
    """hkf_view_frame: (frame, local_pose) -- the frame (voxels, multiples of 8) whose window is centred on the focus of a view from `world_pose`
    (first-cube coordinates), and the pose in that frame's coordinates: what App.render_map_view hands render_view_at; GPU-free"""
    h = load()
    p = np.ascontiguousarray(world_pose, np.float32).reshape(16)
    f = (C.c_int32 * 3)()
    out = np.zeros(16, np.float32)
    h.hkf_view_frame(p.ctypes.data_as(C.c_void_p), C.c_float(size), C.c_uint32(res), f, out.ctypes.data_as(C.c_void_p))
    return tuple(int(x) for x in f), out.reshape(4, 4)
