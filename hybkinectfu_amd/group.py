"""ctypes binding of include/hybkf_group.h (libhybkf_group.so): slab groups -- N z-slab contexts whose per-frame merge runs natively, over
RCCL (one member per device, one or many processes) or on one device (the LOCAL backend's reduction kernels).

Group.local / rccl_all / rccl_rank build one; frame() enqueues a frame on every member; members() are non-owning lib.Context views for
read-backs.  Live groups are kept in a registry (live_groups): a leaked member context would switch the persistent tracking loops off for
everything that runs after it in the process, so harnesses close what a failed test left open.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import lib as K
from . import scene as S

LIB_PATH = os.path.join(K.PKG_DIR, "libhybkf_group.so")

LOCAL, RCCL_ALL, RCCL_RANK = 0, 1, 2
MAX_MEMBERS, UNIQUE_ID_BYTES = 16, 128
ERR_ARG, ERR_STATE, ERR_ALLOC, ERR_RCCL = 1001, 1002, 1003, 1004

# every function include/hybkf_group.h declares
SYMBOLS = [
    "kf_group_error_string", "kf_group_unique_id", "kf_group_validate", "kf_group_create", "kf_group_destroy", "kf_group_members", "kf_group_set_pose",
    "kf_group_frame", "kf_group_frame_members", "kf_group_track_result", "kf_group_member", "kf_group_marching_cubes",
    "kf_group_triangle_count", "kf_group_read_triangles", "kf_group_merge_timing", "kf_group_read_merge_ms", "kf_group_synchronize",
    "kf_group_stream",
    "kf_group_create_color", "kf_group_validate_color", "kf_group_frame_color", "kf_group_frame_members_color",
    "kf_group_view_validate", "kf_group_render_view", "kf_group_view_size", "kf_group_view_device", "kf_group_read_view",
    "kf_group_shift_plan", "kf_group_shift_volume", "kf_group_raycast", "kf_group_volume_origin",
]


class Transfer(C.Structure):
    _fields_ = [("from_member", C.c_uint32), ("to_member", C.c_uint32), ("bz_begin", C.c_uint32), ("bz_end", C.c_uint32)]


class GroupParams(C.Structure):
    _fields_ = [("trunc_min", C.c_float), ("trunc_max", C.c_float), ("sigma_pixel", C.c_float), ("sigma_depth", C.c_float),
                ("icp", K.IcpParams), ("integrate", K.IntegrateParams), ("raycast", K.RaycastParams)]


_lib = None


def load():
    """dlopen libhybkf_group.so (after libhybkf.so, which it links); raises if it has not been built"""
    global _lib
    if _lib is None:
        K.load()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libhybkf_group.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = C.CDLL(LIB_PATH)
        _lib.kf_group_error_string.restype = C.c_char_p
        _lib.kf_group_stream.restype = C.c_void_p
        _lib.kf_group_view_device.restype = C.c_void_p
        _lib.kf_group_shift_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int32, C.POINTER(Transfer), C.c_uint32]
        _lib.kf_group_shift_volume.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        _lib.kf_group_volume_origin.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    return _lib


class GroupError(RuntimeError):
    def __init__(self, what, status):
        super().__init__("%s failed: %d (%s)" % (what, status, load().kf_group_error_string(status).decode()))
        self.status = status


def _chk(st, what):
    if st != 0:
        raise GroupError(what, st)


def stock_params(trunc_max=None, integ_dist=None, levels=3):
    """the parameters SlabPipeline runs with (scene.STOCK, its workload's trunc_max / integ_dist)"""
    P = S.STOCK
    return GroupParams(P["depth_trunc_min"], P["depth_trunc_max"] if trunc_max is None else trunc_max, P["filter_sigma_pixel"], P["filter_sigma_depth"],
                       K.IcpParams(levels, P["icp_thre_sin_angle"], P["icp_thre_dist"], P["camera_shake_dist"], P["camera_shake_angle"]),
                       K.IntegrateParams(P["integrate_sdf_trunc"], P["integrate_depth_trunc"] if integ_dist is None else integ_dist),
                       K.RaycastParams(P["raycast_increment_factor"] * P["integrate_sdf_trunc"]))


def base_config(kcam, res, size, max_weight=None, levels=3, max_triangles=0, device=0, has_color=False):
    return K.Config(kcam, kcam, K.VolumeParams(int(res), float(size), S.STOCK["volume_max_weight"] if max_weight is None else max_weight),
                    levels, max_triangles, int(has_color), device, 0, 0, 0)


def unique_id():
    """ncclGetUniqueId as bytes: made on one rank, handed to every rank (Group.rccl_rank)"""
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    _chk(load().kf_group_unique_id(buf), "kf_group_unique_id")
    return bytes(buf)


def _args(cuts, devices, uid):
    cuts_a = (C.c_uint32 * len(cuts))(*cuts)
    devs_a = (C.c_int32 * max(1, len(devices)))(*devices) if devices is not None else None
    uid_a = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(uid) if uid is not None else None
    return cuts_a, devs_a, uid_a


def validate_status(cfg, params, backend, cuts, devices=None, halo=0, uid=None, rank=0, world=1):
    """kf_group_validate: the argument checks of kf_group_create alone (no HIP or RCCL call; a valid layout returns 0)"""
    cuts_a, devs_a, uid_a = _args(cuts, devices, uid)
    return load().kf_group_validate(C.byref(cfg) if cfg is not None else None, C.byref(params) if params is not None else None, backend,
                                    len(cuts) - 1, cuts_a, devs_a, halo, uid_a, rank, world)


def validate_color_status(cfg, params, backend, cuts, devices=None, halo=0, uid=None, rank=0, world=1, angle_weight=True):
    """kf_group_validate_color: the argument checks of kf_group_create_color alone"""
    cuts_a, devs_a, uid_a = _args(cuts, devices, uid)
    return load().kf_group_validate_color(C.byref(cfg) if cfg is not None else None, C.byref(params) if params is not None else None, int(angle_weight),
                                          backend, len(cuts) - 1, cuts_a, devs_a, halo, uid_a, rank, world)


def view_validate_status(color_group, mode, cam):
    """kf_group_view_validate: the refusals of kf_group_render_view alone (no HIP call); cam: lib.camera or None"""
    return load().kf_group_view_validate(int(bool(color_group)), int(mode), C.byref(cam) if cam is not None else None)


def shift_plan(res, cuts, halo, dz):
    """kf_group_shift_plan: the transfers (from_member, to_member, bz_begin, bz_end) of a z shift by dz voxels, ordered by receiver, then by layer;
    None for arguments the library refuses.  Host only"""
    lib = load()
    cuts_a = (C.c_uint32 * len(cuts))(*cuts)
    n = lib.kf_group_shift_plan(int(res), len(cuts) - 1, cuts_a, int(halo), int(dz), None, 0)
    if n < 0:
        return None
    out = (Transfer * max(n, 1))()
    assert lib.kf_group_shift_plan(int(res), len(cuts) - 1, cuts_a, int(halo), int(dz), out, n) == n
    return [(t.from_member, t.to_member, t.bz_begin, t.bz_end) for t in out[:n]]


def create_status(cfg, params, backend, cuts, devices=None, halo=0, uid=None, rank=0, world=1):
    """kf_group_create's status alone (the group, if made, is destroyed at once): the validation tests"""
    lib = load()
    cuts_a, devs_a, uid_a = _args(cuts, devices, uid)
    h = C.c_void_p()
    st = lib.kf_group_create(C.byref(cfg) if cfg is not None else None, C.byref(params) if params is not None else None, backend, len(cuts) - 1,
                             cuts_a, devs_a, halo, uid_a, rank, world, C.byref(h))
    if st == 0 and h:
        lib.kf_group_destroy(h)
    return st


_LIVE = weakref.WeakSet()


def live_groups():
    return [g for g in list(_LIVE) if g.h]


class Group:
    """One kf_group.  Use the constructors local / rccl_all / rccl_rank."""

    def __init__(self, kcam, res, size, backend, cuts, devices=None, halo=0, params=None, max_weight=None, levels=3, max_triangles=0,
                 uid=None, rank=0, world=1, has_color=False, angle_weight=True):
        self.lib = load()
        self.cam, self.res, self.size, self.levels = kcam, int(res), float(size), int(levels)
        self.cuts = [int(z) for z in cuts]
        self.n = len(self.cuts) - 1
        self.params = params if params is not None else stock_params(levels=levels)
        device = devices[0] if devices else 0
        self.has_color, self.angle_weight = bool(has_color), bool(angle_weight)
        self.cfg = base_config(kcam, res, size, max_weight, levels, max_triangles, device, has_color=self.has_color)
        cuts_a = (C.c_uint32 * len(self.cuts))(*self.cuts)
        devs_a = (C.c_int32 * self.n)(*devices) if devices is not None else None
        uid_a = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(uid) if uid is not None else None
        self.h = C.c_void_p()
        if self.has_color:
            _chk(self.lib.kf_group_create_color(C.byref(self.cfg), C.byref(self.params), int(self.angle_weight), backend, self.n, cuts_a, devs_a, int(halo),
                                                uid_a, rank, world, C.byref(self.h)), "kf_group_create_color")
        else:
            _chk(self.lib.kf_group_create(C.byref(self.cfg), C.byref(self.params), backend, self.n, cuts_a, devs_a, int(halo), uid_a, rank, world,
                                          C.byref(self.h)), "kf_group_create")
        _LIVE.add(self)
        n, hl = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_group_members(self.h, C.byref(n), C.byref(hl)), "kf_group_members")
        self.halo = hl.value
        self._members = []
        for i in range(self.n):
            m = C.c_void_p()
            _chk(self.lib.kf_group_member(self.h, i, C.byref(m)), "kf_group_member")
            v = K.Context.borrow(m, kcam, res, size, levels)
            v.owned = (self.cuts[i], self.cuts[i + 1])
            self._members.append(v)

    @classmethod
    def borrow(cls, handle, kcam, res, size, levels=3):
        """Wrap a kf_group owned by someone else (HybKinectfuSlabs: hkf_slabs_group): same methods, close() leaves it alone"""
        self = cls.__new__(cls)
        self.lib = load()
        self.cam, self.res, self.size, self.levels = kcam, int(res), float(size), int(levels)
        self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self.borrowed = True
        n, hl = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_group_members(self.h, C.byref(n), C.byref(hl)), "kf_group_members")
        self.n, self.halo, self._members = n.value, hl.value, []
        for i in range(self.n):
            m = C.c_void_p()
            _chk(self.lib.kf_group_member(self.h, i, C.byref(m)), "kf_group_member")
            self._members.append(K.Context.borrow(m, kcam, res, size, levels))
        return self

    @classmethod
    def local(cls, kcam, res, size, cuts, device=0, **kw):
        """N members on one device; the two all-reduces are the group's reduction kernels"""
        return cls(kcam, res, size, LOCAL, cuts, devices=[device] * (len(cuts) - 1), **kw)

    @classmethod
    def rccl_all(cls, kcam, res, size, cuts, devices, **kw):
        """one member per device (distinct), one process: ncclCommInitAll"""
        return cls(kcam, res, size, RCCL_ALL, cuts, devices=list(devices), **kw)

    @classmethod
    def rccl_rank(cls, kcam, res, size, cuts, device, uid, rank, world, **kw):
        """this process's one member of a world-sized group (ncclCommInitRank); `cuts` = [z0, z1], THIS rank's own slab (rank r of a
        layout L of world + 1 cuts passes [L[r], L[r + 1]]; [0, res] at world 1)"""
        return cls(kcam, res, size, RCCL_RANK, cuts, devices=[device], uid=uid, rank=rank, world=world, **kw)

    def members(self):
        """non-owning lib.Context views (download_map / download_volume / stats ...); close() of a view leaves the member alone"""
        return list(self._members)

    def set_pose(self, pose):
        _chk(self.lib.kf_group_set_pose(self.h, C.byref(K.Mat44.of(pose))), "kf_group_set_pose")

    def frame(self, mm, frame_id, rgb=None):
        """mm: a host u16 image (numpy) or the device address (int) of one that every member can read; rgb (a colour group's frames): the
        BGR image, rows x cols x 3 bytes, where mm lies (numpy with numpy, device address with device address).  The kind of call follows
        `rgb`, so a colour group without one -- or a colourless group with one -- gets the library's ERR_STATE"""
        if rgb is not None:
            if isinstance(mm, np.ndarray):
                mm, rgb = np.ascontiguousarray(mm, np.uint16), np.ascontiguousarray(rgb, np.uint8)
                _chk(self.lib.kf_group_frame_color(self.h, mm.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), 0, self.cam.cols, self.cam.rows,
                                                   frame_id), "kf_group_frame_color")
            else:
                _chk(self.lib.kf_group_frame_color(self.h, C.c_void_p(int(mm)), C.c_void_p(int(rgb)), 1, self.cam.cols, self.cam.rows, frame_id),
                     "kf_group_frame_color")
        elif isinstance(mm, np.ndarray):
            mm = np.ascontiguousarray(mm, np.uint16)
            _chk(self.lib.kf_group_frame(self.h, mm.ctypes.data_as(C.c_void_p), 0, self.cam.cols, self.cam.rows, frame_id), "kf_group_frame")
        else:
            _chk(self.lib.kf_group_frame(self.h, C.c_void_p(int(mm)), 1, self.cam.cols, self.cam.rows, frame_id), "kf_group_frame")

    def frame_members(self, dev_ptrs, frame_id, rgb_ptrs=None):
        arr = (C.c_void_p * self.n)(*[int(p) for p in dev_ptrs])
        if rgb_ptrs is not None:
            rgb = (C.c_void_p * self.n)(*[int(p) for p in rgb_ptrs])
            _chk(self.lib.kf_group_frame_members_color(self.h, arr, rgb, self.cam.cols, self.cam.rows, frame_id), "kf_group_frame_members_color")
            return
        _chk(self.lib.kf_group_frame_members(self.h, arr, self.cam.cols, self.cam.rows, frame_id), "kf_group_frame_members")

    def track_result(self, check_lockstep=True):
        """(tracked, pose, status, iterations) of member 0; check_lockstep: every member agrees (else GroupError with ERR_STATE)"""
        r = K.TrackResult()
        _chk(self.lib.kf_group_track_result(self.h, C.byref(r), int(bool(check_lockstep))), "kf_group_track_result")
        return bool(r.tracked), r.pose.numpy(), r.status, r.iterations

    def marching_cubes(self, threshold):
        _chk(self.lib.kf_group_marching_cubes(self.h, C.c_float(threshold)), "kf_group_marching_cubes")

    def triangles(self):
        n = C.c_uint32()
        _chk(self.lib.kf_group_triangle_count(self.h, C.byref(n)), "kf_group_triangle_count")
        out = np.zeros(n.value, dtype=K.TRI_DTYPE)
        if n.value:
            _chk(self.lib.kf_group_read_triangles(self.h, out.ctypes.data_as(C.c_void_p), 0, n.value), "kf_group_read_triangles")
        return out

    # ---- the moving volume ----
    def shift_volume(self, dx, dy, dz):
        """the window moves by whole bricks on every member, brick layers travelling between members for a z shift; asynchronous.  The model maps
        are stale afterwards: raycast() before the next frame (kf_group_shift_volume)"""
        _chk(self.lib.kf_group_shift_volume(self.h, int(dx), int(dy), int(dz)), "kf_group_shift_volume")

    def raycast(self):
        """the merged raycast from the device-resident pose alone: steps 5-9 of a frame (kf_group_raycast)"""
        _chk(self.lib.kf_group_raycast(self.h), "kf_group_raycast")

    def volume_origin(self):
        """(x, y, z): the sum of all shifts, in voxels; the members agree (kf_group_volume_origin)"""
        o = (C.c_int32 * 3)()
        _chk(self.lib.kf_group_volume_origin(self.h, o), "kf_group_volume_origin")
        return tuple(o)

    # ---- merged views ----
    def render_view(self, mode, pose, cam, near, far, dev_v=None, dev_n=None):
        """the whole volume from `cam` (lib.camera, any size) and `pose` (None: the device-resident pose) into member 0's BGRA view image; the
        group's own increment; dev_v / dev_n: optional device addresses of float4 maps on member 0's device.  Asynchronous; a bystander to frames"""
        tp = C.byref(K.Mat44.of(pose)) if pose is not None else None
        _chk(self.lib.kf_group_render_view(self.h, int(mode), tp, C.byref(cam) if cam is not None else None, C.c_float(near), C.c_float(far),
                                           C.c_void_p(dev_v), C.c_void_p(dev_n)), "kf_group_render_view")

    def view_size(self):
        """(cols, rows) of the last view"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.lib.kf_group_view_size(self.h, C.byref(a), C.byref(b)), "kf_group_view_size")
        return a.value, b.value

    def view_device(self):
        """device address of the last view's image on member 0's device, valid in stream order; None before a view"""
        return self.lib.kf_group_view_device(self.h)

    def read_view(self):
        """the last view as a (rows, cols, 4) uint8 array (b, g, r, a); blocking"""
        cols, rows = self.view_size()
        out = np.empty((rows, cols, 4), np.uint8)
        _chk(self.lib.kf_group_read_view(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)), "kf_group_read_view")
        return out

    def merge_timing(self, on=True):
        _chk(self.lib.kf_group_merge_timing(self.h, int(bool(on))), "kf_group_merge_timing")

    def merge_ms(self):
        """(total ms, frames) of the merges timed since the last call"""
        ms, n = C.c_float(), C.c_uint32()
        _chk(self.lib.kf_group_read_merge_ms(self.h, C.byref(ms), C.byref(n)), "kf_group_read_merge_ms")
        return float(ms.value), int(n.value)

    def stream(self, i=0):
        return self.lib.kf_group_stream(self.h, i)

    def sync(self):
        _chk(self.lib.kf_group_synchronize(self.h), "kf_group_synchronize")

    def close(self):
        if self.h:
            for v in self._members:
                v.h = None
            if not getattr(self, "borrowed", False):
                self.lib.kf_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
