"""Pin the oracle's helper arithmetic against the REFERENCE's own __host__ __device__ headers.

oracle/_ref/libkfref.so is built (oracle/Makefile) from the reference's src/cuda/{tsdfVolume,Mat,DepthCamera,cuda_declar}.h as they
lie, where those sources are present.  Everything here is bit-exact.  Each test splits into its inputs (seeded), what the reference
computes from them (REF_CASES: a function of the live harness) and the comparison with the oracle.  Where the harness is built the
reference side runs live and must equal the stored copy in tests/golden/ref_helpers.npz (tools/make_ref_golden.py writes it); where it
is not, the stored copy stands in for it.
"""
import ctypes as C
import os

import numpy as np

import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_helpers.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rand_pose(rng, scale=1.0):
    a = rng.normal(size=3) * 0.3
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = rng.normal(size=3) * scale
    return m.astype(np.float32)


def reference_side(name, *inputs):
    """What the reference computes for test `name` from `inputs`: live through oracle/_ref/libkfref.so where it is built (and then
    checked bit for bit against the stored copy), else the stored copy.  A dict of arrays."""
    if O.have_ref():
        live = {k: np.asarray(v) for k, v in REF_CASES[name](O.ref(), *inputs).items()}
        if not os.environ.get("KF_REF_REGEN"):                  # (tools/make_ref_golden.py sets it while it writes the copy)
            stored = stored_side(name)
            assert sorted(stored) == sorted(live), name
            for k, v in live.items():
                assert v.dtype == stored[k].dtype and v.shape == stored[k].shape and v.tobytes() == stored[k].tobytes(), (name, k)
        return live
    return stored_side(name)


def stored_side(name):
    g = np.load(GOLD)
    pre = name + "/"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


# ---- the reference side of every test: (harness, inputs...) -> arrays ----

def _ref_struct_sizes(r):
    return dict(sizes=np.array([r.ref_sizeof_voxel(), r.ref_sizeof_camera_params()], np.int64))


def _ref_mat44(r, pairs):
    inv = np.zeros((len(pairs), 16), np.float32)
    mul = np.zeros((len(pairs), 16), np.float32)
    for i, (a, b) in enumerate(pairs):
        r.ref_mat44_inverse(O.fp(O.m16(a)), O.fp(inv[i]))
        r.ref_mat44_mul(O.fp(O.m16(a)), O.fp(O.m16(b)), O.fp(mul[i]))
    return dict(inverse=inv, mul=mul)


def _ref_volume(r, vol):
    res = vol.res
    h = C.c_void_p(r.ref_vol_create(res, C.c_float(vol.size), C.c_float(128.0)))
    for z in range(res):
        for y in range(res):
            for x in range(res):
                q = vol.vox[(z * res + y) * res + x]
                col = (C.c_ubyte * 3)(*[int(c) for c in q["color"]])
                r.ref_vol_set(h, x, y, z, C.c_float(q["tsdf"]), C.c_float(q["weight"]), col)
    return h


def _ref_interpolation(r, vol, pts):
    h = _ref_volume(r, vol)
    ok = np.zeros(len(pts), bool)
    d = np.zeros(len(pts), np.float32)
    tw = np.zeros((len(pts), 2), np.float32)
    for i, p in enumerate(pts):
        d_ref = C.c_float(0)
        ok[i] = bool(r.ref_vol_interp_sdf(h, O.fp(p), C.byref(d_ref)))
        d[i] = d_ref.value
        t, w = C.c_float(0), C.c_float(0)
        r.ref_vol_nearest(h, O.fp(p), C.byref(t), C.byref(w))
        tw[i] = t.value, w.value
    r.ref_vol_destroy(h)
    return dict(ok=ok, sdf=d, nearest=tw)


def _ref_running_average(r, trials):
    """every update of every trial: (tsdf, weight, r, g, b) of the voxel before and after ref_vol_update"""
    h = C.c_void_p(r.ref_vol_create(4, C.c_float(1.0), C.c_float(8.0)))
    col = (C.c_ubyte * 3)(10, 200, 31)
    before, after = [], []
    for (x, y, z), seq in trials:
        for tsdf in seq:
            t, w, c = C.c_float(0), C.c_float(0), (C.c_ubyte * 3)()
            r.ref_vol_get(h, x, y, z, C.byref(t), C.byref(w), c)
            before.append([t.value, w.value] + list(c))
            r.ref_vol_update(h, x, y, z, C.c_float(tsdf), C.c_float(1.0), col, C.c_float(2.0))
            r.ref_vol_get(h, x, y, z, C.byref(t), C.byref(w), c)
            after.append([t.value, w.value] + list(c))
    r.ref_vol_destroy(h)
    return dict(before=np.array(before, np.float32), after=np.array(after, np.float32))


def _ref_integrate(r, res, size, cam, depth, pose, reps):
    """the reference's voxelPosToWorld / Mat44 / projectSkeletonToScreen / updateVoxel over every voxel, `reps` times: the voxels each pass
    updated and the volume after the last"""
    h = C.c_void_p(r.ref_vol_create(res, C.c_float(size), C.c_float(128.0)))
    col = (C.c_ubyte * 3)(0, 0, 0)
    tinv = np.zeros(16, np.float32)
    r.ref_mat44_inverse(O.fp(O.m16(pose)), O.fp(tinv))
    rows, cols = depth.shape
    n_ref = []
    for rep in range(reps):
        n = 0
        for z in range(res):
            for y in range(res):
                for x in range(res):
                    w = np.zeros(4, np.float32)
                    r.ref_vol_voxel_to_world(h, x, y, z, O.fp(w))
                    w[3] = 1.0
                    pf = np.zeros(4, np.float32)
                    r.ref_mat44_vec(O.fp(tinv), O.fp(w), O.fp(pf))
                    if pf[2] <= 0:
                        continue
                    sp = np.zeros(2, np.int32)
                    r.ref_project_to_screen(O.fp(pf), C.byref(cam), O.fp(sp))
                    if sp[0] >= cols - 1 or sp[1] >= rows - 1 or sp[0] < 1 or sp[1] < 1:
                        continue
                    d = depth[sp[1], sp[0]]
                    if d == 0 or not d < np.float32(2.0):
                        continue
                    sdf = np.float32(d - pf[2])
                    if sdf > np.float32(-0.05):
                        tsdf = min(np.float32(1.0), np.float32(sdf / np.float32(0.05)))
                        r.ref_vol_update(h, x, y, z, C.c_float(tsdf), C.c_float(1.0), col, C.c_float(2.0))
                        n += 1
        n_ref.append(n)
    tsdf_v, weight_v = np.zeros((res, res, res), np.float32), np.zeros((res, res, res), np.float32)
    t, w, c = C.c_float(0), C.c_float(0), (C.c_ubyte * 3)()
    for z in range(res):
        for y in range(res):
            for x in range(res):
                r.ref_vol_get(h, x, y, z, C.byref(t), C.byref(w), c)
                tsdf_v[z, y, x], weight_v[z, y, x] = t.value, w.value
    r.ref_vol_destroy(h)
    return dict(n_updated=np.array(n_ref, np.int64), tsdf=tsdf_v, weight=weight_v)


def _ref_vector_helpers(r, cam, samples):
    """samples: (x, y, depth, up, right) -> depthToSkeleton of the pixel and normalize(cross(up, right))"""
    skel = np.zeros((len(samples), 3), np.float32)
    nrm = np.zeros((len(samples), 3), np.float32)
    for i, (x, y, d, up, rt) in enumerate(samples):
        r.ref_depth_to_skeleton(x, y, C.c_float(d), C.byref(cam), O.fp(skel[i]))
        cr = np.zeros(3, np.float32)
        r.ref_cross(O.fp(up), O.fp(rt), O.fp(cr))
        r.ref_normalize(O.fp(cr), O.fp(nrm[i]))
    return dict(skeleton=skel, normal=nrm)


def _ref_color_world_norm(r, vol, pts, vecs):
    h = _ref_volume(r, vol)
    ok = np.zeros(len(pts), bool)
    col = np.zeros((len(pts), 3), np.uint8)
    grid = np.zeros((len(pts), 3), np.int32)
    nrm = np.zeros(len(pts), np.float32)
    for i, (p, v) in enumerate(zip(pts, vecs)):
        c_ref = (C.c_ubyte * 3)(0, 0, 0)
        ok[i] = bool(r.ref_vol_interp_color(h, O.fp(p), c_ref))
        col[i] = list(c_ref)
        r.ref_vol_world_to_voxel(h, O.fp(p), O.fp(grid[i]))
        nrm[i] = r.ref_norm(O.fp(v))
    r.ref_vol_destroy(h)
    return dict(ok=ok, color=col, voxel=grid, norm=nrm)


def _ref_mc_tables(r):
    edge = np.zeros(256, np.int32)
    tri = np.zeros(256 * 16, np.int32)
    r.ref_mc_tables(O.fp(edge), O.fp(tri))
    return dict(edge=edge, tri=tri.reshape(256, 16))


REF_CASES = dict(struct_sizes=_ref_struct_sizes, mat44=_ref_mat44, interpolation=_ref_interpolation, running_average=_ref_running_average,
                 integrate=_ref_integrate, vector_helpers=_ref_vector_helpers, color_world_norm=_ref_color_world_norm, mc_tables=_ref_mc_tables)


# ---- the seeded inputs of every test (tools/make_ref_golden.py runs the reference side on exactly these) ----

def inputs_struct_sizes():
    return ()


def inputs_mat44():
    rng = np.random.default_rng(1)
    return ([(rand_pose(rng, 2.0), rand_pose(rng, 2.0)) for _ in range(200)],)


def _vol(rng, res=16, size=1.5, fill=0.8):
    vol = O.OVolume(res, size, 128.0)
    n = res ** 3
    vol.vox["tsdf"] = rng.uniform(-1, 1, n).astype(np.float32)
    vol.vox["weight"] = np.where(rng.uniform(size=n) < fill, rng.integers(1, 128, n), 0).astype(np.float32)
    vol.vox["color"] = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return vol


def inputs_interpolation():
    rng = np.random.default_rng(2)
    vol = _vol(rng, fill=0.97)
    return vol, [rng.uniform(-0.1, vol.size + 0.1, 3).astype(np.float32) for _ in range(4000)]


def inputs_running_average():
    rng = np.random.default_rng(3)
    trials = []
    for _ in range(50):
        xyz = tuple(int(v) for v in rng.integers(0, 4, 3))
        trials.append((xyz, [np.float32(rng.uniform(-1, 1)) for _ in range(12)]))
    return (trials,)


def inputs_integrate():
    rng = np.random.default_rng(4)
    cam = O.Cam.make(64, 48, 31.5, 23.5, 52.5, 52.5)
    depth = rng.uniform(0.35, 1.6, (48, 64)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.1] = 0
    pose = rand_pose(rng, 0.0)
    pose[:3, 3] = [0.6, 0.55, -0.3]
    return 24, 1.2, cam, depth, pose, 2


def inputs_vector_helpers():
    rng = np.random.default_rng(5)
    cam = O.Cam.make(640, 480, 319.5, 239.5, 525.0, 525.0)
    d = np.ones((480, 640), np.float32)
    d[:] = rng.uniform(0.4, 3.0, d.shape)
    v = O.depth_to_vertices(d, cam)
    samples = []
    for _ in range(300):
        x, y = int(rng.integers(1, 639)), int(rng.integers(1, 479))
        up = (v[y + 1, x, :3] - v[y - 1, x, :3]).astype(np.float32)
        rt = (v[y, x + 1, :3] - v[y, x - 1, :3]).astype(np.float32)
        samples.append((x, y, d[y, x], up, rt))
    return cam, samples


def inputs_color_world_norm():
    rng = np.random.default_rng(9)
    vol = _vol(rng, fill=0.97)
    pts, vecs = [], []
    for _ in range(4000):
        pts.append(rng.uniform(-0.1, vol.size + 0.1, 3).astype(np.float32))
        vecs.append((rng.standard_normal(3) * rng.choice([1e-6, 1.0, 1e4])).astype(np.float32))
    return vol, pts, vecs


def inputs_mc_tables():
    return ()


# ---- the tests: the oracle against the reference side ----

def test_struct_sizes():
    ref = reference_side("struct_sizes")
    assert ref["sizes"][0] == 12 == O.VOXEL_DTYPE.itemsize
    assert ref["sizes"][1] == 24 == C.sizeof(O.Cam)


def test_mat44_inverse_mul_vec():
    pairs, = inputs_mat44()
    ref = reference_side("mat44", pairs)
    for i, (a, b) in enumerate(pairs):
        assert np.array_equal(bits(ref["inverse"][i]), bits(O.mat44_inverse(a).reshape(16)))
        assert np.array_equal(bits(ref["mul"][i]), bits(O.mat44_mul(a, b).reshape(16)))


def test_voxel_world_maps_and_interpolation():
    vol, pts = inputs_interpolation()
    ref = reference_side("interpolation", vol, pts)
    res, size = vol.res, vol.size
    n_ok = 0
    for i, p in enumerate(pts):
        ok, d = O.interpolate_sdf(vol, p)
        assert bool(ref["ok"][i]) == ok
        if ok:
            n_ok += 1
            assert ref["sdf"][i].view(np.uint32) == np.float32(d).view(np.uint32)
        g = np.clip((p * np.float32(res) / np.float32(size)).astype(np.int32), 0, res - 1)
        assert ref["nearest"][i, 0] == vol.tsdf[g[2], g[1], g[0]] and ref["nearest"][i, 1] == vol.weight[g[2], g[1], g[0]]
    assert n_ok > 500


def test_update_voxel_running_average():
    """tsdfVolume.h:57-75 through okf_integrate: one depth pixel per voxel column is hard to arrange, so
    drive both sides with the same per-voxel sequence via a 1-voxel-deep synthetic integrate instead:
    compare the reference updateVoxel chain with the oracle's closed form on random sequences."""
    trials, = inputs_running_average()
    ref = reference_side("running_average", trials)
    col = (10, 200, 31)
    i = 0
    for _, seq in trials:
        for tsdf in seq:
            ot, ow = ref["before"][i, 0], ref["before"][i, 1]
            t_new, w_new = ref["after"][i, 0], ref["after"][i, 1]
            exp_w = min(np.float32(ow + np.float32(1)), np.float32(8.0))
            exp_t = np.float32(np.float32(ot * ow + tsdf * np.float32(1)) / np.float32(ow + np.float32(1)))
            assert w_new == exp_w and t_new.view(np.uint32) == exp_t.view(np.uint32)
            for k in range(3):
                oc = ref["before"][i, 2 + k]
                nc = min(np.float32(255.0), np.float32(np.float32(oc * ow + np.float32(col[k]) * np.float32(2.0)) / np.float32(ow + np.float32(2.0))))
                assert ref["after"][i, 2 + k] == int(nc)
            i += 1
    assert i == 600


def test_integrate_matches_reference_helpers():
    """Run the oracle's integrate on a small volume and replay every voxel through the reference's
    voxelPosToWorld / Mat44 / projectSkeletonToScreen / updateVoxel: identical tsdf+weight bits."""
    res, size, cam, depth, pose, reps = inputs_integrate()
    ref = reference_side("integrate", res, size, cam, depth, pose, reps)
    nrm = np.zeros(depth.shape + (4,), np.float32)
    vol = O.OVolume(res, size, 128.0)
    for rep in range(reps):
        n_upd = O.integrate(vol, depth, nrm, None, False, False, pose, 0.05, 2.0, cam, cam)
        assert ref["n_updated"][rep] == n_upd and n_upd > 500
    assert np.array_equal(ref["tsdf"].view(np.uint32), vol.tsdf.view(np.uint32))
    assert np.array_equal(ref["weight"], vol.weight)


def test_vector_helpers():
    cam, samples = inputs_vector_helpers()
    ref = reference_side("vector_helpers", cam, samples)
    rng = np.random.default_rng(5)
    d = np.ones((480, 640), np.float32)
    d[:] = rng.uniform(0.4, 3.0, d.shape)
    v = O.depth_to_vertices(d, cam)
    n = O.vertices_to_normals(v)
    for i, (x, y, _, _, _) in enumerate(samples):
        assert np.array_equal(bits(ref["skeleton"][i]), bits(v[y, x, :3]))
        assert np.array_equal(bits(ref["normal"][i]), bits(n[y, x, :3]))


def test_color_interpolation_world_to_voxel_and_norm():
    """tsdfVolume.h:123-148 interpolateColor (validity + the truncating float->uchar result), :50-56 worldPosToVoxel and
    cuda_declar.h norm(): the oracle's restatements against the reference's own headers, bit for bit."""
    vol, pts, vecs = inputs_color_world_norm()
    ref = reference_side("color_world_norm", vol, pts, vecs)
    n_ok = 0
    for i, (p, v) in enumerate(zip(pts, vecs)):
        ok, c = O.interpolate_color(vol, p)
        assert bool(ref["ok"][i]) == ok
        if ok:
            n_ok += 1
            assert list(ref["color"][i]) == [int(x) for x in c]
        assert np.array_equal(ref["voxel"][i], O.world_to_voxel(vol, p))
        assert ref["norm"][i].view(np.uint32) == np.float32(O.norm(v)).view(np.uint32)
    assert n_ok > 500


def _unpack_mc_inc(path):
    """csrc/mc_tables.inc / oracle/mc_tables.inc: 256 64-bit words, nibble i = edge id of triTable[c][i], 0xF = -1 (tools/pack_mc_tables.py)."""
    import re
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{16})ull", open(path).read())]
    assert len(words) == 256
    tri = np.full((256, 16), -1, np.int32)
    edge = np.zeros(256, np.int32)
    for c, w in enumerate(words):
        for i in range(16):
            nib = (w >> (4 * i)) & 0xF
            if nib != 0xF:
                tri[c, i] = nib
                edge[c] |= 1 << nib
    return edge, tri


# sha256 of the reference's tables as its own header compiles them (int32 little endian: edgeTable[256], triTable[256][16]), recorded from
# oracle/_ref/libkfref.so::ref_mc_tables so that the pin also holds where the reference is absent (test_mc_tables_hash_without_reference)
MC_EDGE_SHA256 = "ffc58719f11be7a8b34988740a15dcd043dc314a3e2fe01e917fd796001815b9"
MC_TRI_SHA256 = "85e6eb7486ad0101a95aaf3b332a15ba6e5d187a24d31c5eb77874d3aa45d996"


def test_marching_cubes_tables_equal_the_reference_header():
    """edgeTable / triTable of src/cuda/marchingcube_table.h:19,56, compiled as they lie, against the packed tables the HIP kernels
    (hybkinectfu_amd/csrc/mc_tables.inc) and the oracle (oracle/mc_tables.inc) carry: element for element."""
    import hashlib
    import os
    ref = reference_side("mc_tables")
    edge, tri = ref["edge"], ref["tri"]
    assert hashlib.sha256(edge.tobytes()).hexdigest() == MC_EDGE_SHA256 and hashlib.sha256(tri.tobytes()).hexdigest() == MC_TRI_SHA256
    for rel in ("hybkinectfu_amd/csrc/mc_tables.inc", "oracle/mc_tables.inc"):
        e, t = _unpack_mc_inc(os.path.join(O.ROOT, rel))
        assert np.array_equal(t, tri), rel
        assert np.array_equal(e, edge), rel          # the 12-bit edge mask of a case is exactly the set of edges its triangles use
