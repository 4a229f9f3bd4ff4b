"""GPU: the z-slab merge SlabPipeline runs, from every side, against the oracle's whole-volume raycast.

Every slab marches every ray and clips the march to its owned layers (the slab clip of raycast_tile): kf_raycast_volume_slab_cross_spec, the MIN over
the slabs' crossing words, kf_slab_ray_normals_spec (the vertex's owner evaluates its gradient), the integer SUM of the candidates and
kf_set_model_maps_rays.  The rest of the suite merges only rays that rise through the slabs (dir.z > 0, near slab first).  Here the viewpoints of
raycast_scenarios.py -- falling rays (the far slab meets the surface first), rays parallel to the slab planes, cameras inside the volume and inside a
solid -- cast the analytic volumes at 104^3 and 128^3 over 2 and 3 slabs, at the default forms; the merged maps and levels 1 and 2 of their pyramids
must equal the oracle's bit for bit."""
import numpy as np
import pytest
import torch

import raycast_scenarios as R
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import pipeline as PL

pytestmark = pytest.mark.gpu
P = R.P


def _merge(slabs, cam, pose, inc, near, far, dev):
    """the slab protocol of SlabPipeline on contexts that share one device; returns the crossing words' MIN"""
    tas, owns, specs = [], [], []
    for c in slabs:
        ta, own = torch.empty((cam[1], cam[0]), dtype=torch.int64, device=dev), torch.empty((cam[1], cam[0]), dtype=torch.int64, device=dev)
        spec = torch.empty((cam[1], cam[0], 3), dtype=torch.float32, device=dev)
        c.raycast_slab_cross_spec(pose, inc, near, far, ta.data_ptr(), own.data_ptr(), spec.data_ptr())
        f = c.raycast_form()
        assert f["kernel"] == K.RC_PLAIN and f["output"] == K.RC_OUT_TA_SPEC and f["pyramid"] == 0, f
        tas.append(ta); owns.append(own); specs.append(spec)
    for c in slabs:
        c.sync()
    ta_min = torch.stack(tas).min(dim=0).values.contiguous()
    acc = torch.zeros((cam[1], cam[0], 3), dtype=torch.int32, device=dev)
    for c, own, spec in zip(slabs, owns, specs):
        cand = torch.empty((cam[1], cam[0], 3), dtype=torch.float32, device=dev)
        c.slab_ray_normals_spec(pose, inc, near, far, ta_min.data_ptr(), own.data_ptr(), spec.data_ptr(), cand.data_ptr())
        c.sync()
        acc += cand.view(torch.int32)
    rays = acc.view(torch.float32).contiguous()
    for c in slabs:
        c.set_model_maps_rays(pose, ta_min.data_ptr(), rays.data_ptr())
        c.sync()
    return ta_min


@pytest.mark.parametrize("vid", ["a104", "a128"])
def test_slab_merge_from_every_side_equals_the_whole_volume(vid):
    vol = next(v for v in R.VOLUMES if v[0] == vid)
    _, res, size, _, _ = vol
    data = R.volume_data(vol)
    ovol = R.oracle_volume(vol, data)
    inc = R.inc_for(res, size)
    halo = PL.slab_halo_layers(res, size, inc)
    dev = torch.device("cuda", 0)
    calls = R.calls(vol)
    want = {call[0]: R.oracle_maps(vol, ovol, call) for call in calls}
    for n in (2, 3):
        for cam in sorted({call[1] for call in calls}):
            kcam = K.camera(*cam)
            slabs = [K.Context(kcam, res, size, P["volume_max_weight"], levels=3, slab=r, halo=halo) for r in PL.slab_ranges(res, n)]
            for c in slabs:
                c.upload_volume(data[0][c.stored[0]:c.stored[1]], data[1][c.stored[0]:c.stored[1]])
            falling = 0
            for k, ccam, view, pose, near, far in calls:
                if ccam != cam:
                    continue
                ta_min = _merge(slabs, cam, pose, inc, near, far, dev)
                w = want[k]
                # (there is something to compare: the scenario's own minimum, met by the merge's crossings too)
                assert int((ta_min.cpu().numpy() >> 32 != 0x7F800000).sum()) >= R.min_hits(view, cam), (n, k)
                for c in slabs:
                    for lv, (tv, tn) in enumerate((("v", "n"), ("v1", "n1"), ("v2", "n2"))):
                        gv, gn = c.download_map(K.MAP_MODEL_VERTICES, lv), c.download_map(K.MAP_MODEL_NORMALS, lv)
                        assert np.array_equal(gv.view(np.uint32), w[tv].view(np.uint32)), (n, k, lv, c.owned)
                        assert np.array_equal(gn.view(np.uint32), w[tn].view(np.uint32)), (n, k, lv, c.owned)
                falling += int(pose[2, 2] < 0)
            assert falling >= 3 or cam != R.RAGGED, falling
            for c in slabs:
                c.close()
