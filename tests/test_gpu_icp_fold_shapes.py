"""GPU: the persistent tracking loops at publisher counts that sit on the edges of the fold's slot rule.

A lane of the fold (fold_partials_tagged, csrc/track.hip) polls, per batch of 13 x parts publishers, only as many tagged words as the batch has slot rows with a
publisher (icp_fold_batch_slots, csrc/icp_fold_slots.h: 3, 10 or 13 of them).  At 16 parts (512 lanes) the images below put the publishers of
their pyramid levels where that count changes, or where a second batch begins:
  256 x 128 -> 22 / 16 / 4 publishers (a full first row, and a ragged one);   272 x 128 -> 23 / 17 / 5 (the second row begins at 17);
  656 x 492 -> 211 / 158 / 40 (above 13 x 16 = 208: a second batch with 3 real slots);   the SDF loop at VGA: 256 publishers, two batches.
Same helpers and assertions as tests/test_gpu_track_forms.py: the persistent loop against the one-launch-per-step form (bitwise for the ICP, whose forms deal
pixels alike; to tolerance for the SDF tracker) and both within 1e-4 of the oracle."""
import numpy as np
import pytest

import oracle_lib as O
from hybkinectfu_amd import lib as K
from test_gpu_parity import _tracking_case, mid_cam
from test_gpu_track_forms import SDF, _is, _oracle_pose, _track, _track_sdf

pytestmark = pytest.mark.gpu

ICP_THREADS, ICP_PX, FOLD_BATCH = 512, 3, 13
PARTS = ICP_THREADS // 32


def _div_up(a, b):
    return (a + b - 1) // b


def _publishers(cols, rows, levels=3):
    """icp_level_geometry (csrc/icp_fold_slots.h) for every pyramid level: the fewest pixels per lane the launch's level-0 grid can hold"""
    grid0 = _div_up(cols * rows, ICP_THREADS * ICP_PX)
    out = []
    for l in range(levels):
        npx = (cols >> l) * (rows >> l)
        px_l = next((p for p in range(1, ICP_PX) if _div_up(npx, ICP_THREADS * p) <= grid0), ICP_PX)
        out.append(_div_up(npx, ICP_THREADS * px_l))
    return out


def _cam(cols, rows):
    """the VGA camera's field of view at another image size"""
    f = 525.0 * cols / 640.0
    return (cols, rows, (cols - 1) / 2.0, (rows - 1) / 2.0, f, f)


@pytest.mark.parametrize("res,cols,rows,want", [(64, 256, 128, [22, 16, 4]), (64, 272, 128, [23, 17, 5]), (128, 656, 492, [211, 158, 40])])
def test_icp_loop_at_the_edges_of_the_slot_rule(res, cols, rows, want):
    assert _publishers(cols, rows) == want
    if cols == 272:
        assert want[1] == PARTS + 1                              # one publisher in the second slot row
    if cols == 656:
        assert FOLD_BATCH * PARTS < want[0] <= FOLD_BATCH * PARTS + 3 * PARTS      # a second batch, of at most 3 real slots
    size, trunc = 3.0, 5 * 3.0 / res
    ctx, ovol, pose, nxt, ocam, maps = _tracking_case(res, size, _cam(cols, rows), trunc)
    ok_o, pose_o = _oracle_pose(maps, ocam, pose)
    ok1, p1, st1, it1, form1, sums1 = _track(ctx, pose)
    assert _is(form1, 1)                                        # alone on the device: the persistent loop -- a size it refuses must not pass silently
    other = K.Context(K.camera(*mid_cam()), 32, 3.0, levels=3)      # a second live context: one launch per step
    ok2, p2, st2, it2, form2, sums2 = _track(ctx, pose)
    other.close()
    assert _is(form2, 2)
    assert ok1 and ok2 and ok_o and st1 == st2 == 0 and it1 == it2 == 19
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))            # same pose bits
    assert np.array_equal(sums1.view(np.uint32), sums2.view(np.uint32))      # same final 27 sums
    for p in (p1, p2):
        assert np.max(np.abs(p[:3, 3] - pose_o[:3, 3])) < 1e-4 and np.max(np.abs(p[:3, :3] - pose_o[:3, :3])) < 1e-4
    ok3, p3, _, _, form3, _ = _track(ctx, pose)              # alone again: back on the loop, same bits
    assert _is(form3, 1) and np.array_equal(p3.view(np.uint32), p1.view(np.uint32))
    ctx.close()


def test_sdf_loop_with_a_fold_of_two_batches():
    """VGA: the SDF loop runs one workgroup per CU, at most one per 8 tiles of 8 x 8 pixels -- 256 publishers on a 256-CU device: 13 + 3 slot rows"""
    import torch
    from hybkinectfu_amd import scene as S
    cam = S.vga_camera()
    n_pub = min(torch.cuda.get_device_properties(0).multi_processor_count, _div_up(_div_up(cam[0], 8) * _div_up(cam[1], 8), ICP_THREADS // 64))
    assert FOLD_BATCH * PARTS < n_pub <= FOLD_BATCH * PARTS + 3 * PARTS, n_pub
    res = 128
    size, trunc = 3.0, 5 * 3.0 / res
    ctx, ovol, pose, nxt, ocam, (v, n, ov, on, tr) = _tracking_case(res, size, cam, trunc, n_warm=3)
    ok_o, pose_o, it_o = O.sdf_estimate(ovol, tr, ocam, *SDF, pose)
    ok1, p1, st1, it1, form1, sums1 = _track_sdf(ctx, pose)
    assert _is(form1, 1)
    other = K.Context(K.camera(*mid_cam()), 32, 3.0, levels=3)
    ok2, p2, st2, it2, form2, sums2 = _track_sdf(ctx, pose)
    other.close()
    assert _is(form2, 2)
    assert ok_o and ok1 and ok2 and st1 == st2 == 0 and it1 == it2 == it_o, (it1, it2, it_o)
    for p in (p1, p2):
        assert np.max(np.abs(p - pose_o)) < 1e-4
    assert np.max(np.abs(sums1 - sums2)) <= 2e-5 * np.max(np.abs(sums2))     # the last iteration's system, two summation orders
    ok3, p3, _, it3, form3, sums3 = _track_sdf(ctx, pose)                      # the loop again: reproducible to the bit
    assert _is(form3, 1) and np.array_equal(p3.view(np.uint32), p1.view(np.uint32)) and np.array_equal(sums3.view(np.uint32), sums1.view(np.uint32))
    ctx.close()
