"""GPU: the persistent ICP loop's fold in 16-byte pairs (csrc/track.hip: fold_batch_pairs; csrc/icp_fold_slots.h).

A publisher's sums 2m and 2m + 1 are one aligned unit {value, tag, value, tag} of its slot row; a lane of the fold polls one such unit per publisher with
one 16-byte load, checks both tags and adds two chains.  Pair 13 carries sum 26 and the padding word, which nobody writes and whose tag is not looked at; a
lane whose slot row is ragged polls its own first unit again and drops it.  The images below put both
on the same lanes: few publishers per level, a second slot row with ONE publisher, a level with a single publisher.  What must hold is what held for
single words (tests/test_gpu_icp_fold_shapes.py, whose helpers these are): the loop's pose bits and final 27 sums are the per-step form's.

Stale halves: the slot arrays of a context are zeroed when it is created and never again.  From the second launch on, every unit a fold polls holds an
earlier launch's halves -- plausible values under an older tag -- until its publisher has stored this launch's.  A context's camera is fixed, so one
context cannot track at two image sizes; the earlier launch here is a track of the SAME image from ANOTHER start pose (different sums in every unit),
at the shape with two batches (656 x 492: 211 / 158 / 40 publishers) and at 256 x 128 (22 / 16 / 4), and the result is compared with the context's
first launch, which ran on zeroed slots.

The SDF loop keeps single words on both sides; its case at VGA (256 publishers, two batches) is tests/test_gpu_icp_fold_shapes.py::test_sdf_loop_with_a_fold_of_two_batches, unchanged."""
import numpy as np
import pytest

from hybkinectfu_amd import lib as K
from test_gpu_icp_fold_shapes import PARTS, FOLD_BATCH, _cam, _publishers
from test_gpu_parity import _tracking_case, mid_cam
from test_gpu_track_forms import _is, _track

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("res,cols,rows,want", [(64, 256, 128, [22, 16, 4]), (64, 272, 128, [23, 17, 5]), (64, 96, 64, [4, 3, 1])])
def test_pair_exchange_loop_equals_the_per_step_form(res, cols, rows, want):
    assert _publishers(cols, rows) == want
    if cols == 272:
        assert want[1] == PARTS + 1                              # a second slot row with one publisher: fifteen lanes per pair poll their first unit again
    if cols == 96:
        assert want[2] == 1                                      # a level with a single publisher: every part but the first adds nothing
    size, trunc = 3.0, 5 * 3.0 / res
    ctx, ovol, pose, nxt, ocam, maps = _tracking_case(res, size, _cam(cols, rows), trunc)
    ok1, p1, st1, it1, form1, sums1 = _track(ctx, pose)
    assert _is(form1, 1)                                        # alone on the device: the persistent loop
    other = K.Context(K.camera(*mid_cam()), 32, 3.0, levels=3)      # a second live context: one launch per step
    ok2, p2, st2, it2, form2, sums2 = _track(ctx, pose)
    other.close()
    assert _is(form2, 2)
    assert ok1 and ok2 and st1 == st2 == 0 and it1 == it2 == 19
    assert np.array_equal(_bits(p1), _bits(p2))                 # same pose bits
    assert np.array_equal(_bits(sums1), _bits(sums2))           # same final 27 sums, the pair with the padding half included
    ctx.close()


@pytest.mark.parametrize("res,cols,rows,want", [(128, 656, 492, [211, 158, 40]), (64, 256, 128, [22, 16, 4])])
def test_halves_of_earlier_launches_are_rejected_by_their_tags(res, cols, rows, want):
    assert _publishers(cols, rows) == want
    if cols == 656:
        assert FOLD_BATCH * PARTS < want[0]                     # two batches: the second polls rows the first launch wrote, too
    size, trunc = 3.0, 5 * 3.0 / res
    ctx, ovol, pose, nxt, ocam, maps = _tracking_case(res, size, _cam(cols, rows), trunc)
    ok0, p0, st0, it0, form0, sums0 = _track(ctx, pose)         # the context's first launch: zeroed slots
    assert _is(form0, 1) and ok0 and st0 == 0 and it0 == 19
    moved = pose.copy()
    moved[:3, 3] += np.float32(0.004)                           # another start: other sums in every unit of every step that runs
    _, p_m, _, _, form_m, sums_m = _track(ctx, moved)
    assert _is(form_m, 1) and not np.array_equal(_bits(sums_m), _bits(sums0))
    ok1, p1, st1, it1, form1, sums1 = _track(ctx, pose)         # nothing cleared in between
    assert _is(form1, 1) and ok1 and st1 == 0 and it1 == 19
    assert np.array_equal(_bits(p1), _bits(p0)) and np.array_equal(_bits(sums1), _bits(sums0))
    ctx.close()
