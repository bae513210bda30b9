"""CPU tier: the inputs of the host model of reintegrateCloud (tests/reintegrate_cases.py) hold every case the kernel can get
wrong -- voxels both poses select, voxels only one of them selects, voxels the removal clears and the addition observes
again, NaN pixels, voxels beyond the truncation distance, and, in the 64^3 flag case, in-band additions in cells nothing has
flagged beside free space that rests at the hinge value on both sides.  The GPU tier compares the product with this model
bit for bit.  The floors stand well under the figures the model gives (tests/test_reintegrate_gpu.py prints them)."""
import numpy as np
import pytest

from cpu_tsdf_amd import synth
from oracle.oracle import OracleVolume
from tests import deintegrate_cases as dc
from tests import reintegrate_cases as rc


def integrate(ov, fr):
    tr, dep, col = fr
    return ov.integrate(dep, col, synth.cam_from_vol_f32(tr), planes=ov.reference_cull_planes(tr))


def test_the_correction_is_rigid_and_small():
    c = rc.correction(3.0)
    assert np.allclose(c[:3, :3] @ c[:3, :3].T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(c[:3, :3]), 1.0)
    assert np.allclose(c[:3, 3], (0.12, -0.039, 0.063)) and np.array_equal(c[3], (0, 0, 0, 1))
    angle = np.degrees(np.arccos((np.trace(c[:3, :3]) - 1) / 2))
    assert 1.5 < angle < 1.8


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("grid", list(dc.GRIDS))
def test_the_frames_hold_every_case(grid, kind):
    vol, sc = dc.volume(grid, color=True)
    fr = dc.abc(sc, kind)
    ov = OracleVolume(vol._p)
    for f in fr:
        integrate(ov, f)
    tr, dep, col = fr[1]
    new = rc.correction(sc.size) @ tr
    both, only_old, only_new, again = rc.repose_sets(vol._p, dep, col, tr, new, ov.w)
    nans, beyond = dc.frame_facts(vol._p, dep, col, tr)
    w_before = ov.w.copy()
    st = rc.reintegrate_frame(ov, dep, col, tr, new)
    print(f"{grid} {kind}: old {st[0]} new {st[3]} both {both} only old {only_old} only new {only_new} cleared and observed again "
          f"{again}; lowered {st[1]} cleared {st[2]}; {nans} NaN pixels, {beyond} voxels beyond the truncation distance")
    assert st[4] == both and st[0] == both + only_old and st[3] == both + only_new
    assert nans > 10 and beyond > 100
    if kind == "inside":
        assert both > 500 and only_old > 300 and only_new > 300
    else:
        assert both > 20000 and only_old > 500 and only_new > 500 and again > 100
    # the weights: one down where old selected an observed voxel, one up where new observes (no saturation at max_weight 100)
    so = dc.observation(vol._p, dep, col, tr)[0]
    sn = dc.observation(vol._p, dep, col, new)[0]
    assert np.array_equal(ov.w, w_before - (so & (w_before != 0)) + sn)


def test_both_poses_equal_leaves_the_weights_and_the_observed_set():
    """old == new: every selected voxel loses and regains one count; d and the colour move by rounding only."""
    vol, sc = dc.volume("32", color=True)
    fr = dc.abc(sc, "rolled")
    ov = OracleVolume(vol._p)
    for f in fr:
        integrate(ov, f)
    before = (ov.d.copy(), ov.w.copy(), ov.rgb.copy())
    tr, dep, col = fr[1]
    st = rc.reintegrate_frame(ov, dep, col, tr, tr)
    assert st[0] == st[1] == st[3] == st[4] > 20000
    assert np.array_equal(ov.w, before[1])
    assert float(np.abs(ov.d - before[0]).max()) <= 1e-5
    assert int(np.abs(ov.rgb.astype(np.int32) - before[2].astype(np.int32)).max()) <= 1


def test_a_missing_pose_makes_it_one_of_the_two_calls():
    vol, sc = dc.volume("32", color=True)
    fr = dc.abc(sc, "outside")
    a, b = OracleVolume(vol._p), OracleVolume(vol._p)
    for f in fr:
        integrate(a, f), integrate(b, f)
    tr, dep, col = fr[1]
    st = rc.reintegrate_frame(a, dep, col, tr, None)
    assert st[:3] == dc.remove_frame(b, dep, col, tr) and st[3:] == (0, 0)
    assert np.array_equal(a.d.view(np.uint32), b.d.view(np.uint32)) and np.array_equal(a.w, b.w) and np.array_equal(a.rgb, b.rgb)
    st = rc.reintegrate_frame(a, dep, col, None, tr)
    assert st == (0, 0, 0, integrate(b, fr[1]), 0)
    assert np.array_equal(a.d.view(np.uint32), b.d.view(np.uint32)) and np.array_equal(a.w, b.w) and np.array_equal(a.rgb, b.rgb)


@pytest.mark.parametrize("who", ["own B", "stranger"])
def test_the_flag_case_holds_additions_no_launch_has_flagged(who):
    """The 64^3 flag case of tests/test_deintegrate_gpu.flag_case: re-posing frame B (or the stranger sphere of 0.36) puts
    in-band additions into cells that no earlier launch and not the removal half can have flagged, while most of what both
    poses select rests at the hinge value p on both sides."""
    vol, sc = dc.volume((64, 64, 64), color=True, max_weight=3.0, trunc=dc.RESTING_TRUNC)
    sc = synth.Scene(sc.size, sc.width, sc.height, box=0.6)
    model = rc.ReposeModel(vol._p, cull=True)
    trs = [synth.turntable_pose(i, 8, sc.size) for i in (0, 1, 2)]
    for i, tr in enumerate(trs):
        model.integrate(*dc.frame(sc, i, tr), tr)
    p = np.float32(dc.RESTING_TRUNC[0]) / np.float32(dc.RESTING_TRUNC[1])
    scene, idx = (sc, 1) if who == "own B" else (synth.Scene(sc.size, sc.width, sc.height, sphere=0.36, box=0.6), 7)
    dep, col = dc.frame(scene, idx, trs[1])
    fresh, resting = rc.flag_facts(model.ov, vol._p, dep, col, trs[1], rc.correction(sc.size) @ trs[1], p)
    print(f"{who}: {fresh} in-band additions in cells nothing has flagged, {resting} resting voxels selected by both at p")
    assert fresh > 100 and resting > 100000
