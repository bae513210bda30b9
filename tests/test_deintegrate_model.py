"""CPU tier: properties of the host model of deintegrateCloud (tests/deintegrate_cases.py) that hold whatever the product
does -- the GPU tier compares the product with this model bit for bit, so what the model promises is what the feature
promises.  32^3, 64 x 48 frames, default truncation limits."""
import numpy as np
import pytest

from cpu_tsdf_amd import synth
from oracle.oracle import OracleVolume
from tests import deintegrate_cases as dc

# The colour of A, C after "A, B, C, remove B" against A, C integrated directly, per channel, in byte steps: the maximum
# measured by this test on the CPU (deterministic; 2026-10-21, all three poses, 32^3).  The forward update truncates
# (up to one step lost per frame), the removal rounds to nearest.
MAX_COLOUR_STEPS = 1


def integrate(ov, fr):
    tr, dep, col = fr
    return ov.integrate(dep, col if ov.rgb is not None else None, synth.cam_from_vol_f32(tr), planes=ov.reference_cull_planes(tr))


@pytest.mark.parametrize("color", [True, False])
@pytest.mark.parametrize("kind", dc.KINDS)
def test_a_then_remove_a_is_the_reset_volume(kind, color):
    vol, sc = dc.volume("32", color=color)
    a = dc.abc(sc, kind)[1]
    ov, fresh = OracleVolume(vol._p), OracleVolume(vol._p)
    n = integrate(ov, a)
    assert n > 500
    assert dc.remove_frame(ov, a[1], a[2], a[0]) == (n, n, n)
    assert np.array_equal(ov.d.view(np.uint32), fresh.d.view(np.uint32)) and np.array_equal(ov.w, fresh.w)
    if color:
        assert np.array_equal(ov.rgb, fresh.rgb)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_a_b_c_remove_b_against_a_c(kind):
    """Three frames (W <= 3): the weights and the observed set are exactly those of A, C alone; d within the project's
    parity bound; colour within MAX_COLOUR_STEPS."""
    vol, sc = dc.volume("32", color=True)
    fr = dc.abc(sc, kind)
    ov, ref = OracleVolume(vol._p), OracleVolume(vol._p)
    for f in fr:
        integrate(ov, f)
    for f in (fr[0], fr[2]):
        integrate(ref, f)
    sel, low, gone = dc.remove_frame(ov, fr[1][1], fr[1][2], fr[1][0])
    assert sel == low > 500 and ov.w.max() <= 2
    assert np.array_equal(ov.w, ref.w)
    assert np.array_equal(ov.w > 0, ref.w > 0) and np.array_equal(ov.d == -1, ref.d == -1)
    dd = float(np.abs(ov.d - ref.d).max())
    steps = int(np.abs(ov.rgb.astype(np.int32) - ref.rgb.astype(np.int32)).max())
    print(f"{kind}: {sel} selected, {gone} back to unobserved, max |dd| = {dd:.3g}, max colour step = {steps}")
    assert dd <= 1e-5
    assert steps == MAX_COLOUR_STEPS
    assert np.array_equal(ov.rgb[ov.w == 0], ref.rgb[ov.w == 0])


@pytest.mark.parametrize("kind", dc.KINDS)
def test_voxels_that_only_saw_the_hinge_keep_its_bits(kind):
    """trunc = (0.011, 0.02) under max_weight 3: the hinge value p = 0.55 rests under the forward update for every weight
    up to 3 ((p * w + p) / (w + 1) == p in float32), but (p * 3 - p) / 2 is NOT p: only the equal-bits rule keeps a voxel
    that three frames saw in free space at p when one of them leaves.  The band is narrow enough for free space to exist
    at 32^3."""
    trunc = dc.RESTING_TRUNC
    f = np.float32
    p_ = f(trunc[0]) / f(trunc[1])
    assert all(f(f(p_ * f(k)) + p_) / f(k + 1) == p_ for k in range(4)) and f(f(p_ * f(3)) - p_) / f(2) != p_
    vol, sc = dc.volume("32", color=False, trunc=trunc, max_weight=3.0)
    fr = dc.abc(sc, kind)
    p = np.float32(trunc[0]) / np.float32(trunc[1])
    ov = OracleVolume(vol._p)
    only_hinge = np.ones(ov.d.shape, bool)
    for tr, dep, col in fr:
        sel, d_new, _ = dc.observation(vol._p, dep, None, tr)
        only_hinge &= ~sel | (d_new == p)
        integrate(ov, (tr, dep, None))
    seen_by_b, _, _ = dc.observation(vol._p, fr[1][1], None, fr[1][0])
    rest = only_hinge & (ov.w > 0)
    assert (rest & seen_by_b & (ov.w == 3)).sum() > 50 and np.all(ov.d[rest] == p)
    dc.remove_frame(ov, fr[1][1], None, fr[1][0])
    still = rest & (ov.w > 0)
    assert (still & seen_by_b).sum() > 50
    assert np.all(ov.d[still].view(np.uint32) == np.array(p, np.float32).view(np.uint32))
    assert np.all(ov.d[rest & (ov.w == 0)] == -1)
