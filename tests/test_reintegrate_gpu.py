"""GPU tier: tsdf_hip_reintegrate (cpu_tsdf_amd/csrc/tsdf_reintegrate.hip) -- a fused frame re-posed in one sweep.  Every
expectation is the host model of tests/reintegrate_cases.py (the removal model of tests/deintegrate_cases.py under the old
pose, then the oracle's integrate under the new pose with the new pose's planes), compared BIT FOR BIT with download() on d,
w and rgb.  The "band seen" flags are checked through what their readers do afterwards: the fast integrate kernels' implied
distances and marching cubes' skips."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection time, before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import reference_cull_planes
from oracle.oracle import OracleVolume
from tests import deintegrate_cases as dc
from tests import pose_cases
from tests import reintegrate_cases as rc
from tests.common import assert_same_f32
from tests.sequence_model import assert_same_mesh, compare
from tests.sequence_util import march, read_detail
from tests.test_occupied_gpu import check as check_occupied
from tests.test_occupied_gpu import expected as expected_occupied

pytestmark = pytest.mark.gpu
PACKED, F32W = capi.LAYOUT_PACKED, capi.LAYOUT_F32W
LAYOUTS = {"packed": PACKED, "f32w": F32W}


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def cfv(tr):
    return synth.cam_from_vol_f32(tr)


def oracle_integrate(ov, fr, zb=0, ze=0):
    tr, dep, col = fr
    return ov.integrate(dep, col if ov.rgb is not None else None, cfv(tr), zb, ze, planes=ov.reference_cull_planes(tr))


def integrate(vol, fr, **kw):
    tr, dep, col = fr
    return vol.integrateCloud(dep, col if vol._p.integrate_color else None, tr, **kw)


def repose(vol, fr, new, count=True):
    tr, dep, col = fr
    return vol.reintegrateCloud(dep, col if vol._p.integrate_color else None, tr, new, count=count)


def model_repose(ov, fr, new):
    return rc.reintegrate_frame(ov, fr[1], fr[2], fr[0], new)


def same_planes(got, want, what):
    assert_same_f32(got[0], want[0], what + ": d")
    assert_same_f32(got[1], want[1], what + ": w")
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]), what + ": rgb"


def raw_call(vol, dep, col, To, po, Tn, pn, n=None):
    """The C entry point itself: its return code."""
    f32 = lambda a: None if a is None else capi.as_f32p(np.ascontiguousarray(a, np.float32))
    return capi.load().tsdf_hip_reintegrate(vol._h, None if dep is None else capi.as_f32p(dep), None if col is None else capi.as_u8p(col),
                                            f32(To), f32(po), f32(Tn), f32(pn), n)


_MODELS = {}


def abc_model(grid, kind, color, order):
    """Frames A, B, C of `kind` on `grid`, B's corrected pose, and the model after A, B, C, re-pose B with its five counts.
    Shared, never modified."""
    key = (grid, kind, color, order)
    if key not in _MODELS:
        vol, sc = dc.volume(grid, color=color, order=order)
        fr = dc.abc(sc, kind)
        new = rc.correction(sc.size) @ fr[1][0]
        ov = OracleVolume(vol._p)
        for f in fr:
            oracle_integrate(ov, f)
        st = model_repose(ov, fr[1], new)
        assert st[0] == st[1] > 500 and st[3] > 500 and 0 < st[4] < min(st[0], st[3]), (key, st)
        _MODELS[key] = (fr, new, ov, st)
    return _MODELS[key]


# ---- 1. A, B, C, re-pose B: every layout, colour setting, transform order, grid and pose -------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_b_c_repose_b_equals_the_model(gpu, layout, color, order):
    for grid in dc.GRIDS:
        for kind in dc.KINDS:
            fr, new, ov, st = abc_model(grid, kind, color, order)
            vol, _ = dc.volume(grid, color=color, order=order, layout=LAYOUTS[layout])
            vol.reset()
            assert vol.getLayout() == LAYOUTS[layout]
            for f in fr:
                integrate(vol, f)
            n = repose(vol, fr[1], new)
            what = f"{grid} {kind} {layout} colour {color} order {order}"
            compare(vol, ov, what)
            got = vol.reintegrateStats()
            print(what, "stats", got, "model", st)
            assert n == (st[1], st[3]) and got[:5] == st, (what, n, got, st)
            vol.close()


# ---- 2. the product's own two calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", dc.KINDS)
def test_equals_deintegrate_then_integrate(gpu, kind, layout):
    """A twin handle takes deintegrateCloud(old) + integrateCloud(new): the planes, the mesh and the occupied list agree."""
    fr, new, ov, st = abc_model("38x24x36", kind, True, 0)
    one, _ = dc.volume("38x24x36", color=True, layout=LAYOUTS[layout])
    two, _ = dc.volume("38x24x36", color=True, layout=LAYOUTS[layout])
    for vol in (one, two):
        vol.reset()
        for f in fr:
            integrate(vol, f)
    tr, dep, col = fr[1]
    n = repose(one, fr[1], new)
    lowered = two.deintegrateCloud(dep, col, tr, count=True)
    observed = two.integrateCloud(dep, col, new, count=True)
    assert n == (lowered, observed) == (st[1], st[3])
    same_planes(one.download(), two.download(), f"{kind} {layout}: one call against two")
    compare(one, ov, f"{kind} {layout}")
    m1, m2 = march(one, True)[0], march(two, True)[0]
    assert len(m1["cells"]) > 100
    assert_same_mesh(m1, m2, f"{kind} {layout}: mesh")
    idx = one.getOccupiedVoxelIndices(None, want=("d", "w", "rgb"))
    idx2 = two.getOccupiedVoxelIndices(None, want=("d", "w", "rgb"))
    assert len(idx[0]) > 100 and all(np.array_equal(a, b) for a, b in zip(idx, idx2))
    check_occupied(one, expected_occupied(ov.d, ov.w, ov.rgb), what=f"{kind} {layout}: occupied")
    one.close()
    two.close()


# ---- 3. saturation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_saturated_voxels_lose_one_count_and_regain_it(gpu, color):
    """max_weight = 2, four frames from one pose, the third re-posed: voxels at the limit go to 1 and, where the new pose
    observes them, back to 2 -- PACKED and F32W agree with the model and with each other."""
    outs = []
    for layout in (PACKED, F32W):
        vol, sc = dc.volume("32", color=color, layout=layout, max_weight=2.0)
        vol.reset()
        tr = dc.pose("outside", sc.size)
        fr = [(tr,) + dc.frame(sc, i, tr) for i in range(4)]
        new = rc.correction(sc.size) @ tr
        ov = OracleVolume(vol._p)
        for f in fr:
            integrate(vol, f)
            oracle_integrate(ov, f)
        assert (ov.w == 2).sum() > 500
        n = repose(vol, fr[2], new)
        st = model_repose(ov, fr[2], new)
        assert n == (st[1], st[3]) and vol.reintegrateStats()[:5] == st and st[2] < st[1]
        assert ov.w.max() == 2 and (ov.w == 1).sum() > 500 and (ov.w == 2).sum() > 500
        outs.append(compare(vol, ov, f"max_weight 2, layout {layout}"))
        vol.close()
    same_planes(outs[0], outs[1], "PACKED against F32W")


def test_a_non_integer_weight_limit_on_f32w(gpu):
    """max_weight = 2.5 (F32W): a voxel at 2.5 has W = ceil(2.5) = 3, goes to 2 and, observed again, to 3 -> clamped to 2.5."""
    vol, sc = dc.volume("32", color=True, layout=F32W, max_weight=2.5)
    vol.reset()
    tr = dc.pose("rolled", sc.size)
    fr = [(tr,) + dc.frame(sc, i, tr) for i in range(4)]
    new = rc.correction(sc.size) @ tr
    ov = OracleVolume(vol._p)
    for f in fr:
        integrate(vol, f)
        oracle_integrate(ov, f)
    assert (ov.w == 2.5).sum() > 500
    n = repose(vol, fr[0], new)
    st = model_repose(ov, fr[0], new)
    assert n == (st[1], st[3]) and (ov.w == 2).sum() > 500 and (ov.w == 2.5).sum() > 500
    compare(vol, ov, "max_weight 2.5")
    vol.close()


# ---- 4. the flags, through their readers -----------------------------------------------------------------------------------
def flag_case():
    """tests/test_deintegrate_gpu.flag_case with the re-pose model: 64^3, PACKED + colour, dc.RESTING_TRUNC under max_weight
    3 -- the record stays at rest_state == 1 and most of the volume is free space in cells whose flag is 0."""
    vol, sc = dc.volume((64, 64, 64), color=True, layout=PACKED, max_weight=3.0, trunc=dc.RESTING_TRUNC)
    sc = synth.Scene(sc.size, sc.width, sc.height, box=0.6)   # the walls outside the grid: only the sphere is a surface
    return vol, sc, rc.ReposeModel(vol._p, cull=True)


def readers_after(vol, model, sc, what):
    """A fourth turntable frame through the fast kernel, then the mesh: (allowed, skipped > 0, flags in use, march read less
    than the whole distance plane)."""
    tr = synth.turntable_pose(3, 8, sc.size)
    dep, col = dc.frame(sc, 3, tr)
    n = vol.integrateCloud(dep, col, tr, count=True)
    assert n == model.integrate(dep, col, tr)
    skipped, allowed = read_detail(vol)
    compare(vol, model.ov, what + ": one more frame through the fast kernel")
    mesh, st = march(vol, True)
    assert len(mesh["cells"]) > 500
    assert_same_mesh(mesh, model.mesh(1.0), what + ": mesh")
    check_occupied(vol, model.occupied(), what=what + ": occupied")
    whole = 64 * 64 * 64 * 4
    print(f"{what}: implied {skipped} of {n}, allowed {allowed}, march read {st[2]} of {whole} bytes, flags {st[3]}")
    return allowed, skipped > 0, st[3] & 1, st[2] < whole


@pytest.mark.parametrize("who", ["own B", "stranger"])
def test_the_flags_survive_a_repose(gpu, who):
    """Re-posing B (or a stranger: a larger sphere whose surface lies in what the volume holds as free space) puts in-band
    additions into cells no launch has flagged; the next integrate goes through the fast kernel with implied distances on
    and may only rebuild distances from counts where the flags still allow it.  Planes equal the model, the mesh equals the
    oracle's march of the model, and the readers skip what they skip in a run that never needed a correction."""
    vol, sc, model = flag_case()
    vol.reset()
    trs = [synth.turntable_pose(i, 8, sc.size) for i in (0, 1, 2)]
    for i, tr in enumerate(trs):
        dep, col = dc.frame(sc, i, tr)
        vol.integrateCloud(dep, col, tr, count=True)
        model.integrate(dep, col, tr)
        assert read_detail(vol)[1] == 1
    compare(vol, model.ov, "three frames")
    p = np.float32(dc.RESTING_TRUNC[0]) / np.float32(dc.RESTING_TRUNC[1])
    scene, idx = (sc, 1) if who == "own B" else (synth.Scene(sc.size, sc.width, sc.height, sphere=0.36, box=0.6), 7)
    dep, col = dc.frame(scene, idx, trs[1])
    new = rc.correction(sc.size) @ trs[1]
    fresh, resting = rc.flag_facts(model.ov, vol._p, dep, col, trs[1], new, p)
    assert fresh > 100 and resting > 100000, (fresh, resting)
    n = vol.reintegrateCloud(dep, col, trs[1], new, count=True)
    st = model.reintegrate(dep, col, trs[1], new)
    assert n == (st[1], st[3]) and vol.reintegrateStats()[:5] == st and st[1] > 5000
    compare(vol, model.ov, f"{who} re-posed")
    seen = readers_after(vol, model, sc, f"{who} re-posed")
    assert seen == (1, True, 1, True), seen
    vol.close()
    if who == "own B":   # A, C, B under the corrected pose, D: no correction at all
        vol, sc, model = flag_case()
        vol.reset()
        for i, tr in ((0, trs[0]), (2, trs[2]), (1, new)):
            dep, col = dc.frame(sc, i, trs[i])
            vol.integrateCloud(dep, col, tr)
            model.integrate(dep, col, tr)
        assert readers_after(vol, model, sc, "never corrected") == seen
        vol.close()


# ---- 5. the reference's frustum cull ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_cull_bites_differently_for_the_two_poses(gpu, layout):
    """The off-centre principal point and yawed cameras of test_the_removal_selects_the_culled_set: each half selects the
    set its own pose's pyramid leaves, and planes_new stay in force on the handle."""
    vol, sc = dc.volume("32", color=True, layout=LAYOUTS[layout])
    sc.cx += 0.6 * dc.W / 2
    vol.setCameraIntrinsics(sc.fx, sc.fy, sc.cx, sc.cy)
    vol.reset()
    psi = float(np.arctan(0.6 * (dc.W / 2) / sc.fx))
    yaw = np.eye(4)
    yaw[0, 0], yaw[0, 2], yaw[2, 0], yaw[2, 2] = np.cos(psi), np.sin(psi), -np.sin(psi), np.cos(psi)
    fr = []
    for i in range(3):
        tr = synth.turntable_pose(2 * i + 1, 8, sc.size) @ (yaw @ pose_cases.roll_about_optical_axis(20.0 * i))
        fr.append((tr,) + dc.frame(sc, i, tr))
    ov, unculled = OracleVolume(vol._p), OracleVolume(vol._p)
    for f in fr:
        want = oracle_integrate(ov, f)
        assert want < unculled.integrate(f[1], f[2], cfv(f[0])), "the cull does not bite"
        assert integrate(vol, f, count=True) == want
    tr, dep, col = fr[1]
    new = rc.correction(sc.size) @ tr
    loose_old = int(dc.observation(vol._p, dep, col, tr, cull=False)[0].sum())
    loose_new = int(dc.observation(vol._p, dep, col, new, cull=False)[0].sum())
    n = (C.c_uint64 * 2)()
    po, pn = reference_cull_planes(vol._p, tr), reference_cull_planes(vol._p, new)
    assert not np.array_equal(po, pn)
    assert raw_call(vol, dep, col, cfv(tr), po, cfv(new), pn, n) == capi.OK
    st = model_repose(ov, fr[1], new)
    assert (n[0], n[1]) == (st[1], st[3]) and vol.reintegrateStats()[:5] == st
    assert st[0] < loose_old and st[3] < loose_new
    compare(vol, ov, "culled A, B, C, re-pose B")
    # a raw integrate, no tsdf_hip_set_reference_cull in between: the new pose's planes are in force
    tr3, dep3, col3 = fr[2]
    n1 = C.c_uint64(0)
    capi.check(capi.load().tsdf_hip_integrate(vol._h, capi.as_f32p(dep3), capi.as_u8p(col3), capi.as_f32p(cfv(tr3)), C.byref(n1)), "integrate")
    want = ov.integrate(dep3, col3, cfv(tr3), planes=ov.reference_cull_planes(new))
    twin = OracleVolume(vol._p)
    assert want == n1.value and want != twin.integrate(dep3, col3, cfv(tr3), planes=twin.reference_cull_planes(tr3))
    compare(vol, ov, "a raw integrate under planes_new")
    vol.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_planes_alone(gpu):
    lib = capi.load()
    n = (C.c_uint64 * 2)(7, 9)

    def args(vol, fr, sc):
        tr, dep, col = fr
        new = rc.correction(sc.size) @ tr
        return dep, col, cfv(tr), reference_cull_planes(vol._p, tr), cfv(new), reference_cull_planes(vol._p, new)

    def refused(vol, fr, sc, code, what):
        before = vol.download()
        assert raw_call(vol, *args(vol, fr, sc), n) == code, what
        assert (n[0], n[1]) == (7, 9), what
        same_planes(vol.download(), before, what)

    # the weightings (F32W; setWeighting takes effect at reset()), and the variance state once it has been allocated
    for by_depth, by_variance in ((True, False), (False, True)):
        vol, sc = dc.volume("32", color=True, layout=F32W)
        vol.setWeighting(by_depth=by_depth, by_variance=by_variance)
        vol.reset()
        fr = dc.abc(sc, "outside")
        integrate(vol, fr[0])
        refused(vol, fr[0], sc, capi.E_UNSUPPORTED, f"weighting {by_depth} {by_variance}")
        if by_variance:
            capi.check(lib.tsdf_hip_set_weighting(vol._h, 0, 0), "set_weighting")   # the flag goes, M_ / nsample_ stay
            refused(vol, fr[0], sc, capi.E_UNSUPPORTED, "variance state allocated")
        vol.close()
    # the two colour modes
    for mode in ("RGBNormalized", "LAB"):
        vol, sc = dc.volume("32", color=True)
        vol.setColorMode(mode)
        vol.reset()
        fr = dc.abc(sc, "outside")
        integrate(vol, fr[0])
        refused(vol, fr[0], sc, capi.E_UNSUPPORTED, mode)
        vol.close()
    # a set
    vol, sc = dc.volume("32", color=True)
    vol.setDevices([0, 0])
    vol.reset()
    fr = dc.abc(sc, "outside")
    integrate(vol, fr[0])
    refused(vol, fr[0], sc, capi.E_UNSUPPORTED, "devices [0, 0]")
    assert b"multi" in lib.tsdf_hip_last_error()
    vol.close()
    # null arguments, a missing colour image
    vol, sc = dc.volume("32", color=True)
    vol.reset()
    fr = dc.abc(sc, "outside")
    ov = OracleVolume(vol._p)
    for f in fr:
        integrate(vol, f)
        oracle_integrate(ov, f)
    dep, col, To, po, Tn, pn = args(vol, fr[1], sc)
    before = vol.download()
    assert raw_call(vol, None, col, To, po, Tn, pn, n) == capi.E_INVALID
    assert raw_call(vol, dep, col, None, po, Tn, pn, n) == capi.E_INVALID
    assert raw_call(vol, dep, col, To, po, None, pn, n) == capi.E_INVALID
    assert raw_call(vol, dep, None, To, po, Tn, pn, n) == capi.E_INVALID
    assert lib.tsdf_hip_reintegrate_device(vol._h, None, None, capi.as_f32p(To), None, capi.as_f32p(Tn), None, n) == capi.E_INVALID
    assert lib.tsdf_hip_reintegrate_stats(vol._h, None) == capi.E_INVALID
    assert (n[0], n[1]) == (7, 9)
    same_planes(vol.download(), before, "null arguments")
    # poses that are not finite: both, then new (a plain removal), then old (a plain integrate)
    bad_o, bad_n = To.copy(), Tn.copy()
    bad_o[5] = np.nan
    bad_n[2] = np.inf
    assert raw_call(vol, dep, col, bad_o, po, bad_n, pn, n) == capi.OK and (n[0], n[1]) == (0, 0)
    assert vol.reintegrateStats() == (0, 0, 0, 0, 0, 0)
    assert raw_call(vol, dep, col, bad_o, po, bad_n, pn, None) == capi.OK
    same_planes(vol.download(), before, "two poses that are not finite")
    tr = fr[1][0]
    new = rc.correction(sc.size) @ tr
    assert raw_call(vol, dep, col, To, po, bad_n, pn, n) == capi.OK
    st = rc.reintegrate_frame(ov, dep, col, tr, None)
    assert (n[0], n[1]) == (st[1], 0) and vol.reintegrateStats()[:5] == st and st[1] > 500
    compare(vol, ov, "new pose not finite: a removal")
    assert raw_call(vol, dep, col, bad_o, po, Tn, pn, n) == capi.OK
    st = rc.reintegrate_frame(ov, dep, col, None, new)
    assert (n[0], n[1]) == (0, st[3]) and vol.reintegrateStats()[:5] == st and st[3] > 500
    compare(vol, ov, "old pose not finite: an integrate")
    vol.close()


# ---- 7. frame pairing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_a_held_back_frame_is_launched_before_it_is_reposed(gpu, color):
    """Frame pairing on: B is committed and waits for a partner; re-posing that same B first launches it."""
    vol, sc = dc.volume("32", color=color, layout=PACKED)
    vol.reset()
    fr = dc.abc(sc, "outside")
    new = rc.correction(sc.size) @ fr[1][0]
    ov = OracleVolume(vol._p)
    integrate(vol, fr[0])
    oracle_integrate(ov, fr[0])
    vol.setFramePairing(True)
    integrate(vol, fr[1], pipelined=True)
    n_b = oracle_integrate(ov, fr[1])
    n = repose(vol, fr[1], new)
    st = model_repose(ov, fr[1], new)
    assert n == (st[1], st[3]) and st[0] == st[1] == n_b
    compare(vol, ov, "commit B, re-pose B")
    vol.setFramePairing(False)
    vol.close()


# ---- 8. slab handles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,cut", [("32", 13), ("40x24x36", 13)])
def test_two_slab_handles_against_one_whole_handle(gpu, grid, cut):
    """setZSlab(0, 13, halo 1) and setZSlab(13, nz, halo 1): runs of 13 and 19 (or 23) planes, starting at plane 13 -- the z
    loop's tail and an unaligned start.  The two parts are the whole handle's planes, and the model's."""
    fr, new, ov, st = abc_model(grid, "rolled", True, 0)
    nz = dc.GRIDS[grid][2]
    parts, counts = [], np.zeros(2, np.int64)
    for zb, ze in ((0, cut), (cut, nz)):
        vol, _ = dc.volume(grid, color=True, layout=PACKED)
        vol.setZSlab(zb, ze, halo=1)
        vol.reset()
        for f in fr:
            integrate(vol, f)
        counts += repose(vol, fr[1], new)
        parts.append(vol.download())
        vol.close()
    whole, _ = dc.volume(grid, color=True, layout=PACKED)
    whole.reset()
    for f in fr:
        integrate(whole, f)
    assert repose(whole, fr[1], new) == tuple(counts) == (st[1], st[3])
    got = whole.download()
    whole.close()
    halves = tuple(np.concatenate([a[k], b[k]]) for k in range(3) for a, b in [parts])
    same_planes(halves, got, "two slabs against the whole handle")
    same_planes(got, (ov.d, ov.w, ov.rgb), "the whole handle against the model")


# ---- 9. the device-pointer entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_the_device_entry_equals_the_host_entry(gpu, color):
    fr, new, ov, st = abc_model("40x24x36", "inside", color, 0)
    outs = []
    for device in (False, True):
        vol, _ = dc.volume("40x24x36", color=color, layout=PACKED)
        vol.reset()
        for f in fr:
            integrate(vol, f)
        tr, dep, col = fr[1]
        if device:
            t = torch.empty((2, dc.H, dc.W), dtype=torch.float32, device="cuda")
            t[0].copy_(torch.from_numpy(dep))
            if color:
                t[1].view(torch.uint8).view(dc.H, dc.W, 4).copy_(torch.from_numpy(col))
            torch.cuda.synchronize()
            ptrs = (t[0].data_ptr(), t[1].data_ptr() if color else 0)
            assert vol.reintegrateCloudDevice(*ptrs, tr, new) is True   # asynchronous
            vol.synchronize()
            assert vol.reintegrateStats()[5] >= 0
            outs.append(compare(vol, ov, "device entry, not counting"))
            # ... and back, counting: the model of the way back is the model of any re-pose
            back = OracleVolume(vol._p)
            back.d[...], back.w[...] = ov.d, ov.w
            if color:
                back.rgb[...] = ov.rgb
            want = rc.reintegrate_frame(back, dep, col, new, tr)
            assert vol.reintegrateCloudDevice(*ptrs, new, tr, count=True) == (want[1], want[3])
            assert vol.reintegrateStats()[:5] == want
            compare(vol, back, "device entry, counting, the way back")
        else:
            assert repose(vol, fr[1], new) == (st[1], st[3])
            outs.append(compare(vol, ov, "host entry"))
        vol.close()
    same_planes(outs[0], outs[1], "device against host")


# ---- 10. random sequences -----------------------------------------------------------------------------------------------------
SHIFTS = [(1, 0, 0), (0, -1, 0), (0, 0, 2), (-3, 1, 0), (2, 0, -1)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_sequences(gpu, seed):
    """20 steps of integrate / re-pose / remove / shift / reconstruct / occupied / download on PACKED + colour (max_weight 4:
    counts saturate) against ReposeModel.  A re-posed frame is one of those integrated so far, posed through the shifts
    since, and is tracked afterwards under its new pose; now and then it is a stranger."""
    rng = np.random.RandomState(4200 + seed)
    vol, sc = dc.volume("32", color=True, layout=PACKED, max_weight=4.0, trunc=(0.012, 0.012))
    vol.reset()
    model = rc.ReposeModel(vol._p, cull=True)
    fix = [rc.correction(sc.size), np.linalg.inv(rc.correction(sc.size))]
    inside, n_frames, tally = [], 0, {}
    for step in range(20):
        op = ["integrate", "integrate", "repose", "repose", "repose", "remove", "shift", "mesh", "occupied", "download"][rng.randint(10)]
        if op in ("repose", "remove") and not inside:
            op = "integrate"
        what = f"seed {seed} step {step} {op}"
        tally[op] = tally.get(op, 0) + 1
        if op == "integrate":
            kind = dc.KINDS[rng.randint(3)]
            tr = dc.pose(kind, sc.size, int(rng.randint(2)))
            dep, col = dc.frame(sc, n_frames, tr)
            n_frames += 1
            T = model.pose(tr)
            assert vol.integrateCloud(dep, col, T, count=True) == model.integrate(dep, col, T), what
            inside.append((tr, dep, col))
        elif op == "repose":
            if rng.rand() < 0.25:
                tr = dc.pose("rolled", sc.size, 1)
                dep, col = dc.frame(sc, 50 + step, tr)
            else:
                tr, dep, col = inside.pop(rng.randint(len(inside)))
            new = fix[rng.randint(2)] @ tr
            To, Tn = model.pose(tr), model.pose(new)
            n = vol.reintegrateCloud(dep, col, To, Tn, count=True)
            st = model.reintegrate(dep, col, To, Tn)
            assert n == (st[1], st[3]) and vol.reintegrateStats()[:5] == st, (what, n, st)
            inside.append((new, dep, col))
        elif op == "remove":
            tr, dep, col = inside.pop(rng.randint(len(inside)))
            T = model.pose(tr)
            n = vol.deintegrateCloud(dep, col, T, count=True)
            st = model.deintegrate(dep, col, T)
            assert n == st[1], (what, n, st)
        elif op == "shift":
            s = SHIFTS[rng.randint(len(SHIFTS))]
            model.shift(s, vol.shiftVolume(*s))
        elif op == "mesh":
            w_min = float(rng.choice([0.0, 1.0, 2.0]))
            mesh, _ = march(vol, True, w_min)
            assert_same_mesh(mesh, model.mesh(w_min), what)
        elif op == "occupied":
            check_occupied(vol, model.occupied(), what=what)
        compare(vol, model.ov, what)
    print(f"seed {seed}: {tally}")
    assert tally.get("repose", 0) >= 2, tally
    vol.close()
