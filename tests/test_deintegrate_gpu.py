"""GPU tier: tsdf_hip_deintegrate (cpu_tsdf_amd/csrc/tsdf_deintegrate.hip) -- a frame taken back out of the volume.  Every
expectation is the host model of tests/deintegrate_cases.py (the frame integrated into a fresh oracle volume selects the
voxels and supplies d_new and the colour; then the rule in float32, one operation at a time), compared BIT FOR BIT with
download() on d, w and rgb.  The "band seen" flags are checked through what their readers do afterwards: the fast
integrate kernels' implied distances and marching cubes' skips."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection time, before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests import deintegrate_cases as dc
from tests import pose_cases
from tests.common import assert_same_f32
from tests.sequence_model import assert_same_mesh, compare
from tests.sequence_util import march, read_detail
from tests.test_occupied_gpu import check as check_occupied

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


def deintegrate(vol, fr, count=True):
    tr, dep, col = fr
    return vol.deintegrateCloud(dep, col if vol._p.integrate_color else None, tr, count=count)


def same_planes(got, want, what):
    assert_same_f32(got[0], want[0], what + ": d")
    assert_same_f32(got[1], want[1], what + ": w")
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]), what + ": rgb"


def raw_call(vol, dep, col, T, n=None, device=False):
    """The C entry point itself: its return code."""
    lib = capi.load()
    Tp = None if T is None else capi.as_f32p(np.ascontiguousarray(T, np.float32))
    dp = None if dep is None else capi.as_f32p(dep)
    cp = None if col is None else capi.as_u8p(col)
    return lib.tsdf_hip_deintegrate(vol._h, dp, cp, Tp, n)


_MODELS = {}


def abc_model(grid, kind, color, order):
    """Frames A, B, C of `kind` on `grid`, and the model after A, B, C, remove B with its counts.  Shared, never modified."""
    key = (grid, kind, color, order)
    if key not in _MODELS:
        vol, sc = dc.volume(grid, color=color, order=order)
        fr = dc.abc(sc, kind)
        ov = OracleVolume(vol._p)
        counts = [oracle_integrate(ov, f) for f in fr]
        nans, beyond = dc.frame_facts(vol._p, fr[1][1], fr[1][2], fr[1][0])
        assert nans > 10 and beyond > 100, (key, nans, beyond)   # the frames hold NaN pixels and voxels beyond the truncation distance
        st = dc.remove_frame(ov, fr[1][1], fr[1][2], fr[1][0])
        assert st[0] == counts[1] and st[1] > 500
        _MODELS[key] = (fr, ov, st)
    return _MODELS[key]


# ---- 1. A, B, C, remove B: every layout, colour setting, transform order, grid and pose --------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_b_c_remove_b_equals_the_model(gpu, layout, color, order):
    for grid in dc.GRIDS:
        for kind in dc.KINDS:
            fr, ov, st = abc_model(grid, kind, color, order)
            vol, _ = dc.volume(grid, color=color, order=order, layout=LAYOUTS[layout])
            vol.reset()
            assert vol.getLayout() == LAYOUTS[layout]
            for f in fr:
                integrate(vol, f)
            n = deintegrate(vol, fr[1])
            what = f"{grid} {kind} {layout} colour {color} order {order}"
            compare(vol, ov, what)
            got = vol.deintegrateStats()
            print(what, "stats", got, "model", st)
            assert n == st[1] and got[:3] == st, (what, n, got, st)
            vol.close()


# ---- 2. saturation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_saturated_voxels_lose_one_count(gpu, color):
    """max_weight = 2, four frames from one pose, one removed: every observed voxel sits at the limit and goes to 1 --
    PACKED (k' = k - 1) and F32W (w' = ceil(w) - 1) agree with the model and with each other."""
    outs = []
    for layout in (PACKED, F32W):
        vol, sc = dc.volume("32", color=color, layout=layout, max_weight=2.0)
        vol.reset()
        tr = dc.pose("outside", sc.size)
        fr = [(tr,) + dc.frame(sc, i, tr) for i in range(4)]
        ov = OracleVolume(vol._p)
        for f in fr:
            integrate(vol, f)
            oracle_integrate(ov, f)
        assert (ov.w == 2).sum() > 500
        n = deintegrate(vol, fr[2])
        st = dc.remove_frame(ov, fr[2][1], fr[2][2], fr[2][0])
        assert n == st[1] and st[2] < st[1]
        assert ov.w.max() == 2 and (ov.w == 1).sum() > 500   # (the NaN comb moves: some voxels were seen by three frames only)
        outs.append(compare(vol, ov, f"max_weight 2, layout {layout}"))
        vol.close()
    same_planes(outs[0], outs[1], "PACKED against F32W")


def test_a_non_integer_weight_limit_on_f32w(gpu):
    """max_weight = 2.5 (F32W): a voxel at 2.5 has W = ceil(2.5) = 3 and goes to 2."""
    vol, sc = dc.volume("32", color=True, layout=F32W, max_weight=2.5)
    vol.reset()
    tr = dc.pose("rolled", sc.size)
    fr = [(tr,) + dc.frame(sc, i, tr) for i in range(4)]
    ov = OracleVolume(vol._p)
    for f in fr:
        integrate(vol, f)
        oracle_integrate(ov, f)
    assert (ov.w == 2.5).sum() > 500
    n = deintegrate(vol, fr[0])
    st = dc.remove_frame(ov, fr[0][1], fr[0][2], fr[0][0])
    assert n == st[1] and (ov.w == 2).sum() > 500
    compare(vol, ov, "max_weight 2.5")
    integrate(vol, fr[1])   # ... and back up through the fast kernel: 2 -> 3 -> clamped to 2.5
    oracle_integrate(ov, fr[1])
    compare(vol, ov, "max_weight 2.5, one more frame")
    vol.close()


# ---- 3. A, then remove A ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_then_remove_a_equals_a_fresh_handle(gpu, layout, color):
    for grid in dc.GRIDS:
        for kind in dc.KINDS:
            vol, sc = dc.volume(grid, color=color, layout=LAYOUTS[layout])
            fresh, _ = dc.volume(grid, color=color, layout=LAYOUTS[layout])
            vol.reset()
            fresh.reset()
            a = dc.abc(sc, kind)[1]
            n_obs = integrate(vol, a, count=True)
            assert n_obs > 500
            assert deintegrate(vol, a) == n_obs
            assert vol.deintegrateStats()[:3] == (n_obs, n_obs, n_obs)
            same_planes(vol.download(), fresh.download(), f"{grid} {kind} {layout}")
            vol.close()
            fresh.close()


# ---- 4. the flag rule ---------------------------------------------------------------------------------------------------------
def flag_case():
    """64^3, PACKED + colour, dc.RESTING_TRUNC under max_weight 3: the hinge value rests forward but not under the removal's
    division, the record stays at rest_state == 1, and most of the volume is free space in cells whose flag is 0."""
    vol, sc = dc.volume((64, 64, 64), color=True, layout=PACKED, max_weight=3.0, trunc=dc.RESTING_TRUNC)
    sc = synth.Scene(sc.size, sc.width, sc.height, box=0.6)   # the walls outside the grid: only the sphere is a surface
    model = dc.RemovalModel(vol._p, cull=True)
    return vol, sc, model


def test_removing_a_stranger_sets_the_flags_its_band_needs(gpu):
    """A frame that was never integrated -- a larger sphere, whose surface lies in what the volume holds as free space,
    in cells whose flag is 0 -- is removed: voxels there leave the hinge value.  The next integrate goes through the fast
    kernel with implied distances on; it may only rebuild distances from counts where the flags still allow it.  Planes
    equal the model; the mesh equals the oracle's march of the model."""
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
    resting = (model.ov.w == 3) & (model.ov.d == p)
    # cells (64 x 4 x 1: a whole row group of this grid) that hold no voxel off the hinge value: no launch so far can have set their flag
    off = (model.ov.w > 0) & (model.ov.d != p)
    quiet = ~np.repeat(off.reshape(64, 16, 4 * 64).any(axis=2), 4, axis=1)[:, :, None]
    stranger = synth.Scene(sc.size, sc.width, sc.height, sphere=0.36, box=0.6)
    tr = trs[1]
    dep, col = dc.frame(stranger, 7, tr)
    n = vol.deintegrateCloud(dep, col, tr, count=True)
    st = model.deintegrate(dep, col, tr)
    assert n == st[1] > 5000
    moved = resting & (model.ov.w == 2) & (model.ov.d != p)
    kept = resting & (model.ov.w == 2) & (model.ov.d == p)
    print(f"stranger: {n} weights lowered, {int(moved.sum())} resting voxels moved ({int((moved & quiet).sum())} in cells whose flag was 0), "
          f"{int(kept.sum())} kept the hinge value")
    assert moved.sum() > 500 and (moved & quiet).sum() > 100 and kept.sum() > 5000
    compare(vol, model.ov, "after the stranger left")
    tr = synth.turntable_pose(3, 8, sc.size)
    dep, col = dc.frame(sc, 3, tr)
    n = vol.integrateCloud(dep, col, tr, count=True)
    assert n == model.integrate(dep, col, tr)
    skipped, allowed = read_detail(vol)
    print(f"next frame: {skipped} of {n} observed voxels had their distance rebuilt from the count")
    assert allowed == 1 and skipped > 0, (skipped, n)   # the fast kernel, with distances rebuilt from counts
    compare(vol, model.ov, "one more frame through the fast kernel")
    mesh, st = march(vol, True)
    assert st[3] & 1 == 1 and len(mesh["cells"]) > 500
    assert_same_mesh(mesh, model.mesh(1.0), "mesh after the removal")
    check_occupied(vol, model.occupied(), what="occupied after the removal")
    vol.close()


def test_the_readers_keep_their_skips_after_a_removal(gpu):
    """A, B, C, remove B, D against A, C, D without a removal: the next integrate still rebuilds distances from counts
    (tsdf_hip_last_read_detail out[1] == 1) and marching cubes still reads less than the whole distance plane."""
    seen = []
    for removal in (True, False):
        vol, sc, model = flag_case()
        vol.reset()
        fr = [(tr,) + dc.frame(sc, i, tr) for i, tr in enumerate(synth.turntable_pose(i, 8, sc.size) for i in range(4))]
        for k in ((0, 1, 2) if removal else (0, 2)):
            integrate(vol, fr[k])
            model.integrate(fr[k][1], fr[k][2], fr[k][0])
        if removal:
            assert deintegrate(vol, fr[1]) == model.deintegrate(fr[1][1], fr[1][2], fr[1][0])[1]
            compare(vol, model.ov, "A, B, C, remove B")
        n = integrate(vol, fr[3], count=True)
        assert n == model.integrate(fr[3][1], fr[3][2], fr[3][0])
        skipped, allowed = read_detail(vol)
        mesh, st = march(vol, True)
        compare(vol, model.ov, f"removal {removal}")
        assert_same_mesh(mesh, model.mesh(1.0), f"removal {removal}")
        whole = 64 * 64 * 64 * 4
        print(f"removal {removal}: implied {skipped} of {n}, allowed {allowed}, march read {st[2]} of {whole} bytes, flags {st[3]}")
        seen.append((allowed, skipped > 0, st[3] & 1, st[2] < whole))
        vol.close()
    assert seen[1] == (1, True, 1, True), seen   # the sequence without the removal skips
    assert seen[0] == seen[1], seen              # ... and so does the one with it


# ---- 5. the reference's frustum cull ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_removal_selects_the_culled_set(gpu, layout):
    """A principal point 60 % off centre and a camera yawed so that the grid sits beside the optical axis: the reference's
    pyramid cuts voxels updateVoxel itself would accept (tests/test_integrate_poses_gpu.py).  The removal selects the
    culled set: A, B, C, remove B equals the model, and A then remove A a fresh volume."""
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
    n = deintegrate(vol, fr[1])
    st = dc.remove_frame(ov, fr[1][1], fr[1][2], fr[1][0], cull=True)
    assert n == st[1] and vol.deintegrateStats()[:3] == st
    loose = dc.observation(vol._p, fr[1][1], fr[1][2], fr[1][0], cull=False)[0]
    assert st[0] < int(loose.sum())
    compare(vol, ov, "culled A, B, C, remove B")
    vol.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_planes_alone(gpu):
    lib = capi.load()
    n = C.c_uint64(7)

    def refused(vol, fr, code, what):
        before = vol.download()
        tr, dep, col = fr
        assert raw_call(vol, dep, col, cfv(tr), C.byref(n)) == code, what
        assert n.value == 7, what
        same_planes(vol.download(), before, what)

    # the weightings (F32W; setWeighting takes effect at reset()), and the variance state once it has been allocated
    for by_depth, by_variance in ((True, False), (False, True)):
        vol, sc = dc.volume("32", color=True, layout=F32W)
        vol.setWeighting(by_depth=by_depth, by_variance=by_variance)
        vol.reset()
        fr = dc.abc(sc, "outside")
        integrate(vol, fr[0])
        refused(vol, fr[0], capi.E_UNSUPPORTED, f"weighting {by_depth} {by_variance}")
        if by_variance:
            capi.check(lib.tsdf_hip_set_weighting(vol._h, 0, 0), "set_weighting")   # the flag goes, M_ / nsample_ stay
            refused(vol, fr[0], capi.E_UNSUPPORTED, "variance state allocated")
        vol.close()
    # the two colour modes
    for mode in ("RGBNormalized", "LAB"):
        vol, sc = dc.volume("32", color=True)
        vol.setColorMode(mode)
        vol.reset()
        fr = dc.abc(sc, "outside")
        integrate(vol, fr[0])
        refused(vol, fr[0], capi.E_UNSUPPORTED, mode)
        vol.close()
    # a set
    vol, sc = dc.volume("32", color=True)
    vol.setDevices([0, 0])
    vol.reset()
    fr = dc.abc(sc, "outside")
    integrate(vol, fr[0])
    refused(vol, fr[0], capi.E_UNSUPPORTED, "devices [0, 0]")
    assert b"multi" in lib.tsdf_hip_last_error()
    vol.close()
    # null arguments, a missing colour image, a pose that is not finite
    vol, sc = dc.volume("32", color=True)
    vol.reset()
    fr = dc.abc(sc, "outside")
    tr, dep, col = fr[0]
    integrate(vol, fr[0])
    before = vol.download()
    assert raw_call(vol, None, col, cfv(tr), C.byref(n)) == capi.E_INVALID
    assert raw_call(vol, dep, col, None, C.byref(n)) == capi.E_INVALID
    assert raw_call(vol, dep, None, cfv(tr), C.byref(n)) == capi.E_INVALID
    assert lib.tsdf_hip_deintegrate_device(vol._h, None, None, capi.as_f32p(cfv(tr)), C.byref(n)) == capi.E_INVALID
    assert lib.tsdf_hip_deintegrate_stats(vol._h, None) == capi.E_INVALID
    assert n.value == 7
    T = cfv(tr).copy()
    T[5] = np.nan
    assert raw_call(vol, dep, col, T, C.byref(n)) == capi.OK and n.value == 0
    assert vol.deintegrateStats() == (0, 0, 0, 0)
    assert raw_call(vol, dep, col, T, None) == capi.OK
    same_planes(vol.download(), before, "null arguments and a NaN pose")
    vol.close()


# ---- 7. frame pairing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_a_held_back_frame_is_launched_before_it_is_removed(gpu, color):
    """Frame pairing on: B is committed and waits for a partner; removing that same B first launches it, and what is left
    is the state before the commit (weights exactly, d and colour as the model says)."""
    vol, sc = dc.volume("32", color=color, layout=PACKED)
    vol.reset()
    fr = dc.abc(sc, "outside")
    ov = OracleVolume(vol._p)
    integrate(vol, fr[0])
    oracle_integrate(ov, fr[0])
    w_before = ov.w.copy()
    vol.setFramePairing(True)
    integrate(vol, fr[1], pipelined=True)
    n_b = oracle_integrate(ov, fr[1])
    n = deintegrate(vol, fr[1])
    st = dc.remove_frame(ov, fr[1][1], fr[1][2], fr[1][0])
    assert n == n_b == st[1]
    d, w, _ = compare(vol, ov, "commit B, remove B")
    assert np.array_equal(w, w_before)
    vol.setFramePairing(False)
    vol.close()


# ---- 8. slab handles ---------------------------------------------------------------------------------------------------------
def test_two_slab_handles_against_one_whole_handle(gpu):
    """setZSlab(0, 16, halo 1) and setZSlab(16, 32, halo 1): the launch covers the planes each handle's integrate launches
    write, so the two halves are the whole handle's planes -- and the model's."""
    fr, ov, st = abc_model("32", "rolled", True, 0)
    parts, counts = [], 0
    for zb, ze in ((0, 16), (16, 32)):
        vol, _ = dc.volume("32", color=True, layout=PACKED)
        vol.setZSlab(zb, ze, halo=1)
        vol.reset()
        for f in fr:
            integrate(vol, f)
        counts += deintegrate(vol, fr[1])
        parts.append(vol.download())
        vol.close()
    whole, _ = dc.volume("32", color=True, layout=PACKED)
    whole.reset()
    for f in fr:
        integrate(whole, f)
    assert deintegrate(whole, fr[1]) == counts == st[1]
    got = whole.download()
    whole.close()
    halves = tuple(np.concatenate([a[k], b[k]]) for k in range(3) for a, b in [parts])
    same_planes(halves, got, "two slabs against the whole handle")
    same_planes(got, (ov.d, ov.w, ov.rgb), "the whole handle against the model")


# ---- 9. the device-pointer entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_the_device_entry_equals_the_host_entry(gpu, color):
    fr, ov, st = abc_model("40x24x36", "inside", color, 0)
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
            assert vol.deintegrateCloudDevice(t[0].data_ptr(), t[1].data_ptr() if color else 0, tr) is True   # asynchronous
            vol.synchronize()
            assert vol.deintegrateStats()[3] >= 0
            outs.append(compare(vol, ov, "device entry, not counting"))
            integrate(vol, fr[1])   # put B back and take it out again, counting
            assert vol.deintegrateCloudDevice(t[0].data_ptr(), t[1].data_ptr() if color else 0, tr, count=True) == st[1]
            assert vol.deintegrateStats()[:3] == st
        else:
            assert deintegrate(vol, fr[1]) == st[1]
            outs.append(compare(vol, ov, "host entry"))
        vol.close()
    same_planes(outs[0], outs[1], "device against host")


# ---- 10. random sequences -----------------------------------------------------------------------------------------------------
SHIFTS = [(1, 0, 0), (0, -1, 0), (0, 0, 2), (-3, 1, 0), (2, 0, -1)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_sequences(gpu, seed):
    """20 steps of integrate / remove / shift / reconstruct / occupied / download on PACKED + colour (max_weight 4: counts
    saturate) against RemovalModel.  A removed frame is one of those integrated so far, posed through the shifts since, or
    now and then a stranger."""
    rng = np.random.RandomState(4100 + seed)
    vol, sc = dc.volume("32", color=True, layout=PACKED, max_weight=4.0, trunc=(0.012, 0.012))
    vol.reset()
    model = dc.RemovalModel(vol._p, cull=True)
    inside, n_frames, tally = [], 0, {}
    for step in range(20):
        op = ["integrate", "integrate", "remove", "remove", "shift", "mesh", "occupied", "download"][rng.randint(8)]
        if op == "remove" and not inside:
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
        elif op == "remove":
            if rng.rand() < 0.25:
                tr = dc.pose("rolled", sc.size, 1)
                dep, col = dc.frame(sc, 50 + step, tr)
            else:
                tr, dep, col = inside.pop(rng.randint(len(inside)))
            T = model.pose(tr)
            n = vol.deintegrateCloud(dep, col, T, count=True)
            st = model.deintegrate(dep, col, T)
            assert n == st[1] and vol.deintegrateStats()[:3] == st, (what, n, st)
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
    vol.close()
