"""GPU tier: alignCloud -- tsdf_hip_align_system / tsdf_hip_align against a numpy restatement (tests/align_cases.py) whose
value and gradient are the ORACLE's (OracleVolume.sample), whose gate is restated from download(), the Python mirror's
getVoxelIndex / getVoxelCenter and the declared rule, and whose sums are numpy's in float64.

Bounds (derived, not tuned): the transform and the gate are exact (bits, bytes); each of the 29 sums is within
(n_used + 8) * 2^-53 * sum |term| of numpy's -- the worst case of re-ordered fp64 summation of terms that each carry a
handful of roundings -- and the count is exact; the driver's pose follows its restatement within
10 * cond(A) * (n_used + 8) * 2^-53 per iteration, accumulated."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import AlignmentError, backproject
from oracle.oracle import OracleVolume
from tests import align_cases as ac
from tests.common import assert_same_f32, frames, make_volume

pytestmark = pytest.mark.gpu
F64P = C.POINTER(C.c_double)
LAYOUTS = ["packed", "packed_colour", "f32w"]
SIZES = [1, 63, 257, 70001]   # 70 001 > 256 * 256: the grid-stride loop makes a second trip and the last block is ragged
N_POOL = max(SIZES)


def _configured(res, layout, size=None):
    vol, sc = make_volume(res, color=(layout == "packed_colour"), size=size)
    if layout == "f32w":
        vol.setLayout(capi.LAYOUT_F32W)
    vol.reset()
    assert vol.getLayout() == (capi.LAYOUT_F32W if layout == "f32w" else capi.LAYOUT_PACKED)
    return vol, sc


def _pool(rng, sc, T, frame_pts):
    """N_POOL source points: a frame's back-projection, points spread over (and a little beyond) the volume, and one of
    every special kind, shuffled."""
    inv = np.linalg.inv(T)
    S = sc.size
    box = rng.uniform(-0.56, 0.56, (N_POOL, 3)) * S
    voxel = S / 64
    special_vol = np.array([[0.49 * S, 0.0, 0.0], [0.0, 0.5 * S - 0.2 * voxel, 0.01], [0.01, 0.0, 0.5 * S - 0.2 * voxel], [3 * S, 0.0, 0.0],
                            [0.0, -2 * S, 0.0]])
    src = lambda v: (v @ inv[:3, :3].T + inv[:3, 3])  # noqa: E731
    pts = np.concatenate([frame_pts.astype(np.float64), src(special_vol), src(box)])[:N_POOL - 3]
    pts = np.concatenate([pts, [[np.nan, 0.0, 0.1], [0.0, np.nan, 0.1], [0.0, 0.0, np.nan]]]).astype(np.float32)
    order = np.concatenate([[0], 1 + rng.permutation(len(pts) - 1)])
    return np.ascontiguousarray(pts[order])


def _generic_pose(base):
    """A pose with no exactly representable entry."""
    T = ac.se3_exp([0.011, -0.023, 0.017, 0.0013, -0.0021, 0.0007]) @ base
    assert np.all(T[:3, :4] != T[:3, :4].astype(np.float32)), "an entry of the test pose is a float"
    return T


class Case:
    def finish(self, vol):
        """Put a point that is used first (n = 1 then sums something) and restate both min_weight values once."""
        j = int(np.argmax(ac.restate(vol, self.ov, self.w, self.pts, self.T, 2.0, self.r_max)["used"]))
        self.pts[[0, j]] = self.pts[[j, 0]]
        self.want = {mw: ac.restate(vol, self.ov, self.w, self.pts, self.T, mw, self.r_max) for mw in (0.0, 2.0)}


@pytest.fixture(scope="module")
def fused64(gpu):
    """64^3, 160 x 120, six frames fused into every layout and into the oracle; one shared restatement per min_weight."""
    c = Case()
    c.vols = {}
    for layout in LAYOUTS:
        vol, sc = _configured(64, layout)
        c.vols[layout] = vol
    ov = OracleVolume(c.vols["packed_colour"]._p)
    for i, tr, dep, col in frames(sc, 6, 8):
        for layout, vol in c.vols.items():
            vol.integrateCloud(dep, col if layout == "packed_colour" else None, tr)
        ov.integrate(dep, col, synth.cam_from_vol_f32(tr))
    for layout, vol in c.vols.items():
        d, w, _ = vol.download()
        assert np.array_equal(d.view(np.uint32), ov.d.view(np.uint32)) and np.array_equal(w, ov.w), layout
    c.ov, c.sc, c.w = ov, sc, ov.w
    cam = synth.turntable_pose(1.3, 8, sc.size, tilt=0.2)
    c.T = _generic_pose(cam)
    c.pts = _pool(np.random.RandomState(7), sc, c.T, backproject(sc.depth(cam), sc.fx, sc.fy, sc.cx, sc.cy))
    c.r_max = 0.9
    c.finish(c.vols["packed"])
    yield c
    for vol in c.vols.values():
        vol.close()


@pytest.fixture(scope="module")
def random100(gpu):
    """100^3 of edge 0.39 m (closed-form, non-dyadic centres), smooth-plus-noise distances, ~30 % of the voxels w = 0,
    uploaded as tests/test_query_gpu.py::test_raycast_and_sampling_on_a_random_volume does."""
    c = Case()
    c.vols = {}
    res = 100
    rng = np.random.RandomState(99)
    for layout in LAYOUTS:
        vol, sc = _configured(res, layout, size=0.39)
        c.vols[layout] = vol
    ov = OracleVolume(c.vols["packed"]._p)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, res)] * 3, indexing="ij")
    ov.d[:] = np.clip(0.9 * np.sin(3 * x + 1) * np.cos(2 * y) + 0.5 * z + rng.normal(0, 0.15, ov.d.shape), -1, 1).astype(np.float32)
    ov.w[:] = np.where(rng.rand(*ov.w.shape) < 0.3, 0, np.where(rng.rand(*ov.w.shape) < 0.15, rng.randint(1, 3, ov.w.shape),
                                                            rng.randint(3, 6, ov.w.shape))).astype(np.float32)
    rgb = rng.randint(0, 256, ov.d.shape + (3,)).astype(np.uint8)
    for layout, vol in c.vols.items():
        vol.upload(ov.d, ov.w, rgb if layout == "packed_colour" else None)
    c.ov, c.sc, c.w = ov, sc, ov.w
    c.T = _generic_pose(synth.look_at_pose((0.05, -0.02, -0.1), target=(0.01, 0.0, 0.2)))
    inv = np.linalg.inv(c.T)
    dense = rng.uniform(-0.3, 0.3, (4000, 3)) * sc.size   # well inside: with 70 % observed voxels 0.7^8 of them pass the weights
    c.pts = _pool(rng, sc, c.T, (dense @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    c.r_max = 0.6
    c.finish(c.vols["packed"])
    yield c
    for vol in c.vols.values():
        vol.close()


@pytest.fixture(scope="module", params=["fused64", "random100"])
def case(request):
    return request.getfixturevalue(request.param)


def _sub(want, n):
    """The restatement of the first n points from the one computed for the pool."""
    used = want["used"][:n]
    k = int(want["used"][:n].sum())
    t = want["terms"][:k]
    return dict(q=want["q"][:n], used=used, out=t.sum(0), abs_sum=np.abs(t).sum(0))


def test_the_inputs_contain_every_reason_for_rejection(case):
    w0, w2 = case.want[0.0], case.want[2.0]
    finite = np.isfinite(w0["q"]).all(1)
    assert (finite & ~w0["exists"]).sum() >= 1, "outside the grid"
    assert (w0["exists"] & ~w0["ok"]).sum() >= 1, "in the last cell of an axis"
    assert (~finite).sum() >= 3, "NaN"
    assert (w0["ok"] & ~w0["all_w"]).sum() >= 1, "a neighbour with w = 0"
    assert (w0["all_w"] & ~w0["used"]).sum() >= 1, "|val| >= r_max"
    assert (w0["used"] & ~w2["used"]).sum() >= 1, "min_weight = 2 excludes points that 0 keeps"
    assert w2["used"].sum() >= 50 and w0["used"][0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_transform_gate_system_and_repeatability(case, layout, n):
    vol, pts = case.vols[layout], case.pts[:n]
    for mw in (0.0, 2.0):
        want = _sub(case.want[mw], n)
        out, used, q = vol.alignmentSystem(pts, case.T, mw, case.r_max, want_used=True, want_points=True)
        what = f"{layout}, n = {n}, min_weight = {mw}"
        assert_same_f32(q, want["q"], "xyz_vol, " + what)                                   # 1. transform
        assert used.dtype == bool and np.array_equal(used, want["used"]), what             # 2. gate
        ac.assert_system(out, want, what)                                                   # 3. system
        again = vol.alignmentSystem(pts, case.T, mw, case.r_max)                            # 5. repeatability
        assert again.tobytes() == out.tobytes(), what
    import torch
    d_pts = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    dev = np.empty(29)
    capi.check(capi.load().tsdf_hip_align_system_device(vol._need(), d_pts.data_ptr(), n, np.ascontiguousarray(case.T[:3]).ctypes.data_as(F64P),
                                                        2.0, case.r_max, dev.ctypes.data_as(F64P)), "align_system_device")
    assert dev.tobytes() == out.tobytes(), "host-pointer and device form differ"
    st = (C.c_uint64 * 4)()
    capi.check(capi.load().tsdf_hip_align_stats(vol._need(), st), "align_stats")
    assert [int(st[0]), int(st[1]), int(st[2])] == [n, int(out[28]), 0]


def test_multi_gpu_set_sums_the_same_points(fused64):
    c = fused64
    vol, sc = make_volume(64)
    vol.setDevices([0, 0, 0])
    vol.reset()
    for i, tr, dep, col in frames(sc, 6, 8):
        vol.integrateCloud(dep, None, tr)
    assert capi.load().tsdf_hip_slab_count(vol._need()) == 3
    for n in (257, N_POOL):
        want = _sub(c.want[0.0], n)
        out, used, q = vol.alignmentSystem(c.pts[:n], c.T, 0.0, c.r_max, want_used=True, want_points=True)
        one = c.vols["packed"].alignmentSystem(c.pts[:n], c.T, 0.0, c.r_max, want_used=True)[1]
        assert np.array_equal(used, one) and np.array_equal(used, want["used"])
        assert_same_f32(q, want["q"], "xyz_vol of a set")
        ac.assert_system(out, want, f"three slabs, n = {n}")
    dev = np.empty(29)
    rc = capi.load().tsdf_hip_align_system_device(vol._need(), 1 << 20, 4, np.ascontiguousarray(c.T[:3]).ctypes.data_as(F64P), 0.0, 0.9,
                                                  dev.ctypes.data_as(F64P))
    assert rc == capi.E_UNSUPPORTED
    vol.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arc64(gpu):
    """Test 8's scene: eight poses of a 64-pose turntable fused at 64^3, the frame from between two of them."""
    c = Case()
    c.vol, c.sc = _configured(64, "packed")
    c.ov = OracleVolume(c.vol._p)
    for tr in ac.align_poses(c.sc):
        dep = c.sc.depth(tr)
        c.vol.integrateCloud(dep, None, tr)
        c.ov.integrate(dep, None, synth.cam_from_vol_f32(tr))
    c.cloud, c.T_star, c.starts = ac.align_case(c.vol, c.sc)
    yield c
    c.vol.close()


def test_driver_follows_its_restatement(arc64):
    c = arc64
    K = 8
    poses, conds, counts, log = ac.gauss_newton(c.vol, c.ov, c.ov.w, c.cloud, c.starts["large"], K, 0.0, 0.9)
    tol = np.cumsum([10 * cond * (n + 8) * ac.EPS for cond, n in zip(conds, counts)])
    for k in (1, K):
        T, it, cost = c.vol.alignCloud(c.cloud, c.starts["large"], max_iterations=k, min_step=0.0)
        assert it == k and cost.shape == (k, 2)
        err = np.abs(T[:3] - poses[k - 1][:3]).max()
        print(f"after {k} steps: max pose difference {err:.3e}, bound {tol[k - 1]:.3e}, cond(A) {conds[k - 1]:.1f}, used {counts[k - 1]}")
        assert err <= tol[k - 1], (k, err, tol[k - 1])
        assert np.array_equal(cost[:, 1], log[:k, 1])
        assert np.all(np.abs(cost[:, 0] - log[:k, 0]) <= 1e-9 * log[:k, 0])
        assert np.array_equal(T[3], [0, 0, 0, 1])
    st = (C.c_uint64 * 4)()
    capi.check(capi.load().tsdf_hip_align_stats(c.vol._need(), st), "align_stats")
    assert [int(st[0]), int(st[1]), int(st[2])] == [len(c.cloud), counts[K - 1], K]


def test_it_aligns(arc64):
    c = arc64
    start = ac.pose_error(c.starts["large"], c.T_star)
    TL, itL, costL = c.vol.alignCloud(c.cloud, c.starts["large"], max_iterations=8, min_step=0.0)
    TS, itS, costS = c.vol.alignCloud(c.cloud, c.starts["small"], max_iterations=8, min_step=0.0)
    end = ac.pose_error(TL, c.T_star)
    per_point = costL[:, 0] / costL[:, 1]
    print(f"start {start[0] * 1e3:.2f} mm {start[1]:.4f} rad, end {end[0] * 1e3:.2f} mm {end[1]:.4f} rad, cost per point "
          f"{per_point[0]:.4f} -> {per_point[-1]:.4f}")
    assert end[0] < start[0] and end[1] < start[1]
    assert per_point[-1] < per_point[0] / 5
    apart = ac.pose_error(TL, TS)
    print(f"the two starts end {apart[0]:.2e} m, {apart[1]:.2e} rad apart")
    assert apart[0] < 1e-4 and apart[1] < 1e-4
    # min_step stops it early, at the same poses
    T3, it3, cost3 = c.vol.alignCloud(c.cloud, c.starts["large"], max_iterations=8, min_step=1e-3)
    assert 1 <= it3 < 8 and len(cost3) == it3
    T3b, _, _ = c.vol.alignCloud(c.cloud, c.starts["large"], max_iterations=it3, min_step=0.0)
    assert np.array_equal(T3, T3b)


def test_refusals_and_the_two_statuses(arc64):
    c = arc64
    lib, h = capi.load(), c.vol._need()
    pts = np.ascontiguousarray(c.cloud[:500])
    T = np.ascontiguousarray(c.starts["small"][:3]).reshape(12)
    out, ref = np.full(29, 7.0), np.full(12, 7.0)
    it = C.c_int32(7)
    xp, tp, op, rp = capi.as_f32p(pts), T.ctypes.data_as(F64P), out.ctypes.data_as(F64P), ref.ctypes.data_as(F64P)
    nan = float("nan")
    for args in [(h, xp, 0, tp, 0.0, 0.9, op, None, None), (h, None, 500, tp, 0.0, 0.9, op, None, None), (h, xp, 500, None, 0.0, 0.9, op, None, None),
                 (h, xp, 500, tp, 0.0, 0.9, None, None, None), (h, xp, 500, tp, 0.0, 0.0, op, None, None), (h, xp, 500, tp, 0.0, -1.0, op, None, None),
                 (h, xp, 500, tp, 0.0, nan, op, None, None), (h, xp, 500, tp, nan, 0.9, op, None, None)]:
        assert lib.tsdf_hip_align_system(*args) == capi.E_INVALID, args[2:6]
    assert lib.tsdf_hip_align_system_device(h, None, 500, tp, 0.0, 0.9, op) == capi.E_INVALID
    assert lib.tsdf_hip_align_system_device(h, 1 << 20, 0, tp, 0.0, 0.9, op) == capi.E_INVALID
    for args in [(h, xp, 0, tp, 0.0, 0.9, 8, 0.0, rp, C.byref(it), None), (h, None, 500, tp, 0.0, 0.9, 8, 0.0, rp, C.byref(it), None),
                 (h, xp, 500, None, 0.0, 0.9, 8, 0.0, rp, C.byref(it), None), (h, xp, 500, tp, 0.0, 0.9, 8, 0.0, None, C.byref(it), None),
                 (h, xp, 500, tp, 0.0, 0.0, 8, 0.0, rp, C.byref(it), None), (h, xp, 500, tp, 0.0, 0.9, 0, 0.0, rp, C.byref(it), None),
                 (h, xp, 500, tp, 0.0, 0.9, 8, -1.0, rp, C.byref(it), None), (h, xp, 500, tp, 0.0, 0.9, 8, nan, rp, C.byref(it), None)]:
        assert lib.tsdf_hip_align(*args) == capi.E_INVALID, args[2:8]
    assert np.all(out == 7.0) and np.all(ref == 7.0) and it.value == 7
    # a cloud entirely outside the volume: "no point used", refined == guess
    far = np.ascontiguousarray(pts + np.float32(50.0))
    log = np.full(16, -1.0)
    rc = lib.tsdf_hip_align(h, capi.as_f32p(far), 500, tp, 0.0, 0.9, 8, 0.0, rp, C.byref(it), log.ctypes.data_as(F64P))
    assert rc == capi.ALIGN_NO_POINTS and it.value == 0 and np.array_equal(ref, T)
    assert log[0] == 0.0 and log[1] == 0.0 and np.all(log[2:] == -1.0)
    with pytest.raises(AlignmentError) as e:
        c.vol.alignCloud(far, c.starts["small"])
    assert e.value.code == capi.ALIGN_NO_POINTS and e.value.iterations == 0 and np.array_equal(e.value.refined, c.starts["small"])
    # a cloud on one wall only -- an exactly planar field z = const: rotation about z and translation along x, y are free
    vol, sc = _configured(64, "packed")
    zc = np.array([vol.getVoxelCenter(0, 0, k)[2] for k in range(64)], np.float64)
    d = np.clip((zc - 0.01) / 0.03, -1, 1).astype(np.float32)[:, None, None] * np.ones((64, 64, 64), np.float32)
    vol.upload(np.ascontiguousarray(d), np.ones((64, 64, 64), np.float32))
    rng = np.random.RandomState(2)
    wall = np.ascontiguousarray(np.concatenate([rng.uniform(-0.1, 0.1, (400, 2)), np.full((400, 1), 0.013)], 1), dtype=np.float32)
    G = np.ascontiguousarray(np.eye(4)[:3]).reshape(12)
    ref[:] = 7.0
    rc = lib.tsdf_hip_align(vol._need(), capi.as_f32p(wall), 400, G.ctypes.data_as(F64P), 0.0, 0.9, 8, 0.0, rp, C.byref(it), None)
    assert rc == capi.ALIGN_RANK_DEFICIENT and it.value == 0 and np.array_equal(ref, G)
    sysm = vol.alignmentSystem(wall, np.eye(4))
    assert sysm[28] == 400 and sysm[27] > 0       # ... though every point was used
    with pytest.raises(AlignmentError) as e:
        vol.alignCloud(wall, np.eye(4))
    assert e.value.code == capi.ALIGN_RANK_DEFICIENT
    vol.close()
    # the Python front end applies sample()'s rule to a non-cubic grid
    flat, _ = make_volume(64, res3=(64, 64, 32), size3=(0.25, 0.25, 0.125))
    flat.strict_noncubic = True
    flat.reset()
    with pytest.raises(ValueError):
        flat.alignmentSystem(pts, c.starts["small"])
    with pytest.raises(ValueError):
        flat.alignCloud(pts, c.starts["small"])
    flat.close()
