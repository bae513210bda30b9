"""CPU tier: the model of tests/sequence_model.py checked without the product.  Its shift + integrate composition against an
OracleVolume that integrates the same frame on arrays rolled beforehand by other means (np.roll and index masks, not
tests/shift_cases) -- also per colour mode and weighting, state planes included --, the pose rule against the geometry it
stands for, the in-place uploads, the record's shift rule, and a replay of every case of tests/test_mode_sequences_gpu.py
through the model alone: the conditions its inputs must meet (tests/mode_cases.CONDITIONS) and its tally of operations.  Last,
every case of tests/test_feature_sequences_gpu.py through its driver without a product, and the floors on its inputs."""
import collections

import numpy as np
import pytest

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests.common import assert_same_f32, make_volume
from tests import mode_cases
from tests.sequence_model import Model, clamp_shift, record_for

RES = 32


def rolled(a, s, fill):
    """out[z, y, x] = a[z + sz, y + sy, x + sx] or `fill`: np.roll, then everything that wrapped around is overwritten."""
    out = np.roll(a, (-s[2], -s[1], -s[0]), axis=(0, 1, 2))
    for axis, v in zip((2, 1, 0), s):
        n = a.shape[axis]
        idx = np.arange(n)
        wrapped = (idx + v < 0) | (idx + v >= n)
        sl = [slice(None)] * a.ndim
        sl[axis] = wrapped
        out[tuple(sl)] = fill
    return out


def fused_model(color):
    vol, sc = make_volume(RES, 80, 60, color=color)
    m = Model(vol._p)
    for i in range(3):
        tr = synth.turntable_pose(i, 8, sc.size)
        assert m.integrate(sc.depth(tr), sc.bgra(i) if color else None, m.pose(tr)) > 0
    return vol, sc, m


@pytest.mark.parametrize("color", [True, False])
@pytest.mark.parametrize("s", [(3, -2, 1), (0, 0, -12), (-33, 1, 0), (1, 0, 0)])
def test_shift_then_integrate_equals_integrate_on_rolled_arrays(color, s):
    vol, sc, m = fused_model(color)
    before = (m.ov.d.copy(), m.ov.w.copy(), m.ov.rgb.copy() if color else None)
    moved = np.array(s, np.float64) * sc.size / RES   # what shiftVolume returns: s * size / res
    m.shift(s, moved)
    c = clamp_shift(s, (RES,) * 3)
    want = OracleVolume(vol._p, adopt=(np.ascontiguousarray(rolled(before[0], c, np.float32(-1))),
                                       np.ascontiguousarray(rolled(before[1], c, np.float32(0))),
                                       np.ascontiguousarray(rolled(before[2], c, np.uint8(0))) if color else None))
    assert_same_f32(m.ov.d, want.d, f"rolled d, shift {s}")
    assert_same_f32(m.ov.w, want.w, f"rolled w, shift {s}")
    assert (m.ov.w > 0).sum() < (before[1] > 0).sum() or s == (1, 0, 0)
    tr = synth.turntable_pose(3, 8, sc.size)
    dep, col = sc.depth(tr), sc.bgra(3) if color else None
    posed = m.pose(tr)
    assert np.array_equal(posed[:3, :3], tr[:3, :3]) and np.array_equal(posed[:3, 3], tr[:3, 3] - moved)
    n = m.integrate(dep, col, posed)
    assert n == want.integrate(dep, col, synth.cam_from_vol_f32(posed))
    assert_same_f32(m.ov.d, want.d, "d after one more frame")
    assert_same_f32(m.ov.w, want.w, "w after one more frame")
    if color:
        assert np.array_equal(m.ov.rgb, want.rgb)
    g = np.eye(4)
    g[:3, 3] = moved
    assert np.array_equal(m.G, g)


def test_the_posed_camera_sees_every_surviving_voxel_where_it_was():
    """Voxel (x, y, z) after the shift is voxel (x + sx, y + sy, z + sz) before it: seen from Model.pose(trans) its centre
    has the camera coordinates the old voxel's centre had from `trans`."""
    vol, sc, m = fused_model(False)
    s = (3, -2, 5)
    ctr = [m.ov.centers(a).astype(np.float64) for a in range(3)]
    m.shift(s, np.array(s, np.float64) * sc.size / RES)
    tr = synth.turntable_pose(1, 8, sc.size, tilt=0.2)
    new_cam, old_cam = np.linalg.inv(m.pose(tr)), np.linalg.inv(tr)
    for x, y, z in [(0, 2, 0), (10, 20, 5), (28, 31, 26)]:
        new = new_cam @ np.array([ctr[0][x], ctr[1][y], ctr[2][z], 1.0])
        old = old_cam @ np.array([ctr[0][x + s[0]], ctr[1][y + s[1]], ctr[2][z + s[2]], 1.0])
        assert np.abs(new - old).max() < 1e-12
    verts = np.array([[ctr[0][4], ctr[1][5], ctr[2][6]]], np.float32)   # ... and reconstruct() puts it back where it was
    assert_same_f32(m.to_world(verts), np.array([[ctr[0][4 + s[0]], ctr[1][5 + s[1]], ctr[2][6 + s[2]]]], np.float32), "to_world")


def test_uploads_write_the_box_and_nothing_else():
    vol, sc, m = fused_model(True)
    d0, w0, rgb0 = m.ov.d.copy(), m.ov.w.copy(), m.ov.rgb.copy()
    box = (3, 5, 9, 20, 11, 4)
    d, w, rgb = (a.copy() for a in m.box(*box))
    m.upload(d=d - np.float32(0.25), x0=3, y0=5, z0=9)
    m.upload(w=w + 1, x0=3, y0=5, z0=9)
    sl = (slice(9, 13), slice(5, 16), slice(3, 23))
    assert_same_f32(m.ov.d[sl], d0[sl] - np.float32(0.25), "d in the box")
    assert_same_f32(m.ov.w[sl], w0[sl] + 1, "w in the box")
    outside = np.ones(d0.shape, bool)
    outside[sl] = False
    assert np.array_equal(m.ov.d[outside], d0[outside]) and np.array_equal(m.ov.w[outside], w0[outside])
    assert np.array_equal(m.ov.rgb, rgb0)
    idx, dd, ww, cc = m.occupied(box)
    assert len(idx) > 0 and (idx >= box[:3]).all() and (idx < np.add(box[:3], box[3:])).all()
    assert np.array_equal(dd, m.ov.d[idx[:, 2], idx[:, 1], idx[:, 0]]) and np.array_equal(cc, m.ov.rgb[idx[:, 2], idx[:, 1], idx[:, 0]])
    m.reset()
    assert (m.ov.d == -1).all() and not m.ov.w.any()


def test_a_shift_leaves_the_record_as_it_was():
    for packed, trunc, wmax, can in ((True, (0.03, 0.03), 100.0, True), (True, (0.01, 0.03), 100.0, False),
                                     (True, (0.03, 0.03), 2.5, False), (False, (0.03, 0.03), 4.0, False)):
        rec = record_for(packed, trunc, wmax)
        assert rec.can == can
        assert rec.fast_launch() == can
        state = dict(rec.__dict__)
        rec.shift()
        assert rec.__dict__ == state and rec.fast_launch() == can
        rec.foreign_write()
        rec.shift()
        assert not rec.flags_describe_planes and not rec.fast_launch()
    assert capi.LAYOUT_PACKED != capi.LAYOUT_F32W


# ---- the colour modes and the weightings ----------------------------------------------------------------------------------
MODE_VARIANTS = [("RGBNormalized", True), ("LAB", True), ("by_depth", True), ("by_depth", False), ("by_variance", True),
                 ("by_variance", False), ("by_depth+by_variance", True), ("by_depth+by_variance", False)]


def integrate_directly(ov, mode, dep, col, T):
    """The oracle form of a mode, called as tests/evidence/fuzz_product_colour_modes.oracle_step calls it (no cull)."""
    if mode == "RGBNormalized":
        return ov.integrate_rgbn(dep, col, T)
    if mode == "LAB":
        return ov.integrate_lab(dep, col, T)
    if "by_variance" in mode:
        return ov.integrate_variance(dep, col, T, "by_depth" in mode)
    return ov.integrate(dep, col, T, weight_by_depth=True)


def arrays_of(ov):
    out = {"d": ov.d, "w": ov.w}
    if ov.rgb is not None:
        out["rgb"] = ov.rgb
    for k in range(len(getattr(ov, "cn", ()))):
        out[f"cn[{k}]"] = ov.cn[k]
    if getattr(ov, "M", None) is not None:
        out["M"], out["nsample"] = ov.M, ov.nsample
    return out


def assert_same_arrays(got, want, what):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for name in want:
        if want[name].dtype == np.float32:
            assert_same_f32(got[name], want[name], f"{name} {what}")
        else:
            assert np.array_equal(got[name], want[name]), f"{name} {what}"


@pytest.mark.parametrize("mode,color", MODE_VARIANTS)
@pytest.mark.parametrize("s", [(3, -2, 1), (0, 0, -12), (1, 0, 0)])
def test_shift_then_integrate_equals_integrate_on_rolled_arrays_in_every_mode(mode, color, s):
    vol, sc = make_volume(RES, 80, 60, color=color)
    m = Model(vol._p, mode)
    for i in range(7):   # two poses revisited: nsample passes 5 and the variance weighting acts
        tr = synth.turntable_pose(i % 2, 8, sc.size)
        assert m.integrate(sc.depth(tr, noise_seed=40 + i), sc.bgra(i) if color else None, m.pose(tr)) > 0
    before = {k: a.copy() for k, a in arrays_of(m.ov).items()}
    state = [k for k in before if k not in ("d", "w", "rgb")]
    assert len(state) == {"RGBNormalized": 4, "LAB": 3, "by_depth": 0}.get(mode, 2)
    assert all(before[k].any() for k in state)
    if "by_variance" in mode:
        assert ((before["nsample"] > 5) & (before["w"] % 1 != 0)).sum() > 1000
    if "by_depth" in mode:
        assert (before["w"] % 1 != 0).sum() > 1000
    m.shift(s, np.array(s, np.float64) * sc.size / RES)
    c = clamp_shift(s, (RES,) * 3)
    fill = {"d": np.float32(-1), "w": np.float32(0), "rgb": np.uint8(0), "nsample": np.int32(0)}
    r = {k: np.ascontiguousarray(rolled(a, c, fill.get(k, np.float32(0)))) for k, a in before.items()}
    want = OracleVolume(vol._p, adopt=(r["d"], r["w"], r.get("rgb")))
    if mode in ("RGBNormalized", "LAB"):
        want.cn = np.ascontiguousarray(np.stack([r[k] for k in state]))
    if "by_variance" in mode:
        want.M, want.nsample = r["M"], r["nsample"]
    assert_same_arrays(arrays_of(m.ov), arrays_of(want), f"rolled, {mode}, shift {s}")
    tr = synth.turntable_pose(1, 8, sc.size)
    dep, col = sc.depth(tr, noise_seed=60), sc.bgra(9) if color else None
    posed = m.pose(tr)
    assert m.integrate(dep, col, posed) == integrate_directly(want, mode, dep, col, synth.cam_from_vol_f32(posed)) > 0
    assert_same_arrays(arrays_of(m.ov), arrays_of(want), f"one more frame, {mode}, shift {s}")
    m.reset()
    assert m.mode == mode and [k for k in arrays_of(m.ov)] == list(before) and not any(arrays_of(m.ov)[k].any() for k in state)


def test_variance_box_upload_writes_the_box_and_nothing_else():
    vol, sc = make_volume(RES, 80, 60)
    m = Model(vol._p, "by_variance")
    rng = np.random.RandomState(3)
    m.ov.M[...], m.ov.nsample[...] = rng.uniform(0, 2, m.ov.M.shape), rng.randint(0, 9, m.ov.M.shape)
    M0, n0 = m.ov.M.copy(), m.ov.nsample.copy()
    box, sl = (3, 5, 9, 20, 11, 4), (slice(9, 13), slice(5, 16), slice(3, 23))
    bM, bn = (a.copy() for a in m.variance_box(box))
    assert np.array_equal(bM, M0[sl]) and np.array_equal(bn, n0[sl])
    m.upload_variance(bM + 1, None, box)
    m.upload_variance(None, bn + 2, box)
    M0[sl] += 1
    n0[sl] += 2
    assert np.array_equal(m.ov.M, M0) and np.array_equal(m.ov.nsample, n0) and m.ov.nsample.dtype == np.int32


@pytest.mark.parametrize("case", mode_cases.CASES, ids=mode_cases.case_id)
def test_the_replay_of_every_mode_case_meets_the_conditions(case):
    """The plan of every case of tests/test_mode_sequences_gpu.py through the model alone: tests/mode_cases.CONDITIONS."""
    model, tally = mode_cases.replay(case)
    print(mode_cases.case_id(case), model.assert_conditions(mode_cases.case_id(case)), dict(tally))


def test_the_plans_run_every_legal_operation_three_times_per_mode_and_shape():
    tally = collections.defaultdict(collections.Counter)
    for c in mode_cases.CASES:
        for e in mode_cases.Setup(c).plan[:-2]:
            assert e["op"] in mode_cases.legal_ops(c)
            tally[c.shape, c.mode][e["op"]] += 1
        plan = mode_cases.Setup(c).plan   # a frame held back by pairing meets a shift in every case
        assert any(a["op"] == "ring" and a["n"] % 2 == 1 and b["op"] == "shift" for a, b in zip(plan, plan[1:])), mode_cases.case_id(c)
    assert len(tally) == 10
    for (shape, mode), t in tally.items():
        legal = set().union(*[mode_cases.legal_ops(c) for c in mode_cases.CASES if (c.shape, c.mode) == (shape, mode)])
        assert ("upload_variance" in legal) == ("by_variance" in mode) and ("save_load" in legal) == ("by_" in mode)
        for op in legal:
            assert t[op] >= 3, (shape, mode, op, dict(t))
    for grid in mode_cases.GRIDS:   # pure x shifts of the register path, of whole flag cells and of a cell and one more, on both grids
        x = {e["s"][0] for c in mode_cases.CASES if c.grid == grid for e in mode_cases.Setup(c).plan
             if e["op"] == "shift" and not (e["s"][1] or e["s"][2])}
        assert x >= set(mode_cases.PURE_X), (grid, x)


# ---- the feature sequences (tests/test_feature_sequences_gpu.py) through the models alone --------------------------------------
FEATURE_STATS = {}


def feature_sequences():
    from tests import test_feature_sequences_gpu as fs
    return fs


def _feature_ids():
    fs = feature_sequences()
    return fs.CASES, fs.IDS


@pytest.mark.parametrize("case", _feature_ids()[0], ids=_feature_ids()[1])
def test_the_replay_of_every_feature_case_runs_through_the_models(case, tmp_path):
    """Every case of tests/test_feature_sequences_gpu.py with the same seeds and draws and no product: the prelude's own
    conditions hold of the models, and the figures the floors are asserted on are collected."""
    fs = feature_sequences()
    FEATURE_STATS[case] = stats = fs.run_case(*case, tmp_path, live=False)
    print(fs.IDS[fs.CASES.index(case)], stats.summary())


def test_the_feature_sequences_meet_their_floors():
    """tests/feature_cases.assert_floors over all seeds of a shape (this test needs the replays above to have run in this
    process): every operation and every chain call at least 5 times, removals that found no frame at most a quarter, merges,
    removals, fields and fetches that are not empty, at least 5 E_INVALID states."""
    fs = feature_sequences()
    from tests.feature_cases import Stats
    assert set(FEATURE_STATS) == set(fs.CASES), f"{len(set(fs.CASES) - set(FEATURE_STATS))} replays did not finish in this run"
    total = {shape: Stats() for shape in fs.SHAPES}
    for case, stats in FEATURE_STATS.items():
        total[case[0]].add(stats)
    for shape in fs.SHAPES:
        print(shape, total[shape].summary())
    fs.assert_all_floors(total)
