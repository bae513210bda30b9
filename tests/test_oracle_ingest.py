"""CPU tier: the C oracle's frame ingest (oracle_organize, oracle/tsdf_oracle.c) against the plain Python model of the
same loop in tests/ingest_cases.py, on every case of that file and every image size -- depth bits, filled count, colours
of the filled pixels -- and the coverage floors of the cases, counted from the model alone.  This pins the restatement
that tests/test_ingest_gpu.py then holds tsdf_hip_organize to.  Bar: bit equality."""
import numpy as np
import pytest

from cpu_tsdf_amd import capi
from oracle.oracle import OracleVolume
from tests import ingest_cases as ic
from tests.common import assert_same_f32


def params(s, color=True):
    W, H, fx, fy, cx, cy = s
    p = capi.default_params()
    p.res[:] = (32,) * 3
    p.size[:] = (0.125,) * 3
    p.fx, p.fy, p.cx, p.cy = fx, fy, cx, cy
    p.image_width, p.image_height = W, H
    p.min_sensor_dist, p.max_sensor_dist = 0.0, 0.375
    p.integrate_color = int(color)
    return p


_memo = {}


def run(s, case):
    """(oracle's frame, model's frame with its per-point record), once per case and scene."""
    key = (s, case.name)
    if key not in _memo:
        ov = OracleVolume(params(s, case.color))
        col = None if case.bgra is None else np.ascontiguousarray(case.bgra)
        _memo[key] = ov.organize(case.xyz, col, **case.kw), ic.model_organize(case.xyz, case.bgra, s, detail=True, **case.kw)
    return _memo[key]


def same_frame(got, want, what):
    (d, c, n), (d2, c2, n2) = got, want[:3]
    assert_same_f32(d, d2, f"{what}: depth")
    assert np.array_equal(np.signbit(d), np.signbit(d2)), what
    assert n == n2 == int((~np.isnan(d2)).sum()), (what, n, n2)
    filled = ~np.isnan(d2)
    assert np.array_equal(c[filled], c2[filled]), f"{what}: colours of the filled pixels"
    assert (c[~filled] == [0, 0, 0, 255]).all() and (c2[~filled] == [0, 0, 0, 255]).all(), what


@pytest.mark.parametrize("group", ic.GROUPS)
@pytest.mark.parametrize("size", ic.SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_oracle_equals_the_serial_model(size, group):
    s = ic.scene(*size)
    mine = [c for c in ic.cases(s) if c.group == group]
    assert mine
    for c in mine:
        same_frame(*run(s, c), f"{c.name} at {size}")


@pytest.mark.parametrize("size", ic.SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_floors_of_pixel_edges(size):
    s = ic.scene(*size)
    case = next(c for c in ic.cases(s) if c.name == "pixel_edges")
    _, (depth, _, filled, det) = run(s, case)
    st = ic.edge_stats(s, det)
    print(size, st, "filled", filled)
    ic.check_edge_floors(s, st)
    assert len(np.unique(case.bgra.view("<u4"))) == len(case.bgra)   # every point a different colour
    which = ic.edge_sets(s)
    assert (which == 2).sum() >= 21 * (size[0] + 5) and det["ok"][which == 2].any()   # the diagonal set is there and lands
    # along u alone (the y = 0 set) the four image sizes measured with the oracle before the builder was written hold too
    only_u = {k: v for k, v in ic.edge_stats(s, {k: (v[which == 0] if k != "winner" else v) for k, v in det.items()}).items() if k.endswith("_u")}
    want = {(160, 120): (1770, 18, 10), (7, 5): (87, 17, 5), (65, 3): (742, 18, 14), (1, 1): (18, 18, 3)}.get(size)
    if want:
        assert (only_u["exact_u"], only_u["neg_kept_u"], only_u["at_end_u"]) == want, only_u


@pytest.mark.parametrize("size", ic.SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_floors_of_extremes_units_and_transforms(size):
    s = ic.scene(*size)
    W, H, fx, fy, cx, cy = s
    by_name = {c.name: c for c in ic.cases(s)}
    centre = (int(cy), int(cx))
    # extremes: a pixel with a denormal depth, one with +inf; the three points the loop keeps and the ones it drops
    (_, (d, _, _, det)) = run(s, by_name["extremes"])
    assert ic.is_denormal(d).any() and d[centre] == np.float32(1e-45)
    pts = by_name["extremes"].xyz
    n_list = len(ic.extreme_points(s))
    kept = [tuple(float(v) for v in pts[j, :3]) for j in range(n_list) if det["ok"][j]]
    # (the loop keeps these five and drops the rest of the list: (1e-45, 0, 1e-45) projects round(fx) columns right of cx)
    assert kept == [(0, 0, float(np.float32(1e-45))), (0, 0, float(np.float32(1e-39))), (0, 0, np.inf), (1, 1, np.inf), (0, 0, float(np.float32(3e38)))], kept
    (_, (d, _, _, det2)) = run(s, by_name["extremes_no_denormal"])
    assert np.isposinf(d[centre]) and (W * H == 1 or np.isfinite(d).any())
    # the conversion's limits: fu or fv exactly 2^31 and exactly -2^31, and floats on either side of both
    with np.errstate(invalid="ignore"):
        f = np.concatenate([det["fu"], det["fv"]])
    for lim in (np.float32(2 ** 31), np.float32(-2 ** 31)):
        assert (f == lim).any() and (f == np.nextafter(lim, np.float32(0))).any() and (f == np.nextafter(lim, lim * 2)).any(), lim
    assert ((det["u"] == ic.INT_MIN) | (det["v"] == ic.INT_MIN)).sum() >= 10
    # units: 0 fills nothing either way; the others fill something
    for cloud in ("extremes", "pixel_edges"):
        assert run(s, by_name[f"units_0_zero_nans_{cloud}"])[1][2] == 0 and run(s, by_name[f"units_0_{cloud}"])[1][2] == 0
        assert run(s, by_name[f"units_-1_{cloud}"])[1][2] > 0
    assert run(s, by_name["units_1e30_pixel_edges"])[1][2] > 0 and run(s, by_name["units_1e-30_pixel_edges"])[1][2] > 0
    # transforms: (0, 0, +inf) stays on (cx, cy) under all four; the turn and the NaN entry fill nothing else
    for name in ("turn180", "scale1e20", "nan_entry", "inf_entry"):
        case = by_name[f"transform_{name}"]
        d, _, filled, det = run(s, case)[1]
        z = case.xyz[:, 2]
        x_fin = np.isfinite(case.xyz[:, 0])
        at_inf = np.isposinf(z) & x_fin
        assert at_inf.sum() >= 4 and det["ok"][at_inf].all() and (det["u"][at_inf] == centre[1]).all() and (det["v"][at_inf] == centre[0]).all(), name
        with np.errstate(invalid="ignore"):
            front = np.isfinite(z) & (z > 0)
        if name == "turn180":     # what was in front is behind now, and (0, 0, -1) from behind the camera is in front
            assert not det["ok"][front].any() and det["ok"][np.isfinite(z) & (z < 0)].any() and filled >= 1
        elif name == "scale1e20":
            assert det["ok"][front].sum() >= (10 if W * H > 1 else 1) and np.isfinite(d).any()   # (1 x 1 has no ordinary points)
        else:                     # nothing, or everything, on the one pixel that holds +inf
            small = front & (np.abs(case.xyz[:, :2]) < 1).all(1)
            assert filled == 1 and np.isposinf(d[centre]), (name, filled)
            assert det["ok"][small].all() if name == "inf_entry" else not det["ok"][front].any(), name


@pytest.mark.parametrize("size", ic.SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_floors_of_one_pixel(size):
    s = ic.scene(*size)
    case = next(c for c in ic.cases(s) if c.name == "one_pixel")
    _, (depth, col, filled, det) = run(s, case)
    st = ic.one_pixel_stats(s, case.xyz, depth, det)
    print(size, st)
    ic.check_one_pixel_floors(st)
    assert filled == min(5, size[0])
    assert depth[int(s[5]), int(s[4])] == ic.one_pixel_depths()[0]
    assert len(np.unique(case.bgra.view("<u4"))) == len(case.bgra)


def test_sizes_strides_and_the_int_conversion():
    s = ic.scene(160, 120)
    cs = ic.cases(s)
    assert [len(c.xyz) for c in cs if c.group == "sizes"] == list(ic.SIZES_N)
    assert sorted({c.xyz.shape[1] for c in cs if c.group == "strides"}) == [3, 4, 5, 8]
    assert sorted({c.bgra.shape[1] for c in cs if c.group == "strides" and c.bgra is not None}) == [4, 7, 32]
    assert [c.name for c in cs if c.bgra is None] == ["stride_xyz8_none"] and [c.name for c in cs if not c.color] == ["stride_xyz3_c4_plain_volume"]
    f = np.float32
    assert [ic.to_int(f(v)) for v in (-0.99, -0.0, 0.99, 1.5, -1.5, 2147483520.0, -2147483648.0)] == [0, 0, 0, 1, -1, 2147483520, -2 ** 31]
    assert [ic.to_int(f(v)) for v in (2147483648.0, -2147483904.0, np.inf, -np.inf, np.nan)] == [ic.INT_MIN] * 5
