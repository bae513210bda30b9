"""GPU tier: castRays (tsdf_hip_cast_rays / _device / _stats; include/tsdf_hip.h states the definition).

1. the rays of a pinhole image reproduce renderView bit for bit, in both layouts, with and without TSDF_HIP_RAYS_AS_GIVEN;
2. arbitrary rays -- outside-in and inside-out -- equal the reference ray by ray (the oracle's renderView on a 1 x 1 image,
   tests/castrays_cases.py), hits with valid and with NaN normals and misses among them;
3. per-ray ranges: a range cut short of the hit misses, a longer one changes nothing, a mix equals the oracle ray by ray;
4. the colour is tsdf_hip_lookup_rgb's at the hit point; 127s through the Python class without colour; LAB + rgb is refused;
5. wave tails (n = 1 .. 4000) and the order: every ray's bytes are those of the 4000-ray call, permuted or not, either flag;
6. refused rays among ordinary ones, a ray whose t makes no float progress: the call returns, the neighbours are unchanged;
7. the device form, the stats, every refusal of the header, a frame held back by frame pairing."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection time, before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests import castrays_cases as cc
from tests.common import assert_same_f32, frames, make_volume
from tests.test_query_gpu import VIEWS, fused64  # noqa: F401  (the 64^3 volume of 6 of 8 turntable frames, colour, and its oracle)

pytestmark = pytest.mark.gpu
N = 2000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw(vol, org, u, rng, n, flags, out, rgb=None, st=None):
    return capi.load().tsdf_hip_cast_rays(vol._h, capi.as_f32p(org), capi.as_f32p(u), capi.as_f32p(rng) if rng is not None else None, n, flags,
                                          capi.as_f32p(out), capi.as_u8p(rgb) if rgb is not None else None,
                                          capi.as_u8p(st) if st is not None else None)


@pytest.fixture(scope="module")
def rays64(fused64):
    """The 2 x 2000 rays of (2) on the 64^3 volume: the oracle's answer, computed once, and the library's for all 4000."""
    vol, ov, sc = fused64
    rng = np.random.RandomState(1)
    o1, u1 = cc.family_outside_in(rng, sc.size, N)
    o2, u2 = cc.family_inside_out(rng, sc.size, N)
    org, u = np.ascontiguousarray(np.concatenate([o1, o2])), np.ascontiguousarray(np.concatenate([u1, u2]))
    one = cc.OneRayOracle(vol._p, ov.d, ov.w, ov.rgb)
    want = one.rays(org, u)
    out, st, rgb = vol.castRays(org, u, want_rgb=True)
    return dict(vol=vol, ov=ov, sc=sc, one=one, org=org, u=u, want=want, out=out, st=st, rgb=rgb)


# ---- 1. pixel rays ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [capi.LAYOUT_F32W, capi.LAYOUT_PACKED], ids=["f32w", "packed"])
def test_pixel_rays_reproduce_render_view(gpu, layout):
    vol, sc = make_volume(32, color=True)
    vol.setLayout(layout)
    vol.reset()
    assert vol.getLayout() == layout
    for i, tr, dep, col in frames(sc, 4, 8):
        vol.integrateCloud(dep, col, tr)
    for view in (0, 2):
        tr = VIEWS[view](sc.size)
        want = vol.renderView(tr, 1, camera_frame=False).reshape(-1, 8)
        du = cc.pixel_directions(vol._p, tr)
        org = np.ascontiguousarray(np.tile(np.asarray(tr, np.float64)[:3, 3].astype(np.float32), (len(du), 1)))
        for as_given in (True, False):
            out, st = vol.castRays(org, du, as_given=as_given)
            assert np.array_equal(bits(out), bits(want)), (view, as_given, int((bits(out) != bits(want)).any(1).sum()))
            assert np.array_equal(st, np.isfinite(want[:, :3]).all(1).astype(np.uint8))
            assert 100 < st.sum() < len(st)     # (the comparison is not vacuous: hits and misses, as tests/test_query_gpu.py asks of a view)
    vol.close()


# ---- 2. arbitrary rays --------------------------------------------------------------------------------------------------------
def test_arbitrary_rays_equal_the_reference(rays64):
    r = rays64
    out, want, st = r["out"], r["want"], r["st"]
    assert_same_f32(out[:N], want[:N], "outside-in rays")
    assert_same_f32(out[N:], want[N:], "inside-out rays")
    hit = np.isfinite(want[:, 0])
    assert np.array_equal(st, hit.astype(np.uint8))
    nan_normal = hit & np.isnan(want[:, 3])
    print("hits", int(hit[:N].sum()), int(hit[N:].sum()), "NaN-normal hits", int(nan_normal.sum()), "misses", int((~hit).sum()))
    assert hit[:N].sum() >= 1500 and hit[N:].sum() >= 400
    assert nan_normal.sum() >= 100 and (~hit).sum() >= 100
    miss = want[~hit]
    assert np.isnan(miss[:, :3]).all() and ((miss[:, 3:6] == 0).all(1) | np.isnan(miss[:, 3:6]).all(1)).all()


# ---- 3. per-ray ranges --------------------------------------------------------------------------------------------------------
def test_per_ray_ranges(rays64):
    r = rays64
    vol, one, out = r["vol"], r["one"], r["out"]
    zmin, zmax = vol.getSensorDistanceBounds()
    good = np.flatnonzero((r["st"] == 1) & np.isfinite(out[:, 3]) & (out[:, 6] > 0.02))
    pick = good[np.linspace(0, len(good) - 1, 200).astype(int)]
    org, u, full = r["org"][pick], r["u"][pick], out[pick]
    tstar = full[:, 6]
    short = np.stack([np.full(200, zmin, np.float32), tstar / np.float32(2)], 1).astype(np.float32)
    got, st = vol.castRays(org, u, short)
    want = one.rays(org, u, short)
    assert_same_f32(got, want, "tmax = t*/2")
    assert np.isfinite(want[:, 0]).sum() == 0 and (st == 0).all(), int(np.isfinite(want[:, 0]).sum())
    longer = np.stack([np.full(200, zmin, np.float32), tstar * np.float32(2)], 1).astype(np.float32)
    got, st = vol.castRays(org, u, longer)
    assert np.array_equal(bits(got), bits(full)) and (st == 1).all()
    mix = np.stack([np.full(200, zmin, np.float32), np.full(200, zmax, np.float32)], 1)
    mix[0::4] = short[0::4]
    mix[1::4] = longer[1::4]
    mix[2::4, 0] = tstar[2::4] / np.float32(3)
    mix[2::4, 1] = tstar[2::4] * np.float32(1.5)
    mix[3::8] = [0.05, 0.05]          # tmax == tmin: the loop does not run
    got, st = vol.castRays(org, u, mix)
    want = one.rays(org, u, mix)
    assert_same_f32(got, want, "mixed ranges")
    assert np.array_equal(st, np.isfinite(want[:, 0]).astype(np.uint8)) and 50 < st.sum() < 200
    assert (got[3::8, 6] == np.float32(0.05)).all() and (got[3::8, 7] == 0).all()


# ---- 4. colour ----------------------------------------------------------------------------------------------------------------
def test_colour_is_the_lookup_at_the_hit_point(rays64):
    r = rays64
    vol, out, st, rgb = r["vol"], r["out"], r["st"], r["rgb"]
    hit = st == 1
    pts = np.ascontiguousarray(out[hit, :3])
    c, found = np.empty((len(pts), 3), np.uint8), np.empty(len(pts), np.uint8)
    capi.check(capi.load().tsdf_hip_lookup_rgb(vol._h, capi.as_f32p(pts), len(pts), capi.as_u8p(c), capi.as_u8p(found)), "lookup_rgb")
    c[found == 0] = 0
    assert np.array_equal(rgb[hit], c) and (rgb[~hit] == 0).all()
    assert found.sum() > 2000 and len(np.unique(rgb[hit], axis=0)) > 50
    out2, st2 = vol.castRays(r["org"], r["u"])
    assert np.array_equal(bits(out2), bits(out)) and np.array_equal(st2, st)


def test_colour_without_colour_and_on_lab(gpu):
    vol, sc = make_volume(32, color=False)
    vol.reset()
    for i, tr, dep, col in frames(sc, 3, 8):
        vol.integrateCloud(dep, None, tr)
    rng = np.random.RandomState(5)
    org, u = cc.family_outside_in(rng, sc.size, 500)
    out, st, rgb = vol.castRays(org, u, want_rgb=True)
    hit = st == 1
    assert 300 < hit.sum() < 500
    assert (rgb[hit] == 127).all() and (rgb[~hit] == 0).all()       # (every hit of these rays lies inside the box)
    raw_rgb = np.full((500, 3), 9, np.uint8)
    o2 = np.empty((500, 8), np.float32)
    assert raw(vol, org, u, None, 500, 0, o2, raw_rgb) == capi.OK and (raw_rgb == 0).all()   # the library's bytes: no colour plane
    vol.close()
    vol, sc = make_volume(32, color=True)
    vol.setColorMode("LAB")
    vol.reset()
    for i, tr, dep, col in frames(sc, 2, 8):
        vol.integrateCloud(dep, col, tr)
    o2 = np.full((500, 8), 7.0, np.float32)
    raw_rgb[:] = 9
    s2 = np.full(500, 5, np.uint8)
    assert raw(vol, org, u, None, 500, 0, o2, raw_rgb, s2) == capi.E_UNSUPPORTED
    assert b"LAB" in capi.load().tsdf_hip_last_error()
    assert (o2 == 7.0).all() and (raw_rgb == 9).all() and (s2 == 5).all()
    assert raw(vol, org, u, None, 500, 0, o2, None, s2) == capi.OK and 200 < s2.sum() < 500
    vol.close()


# ---- 5. tails and order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_given", [False, True], ids=["any-order", "as-given"])
def test_tails_and_order(rays64, as_given):
    r = rays64
    vol, org, u = r["vol"], r["org"], r["u"]
    sel = np.random.RandomState(7).permutation(2 * N)     # both families in every prefix
    for n in (1, 63, 64, 65, 257, 4000):
        idx = sel[:n]
        out, st, rgb = vol.castRays(org[idx], u[idx], want_rgb=True, as_given=as_given)
        assert np.array_equal(bits(out), bits(r["out"][idx])), n
        assert np.array_equal(st, r["st"][idx]) and np.array_equal(rgb, r["rgb"][idx]), n
        assert vol.castRaysStats()[:3] == (n, int((st == 1).sum()), 0)


# ---- 6. admission on the device -----------------------------------------------------------------------------------------------
def test_refused_rays_among_ordinary_ones(rays64):
    r = rays64
    vol, sc = r["vol"], r["sc"]
    leaf = np.float32(sc.size) / np.float32(64)
    zmin, zmax = vol.getSensorDistanceBounds()
    hits = np.flatnonzero((r["st"] == 1) & np.isfinite(r["out"][:, 3]))[:8]
    too_long = float(np.float32(cc.bound_range(leaf) * (1 + 1e-3)))
    bad = [  # (o, u, tmin, tmax): every one refused by the rule
        ([np.nan, 0, -0.4], [0, 0, 1], zmin, zmax), ([0, 0, -0.4], [0, np.inf, 1], zmin, zmax), ([0, 0, -0.4], [0, 0, 1], np.nan, zmax),
        ([0, 0, -0.4], [0, 0, 1], zmin, np.inf), ([0, 0, -0.4], [0, 0, 1], -np.inf, zmax), ([0, 0, -0.4], [0, 0, 1], 0.0, too_long),
        ([0, 0, -0.4], [0, 0, 1], -3.0e38, 3.0e38)]
    far = ([0, 0, -0.4], [0, 0, 1], 1e6, 1e6 + 1)
    org, u, rng, kind = [], [], [], []
    for k in range(8):
        org.append(r["org"][hits[k]]), u.append(r["u"][hits[k]]), rng.append((zmin, zmax)), kind.append("hit")
        o, d, a, b = bad[k] if k < 7 else far
        org.append(o), u.append(d), rng.append((a, b)), kind.append("bad" if k < 7 else "far")
    org, u, rng = (np.ascontiguousarray(np.array(x, np.float32)) for x in (org, u, rng))
    kind = np.array(kind)
    for row, kd in zip(range(16), kind):
        ok, cap = cc.admit_rule(org[row], u[row], rng[row, 0], rng[row, 1], leaf)
        assert ok == (kd != "bad"), (row, kd)
    for as_given in (False, True):
        out, st, rgb = vol.castRays(org, u, rng, want_rgb=True, as_given=as_given)
        b = kind == "bad"
        assert (st[b] == 2).all() and np.isnan(out[b, :3]).all() and (out[b, 3:6] == 0).all() and (out[b, 7] == 0).all() and (rgb[b] == 0).all()
        assert np.array_equal(bits(out[b, 6]), bits(rng[b, 0]))           # t = tmin, as given (NaN and -inf included)
        h = kind == "hit"
        assert np.array_equal(bits(out[h]), bits(r["out"][hits])) and (st[h] == 1).all() and np.array_equal(rgb[h], r["rgb"][hits])
        f = kind == "far"
        assert st[f][0] in (0, 3) and not np.isfinite(out[f, :3]).any() and (out[f, 3:6] == 0).all()
        stats = vol.castRaysStats()
        assert stats[:3] == (16, 8, int((st >= 2).sum())) and stats[2] >= 7
    # t = 1e6 makes no float progress with this volume's steps: only the integer cap ends that ray
    assert st[kind == "far"][0] == 3 and out[kind == "far", 6][0] == np.float32(1e6)


# ---- 7. forms and refusals ----------------------------------------------------------------------------------------------------
def test_the_device_form_equals_the_host_form(rays64):
    r = rays64
    vol, n = r["vol"], 2 * N
    t_org = torch.from_numpy(r["org"]).cuda()
    t_dir = torch.from_numpy(r["u"]).cuda()
    rng = np.stack([np.full(n, 0.0, np.float32), np.where(np.arange(n) % 3 == 0, 0.2, 0.75).astype(np.float32)], 1)
    t_rng = torch.from_numpy(rng).cuda()
    for use_rng in (False, True):
        for as_given in (False, True):
            t_out = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda")
            t_rgb = torch.full((n, 3), 9, dtype=torch.uint8, device="cuda")
            t_st = torch.full((n,), 5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert vol.castRaysDevice(t_org.data_ptr(), t_dir.data_ptr(), t_rng.data_ptr() if use_rng else 0, n, t_out.data_ptr(),
                                      t_rgb.data_ptr(), t_st.data_ptr(), as_given=as_given) is True
            stats = vol.castRaysStats()          # (waits for the call)
            out, st, rgb = vol.castRays(r["org"], r["u"], rng if use_rng else None, want_rgb=True)
            assert np.array_equal(bits(t_out.cpu().numpy()), bits(out))
            assert np.array_equal(t_st.cpu().numpy(), st) and np.array_equal(t_rgb.cpu().numpy(), rgb)
            assert stats[:3] == (n, int((st == 1).sum()), 0) and stats[1] > 1000
            if not use_rng:
                assert np.array_equal(bits(out), bits(r["out"]))
    # without rgb and status
    t_out = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vol.castRaysDevice(t_org.data_ptr(), t_dir.data_ptr(), 0, n, t_out.data_ptr())
    vol.synchronize()
    assert np.array_equal(bits(t_out.cpu().numpy()), bits(r["out"]))


def test_refusals_leave_the_outputs_alone(rays64):
    r = rays64
    lib = capi.load()
    org, u = r["org"][:100], r["u"][:100]
    out, rgb, st = np.full((100, 8), 7.0, np.float32), np.full((100, 3), 9, np.uint8), np.full(100, 5, np.uint8)

    def untouched():
        return (out == 7.0).all() and (rgb == 9).all() and (st == 5).all()

    vol = r["vol"]
    assert raw(vol, org, u, None, 100, 2, out, rgb, st) == capi.E_INVALID and untouched()          # unknown flag bits
    assert raw(vol, org, u, None, 100, -1, out, rgb, st) == capi.E_INVALID and untouched()
    assert raw(vol, org, u, None, 0, 0, out, rgb, st) == capi.E_INVALID and untouched()            # n == 0
    assert lib.tsdf_hip_cast_rays(vol._h, None, capi.as_f32p(u), None, 100, 0, capi.as_f32p(out), None, None) == capi.E_INVALID
    assert lib.tsdf_hip_cast_rays(vol._h, capi.as_f32p(org), None, None, 100, 0, capi.as_f32p(out), None, None) == capi.E_INVALID
    assert lib.tsdf_hip_cast_rays(vol._h, capi.as_f32p(org), capi.as_f32p(u), None, 100, 0, None, None, None) == capi.E_INVALID
    assert lib.tsdf_hip_cast_rays(vol._h, capi.as_f32p(org), capi.as_f32p(u), None, 2 ** 31, 0, capi.as_f32p(out), None, None) == capi.E_INVALID
    assert lib.tsdf_hip_cast_rays_device(vol._h, None, None, None, 100, 0, None, None, None) == capi.E_INVALID
    assert lib.tsdf_hip_cast_rays_stats(vol._h, None) == capi.E_INVALID
    assert untouched()
    # a slab handle
    slab, sc = make_volume(32, color=True)
    slab.setZSlab(8, 24, halo=2)
    slab.reset()
    assert raw(slab, org, u, None, 100, 0, out, rgb, st) == capi.E_UNSUPPORTED and untouched()
    assert b"slab" in lib.tsdf_hip_last_error()
    slab.close()
    # a multi-GPU set, here of one device
    if lib.tsdf_hip_device_count() >= 1:
        multi, sc = make_volume(32, color=True)
        multi.setDevices([0])
        multi.reset()
        assert raw(multi, org, u, None, 100, 0, out, rgb, st) == capi.E_UNSUPPORTED and untouched()
        assert b"multi" in lib.tsdf_hip_last_error()
        assert lib.tsdf_hip_cast_rays_device(multi._h, capi.as_f32p(org), capi.as_f32p(u), None, 100, 0, capi.as_f32p(out), None,
                                             None) == capi.E_UNSUPPORTED and untouched()
        multi.close()


def test_a_held_back_frame_is_seen(gpu):
    """Frame pairing on: B is committed and waits for a partner; the rays first launch it."""
    vol, sc = make_volume(32, color=True)
    vol.reset()
    ov = OracleVolume(vol._p)
    fr = list(frames(sc, 2, 8))
    vol.integrateCloud(fr[0][2], fr[0][3], fr[0][1])
    ov.integrate(fr[0][2], fr[0][3], synth.cam_from_vol_f32(fr[0][1]))
    org, u = cc.family_outside_in(np.random.RandomState(11), sc.size, 300)
    before, _ = vol.castRays(org, u)
    vol.setFramePairing(True)
    vol.integrateCloud(fr[1][2], fr[1][3], fr[1][1], pipelined=True)
    ov.integrate(fr[1][2], fr[1][3], synth.cam_from_vol_f32(fr[1][1]))
    out, st = vol.castRays(org, u)
    want = cc.OneRayOracle(vol._p, ov.d, ov.w, ov.rgb).rays(org, u)
    assert_same_f32(out, want, "rays after a held-back frame")
    assert st.sum() > 100 and not np.array_equal(bits(out), bits(before))
    vol.setFramePairing(False)
    vol.close()
