"""GPU tier: the second integrate family -- k_integrate_rgbn (setColorMode("RGBNormalized")), k_lab_image +
k_integrate_lab (setColorMode("LAB")) and k_integrate_plain modes 2 and 4 (weight_by_depth, weight_by_variance) --
against the CULLED oracle (tests/test_oracle_culled_modes.py pins it to the compiled reference), bit for bit:

  * a fixed-seed slice of tests/evidence/fuzz_product_colour_modes.py, run as a subprocess;
  * one case per mode with a narrow camera whose principal point sits 40 % off centre: the product equals the culled
    oracle, and the cull provably removed voxels (the unculled oracle differs);
  * x counts 33, 45 and 70 (rows padded to the pitch, padded lanes read NaN centres);
  * weight_by_depth on a 12 m volume: voxels past 10 m get w_new = 0, fresh ones 0/0 = NaN, and are rendered and meshed;
  * frame pairing on and off;
  * LAB's exact colours (tsdf_lab_exact_colors) in chunks of a few thousand voxels (test knob lab_chunk): mesh colours,
    renderColoredView and lookup_rgb identical to the default chunk and to the oracle;
  * more than 2^32 voxels (2048 x 2048 x 1040) per mode: plane groups straddling z = 512 (2^31 elements) and z = 1024
    (2^32 elements) and the last planes against SlabOracle, colour and variance state included."""
import ctypes as C
import time

import numpy as np
import pytest

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, TSDFVolumeOctree
from oracle import oracle
from oracle.oracle import OracleVolume, SlabOracle
from tests.common import assert_same_f32
from tests.evidence import fuzz_product_colour_modes as hunt
from tests.test_evidence_gpu import run_script
from tests.test_fullsize_gpu import free_gb

pytestmark = pytest.mark.gpu
MODES = hunt.MODES


def case(mode, **kw):
    """A hunt case with fixed, moderate values; `kw` overrides."""
    W, H = 80, 60
    c = dict(mode=mode, color=True, res3=(64, 64, 64), size3=(1.0, 1.0, 1.0), W=W, H=H, fx=1.3 * W, fy=1.3 * W,
             cx=W / 2 - 0.5 + 0.4 * W / 2, cy=H / 2 - 0.5 - 0.2 * H / 2, zmin=0.05, zmax=3.5, pos=0.08, neg=0.05,
             wmax=3.5, order=0, handle="one", n_dev=2, zslab=(0, 0, 0), entry="sync", n_poses=2,
             n_frames=9 if "by_variance" in mode else 4, seed=4242 + MODES.index(mode), off_centre=True)
    c.update(kw)
    if "res3" in kw and "size3" not in kw:   # cubic voxels of 1/64 m
        c["size3"] = tuple(r / 64 for r in c["res3"])
    return c


def test_colour_modes_hunt_slice(gpu):
    rc, out, err = run_script(["tests/evidence/fuzz_product_colour_modes.py", "--cases", "30", "--seed", "601"])
    assert rc == 0, (out[-3000:], err[-2000:])
    assert "30 cases, seed 601: 0 with differences" in out, out[-1500:]
    assert out.count(" ok") >= 30 and out.count("cull-bites") >= 5


@pytest.mark.parametrize("mode", MODES)
def test_off_centre_camera_equals_the_culled_oracle(gpu, mode):
    c = case(mode)
    what, info = hunt.run_case(c, check_cull=True)
    assert not what, what
    assert info["cull_removed"], "the reference's cull removed nothing: the case does not test it"
    assert info["observed"] > 5000
    if "by_variance" in mode:
        assert info["frac"] > 0.01


@pytest.mark.parametrize("nx", [33, 45, 70])
@pytest.mark.parametrize("mode", MODES)
def test_rows_padded_to_the_pitch(gpu, mode, nx):
    c = case(mode, res3=(nx, 40, 36), color=mode in ("RGBNormalized", "LAB") or nx != 45, n_frames=7 if "by_variance" in mode else 3)
    what, info = hunt.run_case(c)
    assert not what, what
    assert info["observed"] > 1000


@pytest.mark.parametrize("mode", MODES)
def test_rows_wider_than_one_block(gpu, mode):
    """260 voxels along x: the plain kernels' second x block (blockIdx.x = 1) with four live lanes.  The camera was chosen
    on the CPU against the oracle alone so that it observes voxels there (336-376 of the 1920, by mode); the default
    camera of `case` observes none, and the test would pass without testing anything."""
    c = case(mode, res3=(260, 24, 20), color=True, seed=2, fx=0.5 * 80, fy=0.5 * 80, zmax=8.0, eye=(7, 11), n_poses=3,
             n_frames=7 if "by_variance" in mode else 3)
    what, info = hunt.run_case(c)
    assert not what, what
    assert info["observed_x256"] >= 300, "the case must observe voxels at x >= 256"


@pytest.mark.parametrize("handle", ["one", "multi"])
def test_weight_by_depth_past_ten_metres(gpu, handle):
    """A 12 m volume seen from 6-11 m: every voxel observed past 10 m gets w_new = 0 -- a fresh voxel d = 0/0 = NaN,
    w = 0 -- the nearer ones fractional weights; the renders, samples and meshes of that volume equal the oracle's."""
    c = case("by_depth", res3=(48, 48, 48), size3=(12.0, 12.0, 12.0), fx=0.9 * 80, fy=0.9 * 80, cx=39.5, cy=29.5,
             zmin=0.0, zmax=40.0, pos=1.0, neg=0.7, wmax=100.0, handle=handle, n_dev=3, n_frames=5, off_centre=False, eye=(0.5, 0.9))
    what, info = hunt.run_case(c)
    assert not what, what
    assert info["nan"] > 100 and info["observed"] > 1000


@pytest.mark.parametrize("mode", MODES)
def test_frame_pairing_on_and_off(gpu, mode):
    for handle in ("one", "multi"):
        for entry in ("pipelined", "paired", "device2"):
            what, _ = hunt.run_case(case(mode, handle=handle, entry=entry, n_dev=3, cx=39.5, cy=29.5, fx=0.7 * 80, fy=0.7 * 80))
            assert not what, (handle, entry, what)


def lab_volume():
    W, H = 96, 72
    v = TSDFVolumeOctree()
    v.setResolution(64, 64, 64)
    v.setGridSize(1.0, 1.0, 1.0)
    v.setImageSize(W, H)
    v.setCameraIntrinsics(0.8 * W, 0.8 * W, W / 2 - 0.5 + 0.35 * W / 2, H / 2 - 0.5)
    v.setSensorDistanceBounds(0.0, 3.0)
    v.setDepthTruncationLimits(0.05, 0.05)
    v.setIntegrateColor(True)
    v.setColorMode("LAB")
    v.reset()
    ov = OracleVolume(v._p)
    sc = synth.Scene(1.0, W, H)
    sc.fx, sc.fy, sc.cx, sc.cy = v._p.fx, v._p.fy, v._p.cx, v._p.cy
    rng = np.random.RandomState(5)
    for i in range(5):
        tr = synth.turntable_pose(i, 5, 1.0, tilt=0.1 * i)
        dep = sc.depth(tr, noise_seed=70 + i)
        col = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
        v.integrateCloud(dep, col, tr)
        ov.integrate_lab(dep, col, synth.cam_from_vol_f32(tr), planes=ov.reference_cull_planes(tr))
    return v, ov


def lab_readers(v):
    out = {}
    for wmin in (0.0, 2.0):
        mc = MarchingCubesTSDFOctree()
        mc.setInputTSDF(v)
        mc.setMinWeight(wmin)
        mc.setColorByRGB(True)
        out[f"mesh{wmin}"] = mc.reconstruct()
    tr = synth.turntable_pose(2, 8, 1.0)
    out["view"] = v.renderColoredView(tr, 1)
    pts = (np.random.RandomState(3).uniform(-0.5, 0.5, (20000, 3))).astype(np.float32)
    rgb, found = np.empty((len(pts), 3), np.uint8), np.empty(len(pts), np.uint8)
    capi.check(capi.load().tsdf_hip_lookup_rgb(v._need(), capi.as_f32p(pts), len(pts), capi.as_u8p(rgb), capi.as_u8p(found)), "lookup_rgb")
    out["lookup"] = (pts, rgb, found)
    return out, tr


def test_lab_exact_colours_in_small_chunks(gpu):
    v, ov = lab_volume()
    try:
        base, tr = lab_readers(v)
        capi.set_tuning("lab_chunk", 3001)
        small, _ = lab_readers(v)
    finally:
        capi.set_tuning("lab_chunk", 16 << 20)
    for wmin in (0.0, 2.0):
        a, b = base[f"mesh{wmin}"], small[f"mesh{wmin}"]
        assert len(a["vertices"]) > 3 * 3001 * 3, "the mesh must span several chunks"
        assert_same_f32(a["vertices"], b["vertices"], "mesh")
        assert np.array_equal(a["rgb"], b["rgb"])
        v_m, c_m, _ = ov.march(wmin, 1)
        assert_same_f32(b["vertices"], v_m, "mesh vs oracle")
        assert np.array_equal(b["rgb"], c_m)
    (ca, ra), (cb, rb) = base["view"], small["view"]
    assert_same_f32(ca, cb, "renderColoredView cloud")
    assert np.array_equal(ra, rb) and np.array_equal(rb, hunt.oracle_colours(ov, cb, tr)) and (rb > 0).any(axis=-1).sum() > 300
    pts, rgb_a, found_a = base["lookup"]
    _, rgb_b, found_b = small["lookup"]
    assert np.array_equal(found_a, found_b) and np.array_equal(rgb_a, rgb_b) and found_b.sum() > 15000
    want = np.zeros_like(rgb_b)
    idx = (C.c_int * 3)()
    for i, (x, y, z) in enumerate(pts):
        if oracle.lib().oracle_containing(C.byref(ov.p), float(x), float(y), float(z), idx):
            want[i] = ov.rgb[idx[2], idx[1], idx[0]]
    assert np.array_equal(rgb_b, want)
    v.close()


# ---------------------------------------------------------------------------------------------------------------------
# more than 2^32 voxels
BIG = (2048, 2048, 1040)
GROUPS = [(509, 515), (1021, 1027), (1036, 1040)]   # z = 512: 2^31 elements; z = 1024: 2^32; the last planes
BYTES = {"RGBNormalized": 28, "LAB": 24, "by_depth": 12, "by_variance": 20, "by_depth+by_variance": 20}


@pytest.mark.parametrize("mode", MODES)
def test_more_than_2_to_the_32_voxels(gpu, mode):
    need = BYTES[mode] * np.prod(BIG, dtype=np.float64) / 2 ** 30 + 4
    if free_gb() < need:
        pytest.skip(f"needs about {need:.0f} GB of free HBM, {free_gb():.0f} GB free")
    t0 = time.time()
    W, H = 320, 240
    vs = 2.0 ** -8   # 8 m x 8 m x 4.06 m
    v = TSDFVolumeOctree()
    v.setResolution(*BIG)
    v.setGridSize(*(r * vs for r in BIG))
    v.setImageSize(W, H)
    v.setCameraIntrinsics(1.2 * W, 1.2 * W, W / 2 - 0.5 - 0.4 * W / 2, H / 2 - 0.5 + 0.3 * H / 2)   # narrow, off centre
    v.setSensorDistanceBounds(0.0, 30.0)
    v.setDepthTruncationLimits(0.1, 0.06)
    v.setWeightTruncationLimit(2.5)
    v.setIntegrateColor(mode != "by_depth")
    if mode in ("RGBNormalized", "LAB"):
        v.setColorMode(mode)
    else:
        v.setWeighting("by_depth" in mode, "by_variance" in mode)
    v.reset()
    slabs = [SlabOracle(v._p, a, b) for a, b in GROUPS]
    size = BIG[2] * vs
    sc = synth.Scene(size, W, H, sphere=0.3, box=0.49)
    sc.fx, sc.fy, sc.cx, sc.cy = v._p.fx, v._p.fy, v._p.cx, v._p.cy
    sc.h = np.array([0.49 * r * vs for r in BIG])
    rng = np.random.RandomState(17)
    frames = [synth.look_at_pose(np.array([0.3, -0.2, -1.0]) * 5.5 * k, target=(0.1, 0.0, 0.2)) for k in (1.0, 1.05, 1.0)]
    n_frames = 7 if "by_variance" in mode else 3
    t_int = 0.0
    for i in range(n_frames):
        tr = frames[i % 3]
        dep = sc.depth(tr, noise_seed=100 + i, noise_sigma=0.01)
        dep[rng.rand(H, W) < 0.02] = np.nan
        col = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
        col[rng.rand(H, W) < 0.03, :3] = 0
        colv = col if v._p.integrate_color else None
        t1 = time.time()
        v.integrateCloud(dep, colv, tr)
        v.synchronize()
        t_int += time.time() - t1
        T = synth.cam_from_vol_f32(tr)
        planes = slabs[0].reference_cull_planes(tr)
        for s in slabs:
            if mode == "RGBNormalized":
                s.integrate_rgbn(dep, colv, T, planes=planes)
            elif mode == "LAB":
                s.integrate_lab(dep, colv, T, planes=planes)
            elif "by_variance" in mode:
                s.integrate_variance(dep, colv, T, weight_by_depth="by_depth" in mode, planes=planes)
            else:
                s.integrate(dep, colv, T, weight_by_depth=True, planes=planes)
    nx, ny, _ = BIG
    for (a, b), s in zip(GROUPS, slabs):
        d, w, rgb = v.download(z0=a, nz=b - a)
        assert (s.w > 0).sum() > 10000, f"planes [{a},{b}) were hardly observed"
        assert_same_f32(d, s.d, f"d [{a},{b})")
        assert_same_f32(w, s.w, f"w [{a},{b})")
        if rgb is not None:
            assert np.array_equal(rgb, s.rgb), f"rgb [{a},{b})"
        if mode in ("RGBNormalized", "LAB"):
            cs = v.downloadColorState(z0=a, nz=b - a)
            for k in range(len(cs)):
                assert_same_f32(cs[k], s.cn[k], f"colour state {k} [{a},{b})")
        if "by_variance" in mode:
            M, ns = np.empty((b - a, ny, nx), np.float32), np.empty((b - a, ny, nx), np.int32)
            capi.check(capi.load().tsdf_hip_download_variance_state(v._need(), 0, 0, a, nx, ny, b - a, capi.as_f32p(M),
                                                                    ns.ctypes.data_as(C.POINTER(C.c_int32))), "download_variance_state")
            assert_same_f32(M, s.M, f"M [{a},{b})")
            assert np.array_equal(ns, s.nsample)
    v.close()
    print(f"\n{mode}: {np.prod(BIG, dtype=np.int64) / 1e9:.2f} G voxels, {n_frames} frames integrated in {t_int:.2f} s, test {time.time() - t0:.1f} s")
