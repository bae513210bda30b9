"""GPU tier: frame ingest (tsdf_hip_organize = the `integrate` program's units / zero->NaN / world->camera /
z-buffer reprojection, src/prog/integrate.cpp:559-618) vs the serial restatement in the oracle, then
integrateCloud on the staged frame vs the oracle fed with the oracle's organised frame.

From test_cases_match_the_oracle on: the clouds of tests/ingest_cases.py (points on and next to pixel boundaries,
denormal / infinite / overflowing coordinates, the int conversion's limits, unit scales and transforms that are not
finite, one pixel under 20 000 points, every stride) at five image sizes down to 1 x 1, against the oracle that
tests/test_oracle_ingest.py pins to a plain model; and the life of the staged frame (include/tsdf_hip.h,
tsdf_hip_organize) on one handle and on a two-slab set.  Bar: bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection time, before the library brings in the HIP runtime (see tests/test_multi_gpu.py)

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests import ingest_cases as ic
from tests.common import assert_same_f32, make_volume

pytestmark = pytest.mark.gpu


def unorganised_cloud(sc, trans, seed, units=1.0, world=None, zeros=False):
    """Back-project a synthetic depth image to a shuffled point list with everything the loop has to cope with:
    several points per pixel (incl. exact z ties with different colours), NaN / zero / negative / infinite
    coordinates, points outside the image."""
    rng = np.random.RandomState(seed)
    dep = sc.depth(trans).astype(np.float64)
    v, u = np.nonzero(np.isfinite(dep))
    z = dep[v, u]
    # jitter inside the pixel so that truncation still lands in (u, v)
    uu = u + rng.uniform(0.05, 0.95, u.size)
    vv = v + rng.uniform(0.05, 0.95, v.size)
    pts = np.stack([(uu - sc.cx) / sc.fx * z, (vv - sc.cy) / sc.fy * z, z], 1)
    farther = pts[rng.choice(len(pts), len(pts) // 3)] * rng.uniform(1.0, 1.5, (len(pts) // 3, 1))  # same rays, hidden
    ties = pts[rng.choice(len(pts), len(pts) // 10)].copy()                                           # exact duplicates
    junk = np.array([[np.nan, 0, 1], [0, 0, 0], [0.1, 0.1, -1.0], [np.inf, 0, 2], [5, 5, 0.1], [0, 0, np.nan],
                     [0, 0, np.inf], [1e30, 1e30, 1e-30]], np.float64)
    if zeros:
        junk = np.concatenate([junk, np.zeros((50, 3))])
    allp = np.concatenate([pts, farther, ties, junk])
    if world is not None:  # express the same points in the world frame
        allp = np.where(np.isfinite(allp).all(1, keepdims=True), allp @ world[:3, :3].T + world[:3, 3], allp)
    allp = allp / units
    order = rng.permutation(len(allp))
    xyz = np.zeros((len(allp), 8), np.float32)  # PCL PointXYZRGBA: 8 floats per point
    xyz[:, :3] = allp[order]
    bgra = rng.randint(0, 256, (len(allp), 32)).astype(np.uint8)  # colour bytes every 32 bytes
    return xyz, bgra


@pytest.mark.parametrize("case", ["camera", "units", "world", "zero_nans"])
def test_organize_matches_serial_loop_and_feeds_integrate(gpu, case):
    vol, sc = make_volume(64, 160, 120, color=True)
    vol.reset()
    ov = OracleVolume(vol._p)
    for i in range(3):
        tr = synth.turntable_pose(i, 8, sc.size)
        units = 0.001 if case == "units" else 1.0
        world = synth.look_at_pose((0.3, -0.2, 0.9), target=(0.05, 0.0, 0.1)) if case == "world" else None
        xyz, bgra = unorganised_cloud(sc, tr, 10 + i, units=units, world=world, zeros=(case == "zero_nans"))
        w2c = np.linalg.inv(world) if world is not None else None
        kw = dict(units=units, zero_nans=(case == "zero_nans"), world_to_cam=w2c)
        d_ref, c_ref, n_ref = ov.organize(xyz, bgra[:, :4].copy(), **kw)
        d_gpu, c_gpu, n_gpu = vol.organize(xyz, bgra, cloud_units=units, zero_nans=(case == "zero_nans"), world_to_cam=w2c)
        assert n_ref == n_gpu and n_ref > 5000
        assert_same_f32(d_gpu, d_ref, f"organised depth, frame {i}")
        filled = np.isfinite(d_ref)
        assert np.array_equal(c_gpu[filled], c_ref[filled]), "colour of the z-buffer winners (incl. ties -> first point)"
        assert (c_gpu[~filled] == [0, 0, 0, 255]).all()
        n_obs = vol.integrateStaged(tr, count=True)
        assert n_obs == ov.integrate(d_ref, c_ref, synth.cam_from_vol_f32(tr))
    d, w, rgb = vol.download()
    assert_same_f32(d, ov.d, "d")
    assert np.array_equal(w, ov.w) and np.array_equal(rgb, ov.rgb)


def test_organize_empty_cloud_and_stride3(gpu):
    vol, sc = make_volume(32, 80, 60)
    vol.reset()
    with pytest.raises(Exception):
        vol.integrateStaged(np.eye(4))  # nothing staged yet
    d, c, n = vol.organize(np.zeros((0, 3), np.float32))
    assert n == 0 and np.isnan(d).all()
    pts = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.5], [0.0, 0.0, 0.5]], np.float32)  # tightly packed xyz, no colour
    d, c, n = vol.organize(pts)
    assert n == 1 and np.nanmin(d) == np.float32(0.5)
    ov = OracleVolume(vol._p)
    d2, _, n2 = ov.organize(pts)
    assert n2 == 1
    assert_same_f32(d, d2, "depth")


# ---- the clouds of tests/ingest_cases.py ---------------------------------------------------------------------------------
RES = 32
SIZE_IDS = [f"{w}x{h}" for w, h in ic.SIZES]
# every image size is handed to setImageSize as it is: create accepts any positive size, 1 x 1 included


def product(size, color=True, devices=None, mode=None, pairing=False):
    """A reset 32^3 volume for image `size` with the camera of ic.scene(*size); (volume, scene, pose to integrate from)."""
    vol, sc = make_volume(RES, size[0], size[1], color=color)
    assert (sc.fx, sc.fy, sc.cx, sc.cy) == ic.scene(*size)[2:]
    if mode:
        vol.setColorMode(mode)
    vol.setDevices(devices)
    vol.setFramePairing(pairing)
    vol.reset()
    return vol, sc, synth.turntable_pose(1, 8, sc.size)


def clear(vol):
    """tsdf_hip_reset on the living handle (TSDFVolumeOctree.reset() makes a new one)."""
    capi.check(capi.load().tsdf_hip_reset(vol._need()), "reset")


def kw_product(kw):
    return dict(cloud_units=kw.get("units", 1.0), zero_nans=kw.get("zero_nans", False), world_to_cam=kw.get("world_to_cam"))


def contiguous(a):
    return None if a is None else np.ascontiguousarray(a)


def assert_frame(got, want, what):
    (d, c, n), (d2, c2, n2) = got, want
    assert_same_f32(d, d2, f"{what}: organised depth")
    assert np.array_equal(np.signbit(d), np.signbit(d2)), what
    assert n == n2, (what, n, n2)
    filled = ~np.isnan(d2)
    assert np.array_equal(c[filled], c2[filled]), f"{what}: colours of the z-buffer winners"
    assert (c[~filled] == [0, 0, 0, 255]).all(), f"{what}: empty pixels"


def assert_grid(vol, ov, what):
    d, w, rgb = vol.download()
    assert_same_f32(d, ov.d, f"{what}: d")
    assert np.array_equal(w, ov.w), f"{what}: w"
    if ov.rgb is not None:
        assert np.array_equal(rgb, ov.rgb), f"{what}: rgb"


def run_case(vol, case, tr, what, fetch=True):
    """organize (+ integrateStaged where the frame has a pixel in the volume's view, ic.feeds_integrate) on a cleared
    volume against the oracle; returns whether the frame was integrated."""
    clear(vol)
    ov = OracleVolume(vol._p)
    want = ov.organize(case.xyz, contiguous(case.bgra), **case.kw)
    got = vol.organize(case.xyz, case.bgra, fetch=fetch, **kw_product(case.kw))
    if fetch:
        assert_frame(got, want, what)
    if not ic.feeds_integrate(want[0], vol._p.max_sensor_dist):
        return False
    n = vol.integrateStaged(tr, count=True)
    # (the product hands the reference's frustum cull over with every pose; under the 65 x 3, 257 x 1 and 1 x 1 cameras it drops voxels)
    planes = ov.reference_cull_planes(tr)
    assert n == ov.integrate(want[0], want[1] if case.color else None, synth.cam_from_vol_f32(tr), planes=planes), what
    assert_grid(vol, ov, what)
    return True


@pytest.mark.parametrize("group", ic.GROUPS)
@pytest.mark.parametrize("size", ic.SIZES, ids=SIZE_IDS)
def test_cases_match_the_oracle(gpu, size, group):
    s = ic.scene(*size)
    vols, fed = {}, set()
    for c in [c for c in ic.cases(s) if c.group == group]:
        if c.color not in vols:
            vols[c.color] = product(size, c.color)
        vol, _, tr = vols[c.color]
        if run_case(vol, c, tr, f"{c.name} at {size}"):
            fed.add(c.name)
    # the cases whose frame must have gone through integrateStaged as well, at every image size
    must = {"pixel_edges": {"pixel_edges"}, "extremes": {"extremes"}, "one_pixel": {"one_pixel"}, "sizes": {"n4097"},
            "strides": {c.name for c in ic.cases(s) if c.group == "strides"}, "units": {"units_-1_pixel_edges"}}.get(group, set())
    assert must <= fed, (must - fed, fed)
    for vol, _, _ in vols.values():
        vol.close()


def test_organize_refuses_bad_strides_and_a_null_cloud(gpu):
    vol, _, _ = product((7, 5))
    lib, h = capi.load(), vol._need()
    xyz, bgra = np.zeros((4, 3), np.float32), np.zeros((4, 4), np.uint8)
    nv = C.c_uint64(0)

    def call(pts, xs, col, cs, n):
        return lib.tsdf_hip_organize(h, capi.as_f32p(pts) if pts is not None else None, xs, capi.as_u8p(col) if col is not None else None,
                                     cs, n, 1.0, 0, None, None, None, C.byref(nv))
    assert call(xyz, 2, bgra, 4, 4) == capi.E_INVALID
    assert call(xyz, 3, bgra, 3, 4) == capi.E_INVALID
    assert call(None, 3, None, 0, 4) == capi.E_INVALID
    with pytest.raises(capi.TsdfHipError, match="no organised frame is staged"):
        vol.integrateStaged(np.eye(4))   # none of the refused calls staged anything
    assert call(None, 3, None, 0, 0) == capi.OK and nv.value == 0   # an empty cloud needs no pointer
    vol.close()


@pytest.mark.parametrize("name", ["pixel_edges", "one_pixel", "extremes"])
def test_asynchronous_organize_equals_the_fetched_form(gpu, name):
    """fetch=False (no output pointer: nothing synchronises between organize and integrateStaged) against the oracle,
    and so against the fetched form that test_cases_match_the_oracle holds to the same oracle; on a second volume."""
    size = (160, 120)
    case = next(c for c in ic.cases(ic.scene(*size)) if c.name == name)
    a, _, tr = product(size)
    b, _, _ = product(size)
    assert run_case(a, case, tr, f"{name}, fetched") and run_case(b, case, tr, f"{name}, asynchronous", fetch=False)
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    a.close()
    b.close()


def test_scratch_is_reused_across_cloud_sizes(gpu):
    """One handle: a 10-point cloud, a 60 000-point cloud, the small one, the large one again (the scratch holds
    z-buffer | points | colours; the second call regrows it, the later ones reuse it; nothing of an earlier cloud or
    z-buffer may show in a later frame)."""
    size = (160, 120)
    s = ic.scene(*size)
    by_name = {c.name: c for c in ic.cases(s)}
    op, pe = by_name["one_pixel"], by_name["pixel_edges"]
    big_xyz = np.concatenate([op.xyz, pe.xyz, pe.xyz[::-1], pe.xyz[::2]])[:60000]
    big_bgra = np.concatenate([op.bgra, pe.bgra, pe.bgra[::-1], pe.bgra[::2]])[:60000]
    assert len(big_xyz) == 60000
    small = ic.Case("small", "scratch", ic.pad(ic.ordinary(s, 10, seed=77)), ic.colours(10, salt=77), {}, True)
    big = ic.Case("big", "scratch", big_xyz, big_bgra, {}, True)
    vol, _, tr = product(size)
    for i, c in enumerate((small, big, small, big)):
        assert run_case(vol, c, tr, f"cloud {i} ({c.name})")
    vol.close()


def test_pinned_caller_memory_gives_the_same_frame(gpu):
    """xyz in pinned host memory (capi.PinnedArray: the library copies from it directly, without its bounce buffer)."""
    size = (65, 3)
    case = next(c for c in ic.cases(ic.scene(*size)) if c.name == "stride_xyz5_c32")
    vol, _, tr = product(size)
    ov = OracleVolume(vol._p)
    want = ov.organize(case.xyz, contiguous(case.bgra))
    pin = capi.PinnedArray(case.xyz.shape, np.float32)
    pin.array[:] = case.xyz
    got_pinned = vol.organize(pin.array, case.bgra)
    got_pageable = vol.organize(case.xyz.copy(), case.bgra)
    assert_frame(got_pinned, want, "pinned")
    assert_frame(got_pageable, want, "pageable")
    assert np.array_equal(got_pinned[0].view(np.uint32), got_pageable[0].view(np.uint32)) and np.array_equal(got_pinned[1], got_pageable[1])
    pin.free()
    vol.close()


@pytest.mark.parametrize("mode", [None, "LAB", "RGBNormalized"])
def test_staged_frame_integrated_twice_from_two_poses(gpu, mode):
    """The staged frame outlives integrateStaged: two calls with two poses equal the oracle fed the frame twice; on the
    default colour volume and on the two colour modes of tests/mode_cases.py."""
    from tests import mode_cases
    from tests.sequence_model import Model
    assert mode is None or mode in mode_cases.COLOUR_MODES
    size = (160, 120)
    vol, sc, _ = product(size, mode=mode)
    model = Model(vol._p, mode, cull=True)   # (the product hands the reference's cull planes over with every frame)
    xyz, bgra = unorganised_cloud(sc, synth.turntable_pose(0, 8, sc.size), 41)
    want = model.ov.organize(xyz, bgra[:, :4].copy())
    assert_frame(vol.organize(xyz, bgra), want, "frame")
    for i in (0, 3):
        tr = synth.turntable_pose(i, 8, sc.size)
        assert vol.integrateStaged(tr, count=True) == model.integrate(want[0], want[1], tr) > 1000
    assert_grid(vol, model.ov, f"mode {mode}")
    vol.close()


# ---- life of the staged frame --------------------------------------------------------------------------------------------
# Between organize(A) and integrateStaged: (a) integrateCloud of a host frame B, (b) a device frame B whose colour image
# does not lie behind its depth image, (c) tsdf_hip_reset, (d) a pipelined host frame B (tsdf_hip_integrate_async =
# frame_begin + commit).  The rule (include/tsdf_hip.h): the staged frame is valid until a call writes the handle's frame
# staging, or until reset; then integrateStaged refuses.  (a), (b), (c) write it on both kinds of handle.  (d) does not on
# one handle -- the pipelined frame goes through the handle's ring, A stays where it was and is integrated after B -- and
# does on a set, whose unpaired commit uploads into every slab's staging; with frame pairing on, the set's commit goes
# through the slabs' rings as well and the two kinds agree (B is held back for a partner and launched by integrateStaged,
# before A).  Never may the volume hold B twice.
LIFE = {("one", "a"): "refused", ("one", "b"): "refused", ("one", "c"): "refused", ("one", "d"): "integrated",
        ("set", "a"): "refused", ("set", "b"): "refused", ("set", "c"): "refused", ("set", "d"): "refused",
        ("one_paired", "d"): "integrated", ("set_paired", "d"): "integrated"}


@pytest.fixture(scope="module")
def life_frames():
    """Frame A (a cloud and its organised form), host frame B, and the oracle's grids after B, after B then A, after B
    twice, and after A alone -- computed once."""
    size = (160, 120)
    vol, sc = make_volume(RES, *size, color=True)
    p = vol._p
    tr_a, tr_b = synth.turntable_pose(0, 8, sc.size), synth.turntable_pose(2, 8, sc.size)
    xyz, bgra = unorganised_cloud(sc, tr_a, 51)
    A = OracleVolume(p).organize(xyz, bgra[:, :4].copy())
    B = (sc.depth(tr_b, noise_seed=9), sc.bgra(5))
    grids = {}
    for key, seq in (("B", [(B, tr_b)]), ("BA", [(B, tr_b), (A, tr_a)]), ("BB", [(B, tr_b), (B, tr_a)]), ("A", [(A, tr_a)]), ("", [])):
        ov = OracleVolume(p)
        for f, tr in seq:
            ov.integrate(f[0], f[1], synth.cam_from_vol_f32(tr))
        grids[key] = ov
    differ = lambda x, y: not np.array_equal(grids[x].d.view(np.uint32), grids[y].d.view(np.uint32))  # noqa: E731
    assert differ("BB", "BA") and differ("BB", "B") and differ("BA", "B") and differ("A", "")
    return dict(size=size, xyz=xyz, bgra=bgra, A=A, B=B, tr_a=tr_a, tr_b=tr_b, grids=grids)


def same_grid(vol, ov):
    d, w, rgb = vol.download()
    return np.array_equal(d.view(np.uint32), ov.d.view(np.uint32)) and np.array_equal(w, ov.w) and np.array_equal(rgb, ov.rgb)


@pytest.mark.parametrize("kind,step", list(LIFE), ids=[f"{k}-{s}" for k, s in LIFE])
def test_life_of_the_staged_frame(gpu, life_frames, kind, step):
    L = life_frames
    vol, sc, _ = product(L["size"], devices=[0, 0] if kind.startswith("set") else None, pairing=kind.endswith("_paired"))
    assert len(vol.slabs()) == (2 if kind.startswith("set") else 1)
    assert_frame(vol.organize(L["xyz"], L["bgra"]), L["A"], "frame A")
    dep, col = L["B"]
    if step == "a":
        vol.integrateCloud(dep, col, L["tr_b"])
    elif step == "b":   # one allocation, the colour image IN FRONT of the depth image
        buf = torch.empty((2, dep.size), dtype=torch.float32, device="cuda:0")
        buf[0].view(torch.uint8).copy_(torch.from_numpy(col.reshape(-1)))
        buf[1].copy_(torch.from_numpy(dep.reshape(-1)))
        torch.cuda.synchronize()
        vol.integrateCloudDevice(buf[1].data_ptr(), buf[0].data_ptr(), L["tr_b"])
        vol.synchronize()
    elif step == "c":
        clear(vol)
    else:
        vol.integrateCloud(dep, col, L["tr_b"], pipelined=True)
    before = "" if step == "c" else "B"
    try:
        vol.integrateStaged(L["tr_a"])
        outcome = "integrated"
    except capi.TsdfHipError as e:
        assert e.code == capi.E_INVALID and "no organised frame is staged" in str(e), e
        outcome = "refused"
    vol.synchronize()
    assert not same_grid(vol, L["grids"]["BB"]), "the frame that took the staged frame's place was integrated a second time"
    want = before if outcome == "refused" else ("A" if step == "c" else "BA")
    assert_grid(vol, L["grids"][want], f"{kind} ({step}): integrateStaged {outcome}")
    assert outcome == LIFE[kind, step], (kind, step, outcome)
    # organize stages a frame again whatever came before
    assert_frame(vol.organize(L["xyz"], L["bgra"]), L["A"], "frame A again")
    vol.integrateStaged(L["tr_a"])
    ov = OracleVolume(vol._p)
    for key in want + "A":
        f, tr = (L["B"], L["tr_b"]) if key == "B" else (L["A"], L["tr_a"])
        ov.integrate(f[0], f[1], synth.cam_from_vol_f32(tr))
    assert_grid(vol, ov, f"{kind} ({step}): after a new organize")
    vol.close()


def test_calls_that_take_no_frame_leave_the_staged_frame_valid(gpu, life_frames):
    """Queries, a download and the cull setter between organize and integrateStaged, on both kinds of handle."""
    L = life_frames
    for devices in (None, [0, 0]):
        vol, sc, _ = product(L["size"], devices=devices)
        vol.organize(L["xyz"], L["bgra"], fetch=False)
        vol.download()
        vol.renderView(L["tr_b"], 4)
        vol.synchronize()
        vol.integrateStaged(L["tr_a"])
        assert_grid(vol, L["grids"]["A"], f"devices {devices}")
        vol.close()


@pytest.mark.parametrize("name", ["pixel_edges", "extremes", "one_pixel"])
@pytest.mark.parametrize("size", [(160, 120), (7, 5), (257, 1)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_two_slab_set_equals_one_handle(gpu, size, name):
    case = next(c for c in ic.cases(ic.scene(*size)) if c.name == name)
    one, _, tr = product(size)
    two, _, _ = product(size, devices=[0, 0])
    f1 = one.organize(case.xyz, case.bgra)
    f2 = two.organize(case.xyz, case.bgra)
    assert_frame(f2, f1, f"{name} at {size}: set against one handle")
    assert np.array_equal(f1[1], f2[1])
    assert one.integrateStaged(tr, count=True) == two.integrateStaged(tr, count=True)
    for x, y in zip(one.download(), two.download()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert run_case(two, case, tr, f"{name} at {size}: set against the oracle")
    one.close()
    two.close()
