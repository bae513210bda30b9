"""GPU tier: tsdf_hip_shift (cpu_tsdf_amd/csrc/tsdf_shift.hip, tsdf_multi.hip) -- the volume's window moved by whole voxels,
in place.  Every expectation is tests/shift_cases.shifted (a numpy roll with the reset values as fill) applied to the arrays
download() returned BEFORE the shift, compared bit for bit; the band flags are checked through what their readers do
(reconstruct, getOccupiedVoxelIndices, the implied distances of integrateCloud) against a twin volume that received the
rolled arrays through upload() and therefore reads everything."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  at collection time, before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree
from tests import shift_cases as sc_
from tests.common import assert_same_f32, frames, make_volume

pytestmark = pytest.mark.gpu


def same_volume(got, want, what):
    assert_same_f32(got[0], want[0], what + ": d")
    assert_same_f32(got[1], want[1], what + ": w")
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]), what + ": rgb"


def shift_raw(lib, vol, s):
    return lib.tsdf_hip_shift(vol._need(), (C.c_int32 * 3)(*s))


# ---- 1. data movement, every layout ------------------------------------------------------------------------------------
RES3 = (130, 10, 7)  # three flag cells in x (the last partial), pitch 132 != nx, a partial cell in y
XS, YS, ZS = [0, 1, -1, 3, -3, 64, -64, 65, -65, 130, -200], [0, 1, -1, 4, -4, 5, -5, 10], [0, 1, -1, 2, -2, 7]
SHIFTS = ([(x, 0, 0) for x in XS if x] + [(0, y, 0) for y in YS if y] + [(0, 0, z) for z in ZS if z] +
          [(5, 3, 2), (-65, -5, -1), (64, 4, 1), (1, 0, 1), (0, -4, 2), (-3, 5, 0), (130, 1, 1), (1, 10, -1), (-1, -1, 7)])
LAYOUTS = [(capi.LAYOUT_PACKED, True), (capi.LAYOUT_PACKED, False), (capi.LAYOUT_F32W, True), (capi.LAYOUT_F32W, False)]


def random_volume(rng, color, max_weight):
    shape = RES3[::-1]
    d = rng.uniform(-1.2, 1.2, shape).astype(np.float32)
    w = rng.randint(0, int(max_weight) + 1, shape).astype(np.float32)
    rgb = rng.randint(0, 256, shape + (3,)).astype(np.uint8) if color else None
    return d, w, rgb


@pytest.mark.parametrize("layout,color", LAYOUTS)
def test_data_movement_in_every_layout(gpu, layout, color):
    vol, _ = make_volume(RES3[0], 80, 60, color=color, res3=RES3, max_weight=3.0)
    vol.setLayout(layout)
    vol.reset()
    assert vol.getLayout() == layout
    rng = np.random.RandomState(7 + layout + 2 * color)
    n = RES3[0] * RES3[1] * RES3[2]
    for s in SHIFTS:
        vol.upload(*random_volume(rng, color, 3.0))
        before = vol.download()
        vol.shiftVolume(*s)
        same_volume(vol.download(), sc_.shifted_volume(*before, s), f"shift {s}")
        st = vol.shiftStats()
        assert st[0] + st[1] == n and st[1] == sc_.reset_count(before[0].shape, s), (s, st)
        assert st[2] == 0  # (uploaded planes: no flags to carry)
    # two shifts in a row == the composition of the helper (what left the grid does not come back)
    for s1, s2 in [((5, 3, 2), (-5, -3, -2)), ((-65, 0, 1), (64, 4, -1)), ((0, 0, 1), (0, 0, 1)), ((3, 0, 0), (0, -4, 0))]:
        vol.upload(*random_volume(rng, color, 3.0))
        before = vol.download()
        vol.shiftVolume(*s1)
        vol.shiftVolume(*s2)
        same_volume(vol.download(), sc_.shifted_volume(*sc_.shifted_volume(*before, s1), s2), f"shifts {s1} then {s2}")
    vol.close()


# ---- 2. colour and variance state ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["RGBNormalized", "LAB"])
def test_float_colour_state_moves_with_the_voxels(gpu, mode):
    vol, sc = make_volume(32, 80, 60, color=True)
    vol.setColorMode(mode)
    vol.reset()
    for i, tr, dep, col in frames(sc, 3, 8):
        vol.integrateCloud(dep, col, tr)
    before, state = vol.download(), vol.downloadColorState()
    assert (before[1] > 0).sum() > 1000 and state.any()
    s = (3, -2, 1)
    vol.shiftVolume(*s)
    same_volume(vol.download(), sc_.shifted_volume(*before, s), mode)
    got = vol.downloadColorState()
    assert got.shape == state.shape
    for c in range(len(state)):
        assert_same_f32(got[c], sc_.shifted(state[c], s, sc_.FILL_STATE), f"{mode} state plane {c}")
    vol.close()


def test_variance_state_moves_with_the_voxels(gpu):
    vol, sc = make_volume(32, 80, 60)
    vol.setLayout(capi.LAYOUT_F32W)
    vol.setWeighting(False, True)
    vol.reset()
    rng = np.random.RandomState(11)
    shape = (32, 32, 32)
    d, w = rng.uniform(-1, 1, shape).astype(np.float32), rng.uniform(0, 9, shape).astype(np.float32)
    M, ns = rng.uniform(0, 2, shape).astype(np.float32), rng.randint(0, 20, shape).astype(np.int32)
    vol.upload(d, w)
    vol.uploadVarianceState(M, ns)
    s = (3, -2, 1)
    vol.shiftVolume(*s)
    gM, gns = vol.downloadVarianceState()
    assert_same_f32(gM, sc_.shifted(M, s, sc_.FILL_STATE), "M")
    assert np.array_equal(gns, sc_.shifted(ns, s, sc_.FILL_STATE)), "nsample"
    same_volume(vol.download(), sc_.shifted_volume(d, w, None, s), "variance volume")
    vol.close()


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one_handle", "set_0_0_0"])
def test_variance_state_moves_over_the_whole_shift_list(gpu, devices):
    """M and nsample on RES3 (three flag cells in x, pitch != nx), fresh random values before every shift: every path of the
    shift kernels moves the float and the int32 plane and fills with zeros.  On a set (slabs of 3, 2, 2 planes) the z
    shifts pull both planes between the slabs."""
    vol, _ = make_volume(RES3[0], 80, 60, res3=RES3, max_weight=9.0)
    vol.setLayout(capi.LAYOUT_F32W)
    vol.setWeighting(False, True)
    vol.setDevices(devices)
    vol.reset()
    rng = np.random.RandomState(23)
    shape = RES3[::-1]
    for s in (SHIFTS if devices is None else MULTI_SHIFTS):
        M, ns = rng.uniform(0.5, 2, shape).astype(np.float32), rng.randint(1, 20, shape).astype(np.int32)
        vol.uploadVarianceState(M, ns)
        vol.shiftVolume(*s)
        gM, gns = vol.downloadVarianceState()
        assert_same_f32(gM, sc_.shifted(M, s, sc_.FILL_STATE), f"M, shift {s}")
        assert np.array_equal(gns, sc_.shifted(ns, s, sc_.FILL_STATE)), f"nsample, shift {s}"
    vol.close()


FLAT3 = (70, 36, 45)  # pitch 72 != nx, a partial second flag cell in x, ny no multiple of the 4-row cell
COLOUR_STATE_SHIFTS = [(1, 0, 0), (-1, 0, 0), (64, 0, 0), (-64, 0, 0), (65, 0, 0), (0, -5, 0), (0, 0, 16), (3, -2, 1), (-65, 4, -2),
                       (5, 3, 2), (0, 4, -1)]


@pytest.mark.parametrize("mode", ["RGBNormalized", "LAB"])
def test_float_colour_state_moves_on_a_flat_grid(gpu, mode):
    """The float colour planes (no upload exists for them: three fused frames) over pure x shifts of +-1, +-64 and 65, a pure
    y, a pure z and mixed shifts, on a grid whose pitch is not nx; re-fused after a reset() where a shift emptied the grid."""
    size = synth.scene_a(FLAT3[0], 80, 60).size
    vol, sc = make_volume(FLAT3[0], 80, 60, color=True, res3=FLAT3, size3=tuple(size * r / FLAT3[0] for r in FLAT3))
    vol.setColorMode(mode)

    def fuse():
        vol.reset()
        for i, tr, dep, col in frames(sc, 3, 8):
            vol.integrateCloud(dep, col, tr)
    fuse()
    fused, full = 1, int((vol.download()[1] > 0).sum())
    for s in COLOUR_STATE_SHIFTS:
        before, state = vol.download(), vol.downloadColorState()
        if (before[1] > 0).sum() < full // 2:   # (the shifts by a whole flag cell and back left six columns)
            fuse()
            fused += 1
            before, state = vol.download(), vol.downloadColorState()
        assert (before[1] > 0).sum() > 1000 and all(plane.any() for plane in state)
        vol.shiftVolume(*s)
        same_volume(vol.download(), sc_.shifted_volume(*before, s), f"{mode}, shift {s}")
        got = vol.downloadColorState()
        assert got.shape == state.shape == ({"RGBNormalized": 4, "LAB": 3}[mode],) + FLAT3[::-1]
        for c in range(len(state)):
            assert_same_f32(got[c], sc_.shifted(state[c], s, sc_.FILL_STATE), f"{mode} state plane {c}, shift {s}")
    assert fused >= 2
    vol.close()


# ---- 3. the flags survive and still mean something ------------------------------------------------------------------------
SIDE = dict(first=8, total=44)  # the frames of tests/test_occupied_gpu.py: from one side, so that cells stay without a flag


@pytest.fixture(scope="module")
def side_frames():
    sc = synth.scene_a(128, 160, 120)
    out = []
    for i in range(SIDE["first"], SIDE["first"] + 7):  # six to fuse, one more for after the shift
        tr = synth.turntable_pose(i, SIDE["total"], sc.size)
        out.append((tr, sc.depth(tr), sc.bgra(i)))
    return out


def fused128(color, side_frames):
    vol, _ = make_volume(128, color=color)
    vol.reset()
    assert vol.getLayout() == capi.LAYOUT_PACKED
    n = 0
    for tr, dep, col in side_frames[:6]:
        n = vol.integrateCloud(dep, col if color else None, tr, count=True)
    assert n > 0
    return vol


def march(vol, color):
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(color)
    mesh = mc.reconstruct(want_cells=True)
    st = (C.c_uint64 * 4)()
    capi.check(capi.load().tsdf_hip_march_stats(vol._need(), st), "march_stats")
    return mesh, [int(v) for v in st]


def read_detail(vol):
    out = (C.c_uint64 * 3)()
    capi.check(capi.load().tsdf_hip_last_read_detail(vol._need(), out), "last_read_detail")
    return [int(v) for v in out]


@pytest.mark.parametrize("s", [(64, 4, 1), (5, 3, 2), (0, 0, -3), (-7, 0, 0)])
@pytest.mark.parametrize("color", [True, False])
def test_flags_survive_and_still_mean_something(gpu, side_frames, color, s):
    vol = fused128(color, side_frames)
    implied_before = read_detail(vol)[1]
    mesh0, _ = march(vol, color)
    occ0 = vol.getOccupiedVoxelIndices()
    st0 = vol.occupiedStats()
    assert len(mesh0["cells"]) > 0 and len(occ0) > 0 and st0[2] == 1
    before = vol.download()
    moved = vol.shiftVolume(*s)
    assert np.array_equal(moved, np.array(s, np.float64) * float(vol._p.size[0]) / 128)
    sst = vol.shiftStats()
    assert sst[2] == 1 and sst[0] + sst[1] == 128 ** 3 and sst[1] == sc_.reset_count(before[0].shape, s), sst
    want = sc_.shifted_volume(*before, s)
    same_volume(vol.download(), want, f"shift {s}")
    twin, _ = make_volume(128, color=color)
    twin.reset()
    twin.upload(*want)
    twin.setGlobalTransform(vol.getGlobalTransform())
    # (a) the same mesh, read through the flags on the shifted handle
    mesh, mst = march(vol, color)
    tmesh, tst = march(twin, color)
    assert mst[3] & 1 == 1 and tst[3] & 1 == 0, (mst, tst)
    assert len(mesh["cells"]) > 0 and np.array_equal(mesh["cells"], tmesh["cells"])
    assert_same_f32(mesh["vertices"], tmesh["vertices"], "mesh vertices")
    if color:
        assert np.array_equal(mesh["rgb"], tmesh["rgb"])
    if s == (64, 4, 1):
        assert len(mesh["cells"]) < len(mesh0["cells"])
    # (b) the same occupied list, scanned through the flags on the shifted handle
    attrs = ("d", "w", "rgb") if color else ("d", "w")
    a, b = vol.getOccupiedVoxelIndices(want=attrs), twin.getOccupiedVoxelIndices(want=attrs)
    st, tst = vol.occupiedStats(), twin.occupiedStats()
    assert 1 <= len(a[0]) <= len(occ0)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert st[2] == 1 and st[1] < 128 ** 3 * 4 and tst[2] == 0 and tst[1] == 128 ** 3 * 4, (st, tst)
    if s == (64, 4, 1):
        assert st[1] <= st0[1], (st, st0)  # an aligned shift maps cells onto cells: they can only drop out
    # (c) one more frame into both, at the pose that looks at the same world point as before
    tr, dep, col = side_frames[6]
    t = np.eye(4)
    t[:3, 3] = -moved
    na = vol.integrateCloud(dep, col if color else None, t @ tr, count=True)
    da = read_detail(vol)
    nb = twin.integrateCloud(dep, col if color else None, t @ tr, count=True)
    db = read_detail(twin)
    assert na == nb and na > 0
    same_volume(vol.download(), twin.download(), f"one more frame after shift {s}")
    if implied_before:
        assert da[1] == 1, da
    assert db[1] == 0, db
    vol.close()
    twin.close()


def test_implied_distances_were_on_before_the_shift(gpu, side_frames):
    """The precondition of (c) above: the PACKED launches of the fuse recipe do run with implied distances."""
    for color in (True, False):
        vol = fused128(color, side_frames)
        assert read_detail(vol)[1] == 1
        vol.close()


# ---- 4. a list made before the shift is stale ------------------------------------------------------------------------------
def test_occupied_list_is_stale_after_a_shift(gpu, side_frames):
    lib = gpu
    vol = fused128(True, side_frames)
    h = vol._need()
    n = C.c_uint64(0)
    capi.check(lib.tsdf_hip_occupied(h, None, C.byref(n)), "occupied")
    idx = np.empty((int(n.value), 3), np.int32)
    p = idx.ctypes.data_as(C.POINTER(C.c_int32))
    assert n.value > 0 and lib.tsdf_hip_occupied_fetch(h, p, None, None, None) == capi.OK
    vol.shiftVolume(1, 0, 0)
    assert lib.tsdf_hip_occupied_fetch(h, p, None, None, None) == capi.E_INVALID
    assert lib.tsdf_hip_occupied_fetch_device(h, None, None, None, None) == capi.E_INVALID
    capi.check(lib.tsdf_hip_occupied(h, None, C.byref(n)), "occupied")
    idx2 = np.empty((int(n.value), 3), np.int32)
    assert lib.tsdf_hip_occupied_fetch(h, idx2.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None) == capi.OK
    assert 0 < len(idx2) <= len(idx) and idx2[:, 0].max() < 127
    vol.close()


# ---- 5. a multi-GPU set equals one handle -----------------------------------------------------------------------------------
MULTI_SHIFTS = [(0, 0, 1), (0, 0, -5), (3, -2, 2), (0, 0, 12)]


@pytest.mark.parametrize("layout,color", [(capi.LAYOUT_PACKED, True), (capi.LAYOUT_F32W, False)])
def test_multi_set_equals_one_handle_on_uploaded_content(gpu, layout, color):
    res3 = (70, 9, 12)
    rng = np.random.RandomState(5)
    shape = res3[::-1]
    for s in MULTI_SHIFTS + [(0, 0, 5), (-3, 2, -2), (0, 0, -12), (2, 1, 0)]:
        vols = []
        for devices in (None, [0, 0, 0]):
            v, _ = make_volume(res3[0], 80, 60, color=color, res3=res3, max_weight=3.0)
            v.setLayout(layout)
            v.setDevices(devices)
            v.reset()
            vols.append(v)
        assert [x[2] - x[1] for x in vols[1].slabs()] == [4, 4, 4]
        d = rng.uniform(-1.2, 1.2, shape).astype(np.float32)
        w = rng.randint(0, 4, shape).astype(np.float32)
        rgb = rng.randint(0, 256, shape + (3,)).astype(np.uint8) if color else None
        for v in vols:
            v.upload(d, w, rgb)
            v.shiftVolume(*s)
        want = sc_.shifted_volume(d, w, rgb, s)
        same_volume(vols[0].download(), want, f"single handle, shift {s}")
        same_volume(vols[1].download(), want, f"three slabs, shift {s}")
        assert vols[1].shiftStats()[:3] == vols[0].shiftStats()[:3]
        for v in vols:
            v.close()


@pytest.mark.parametrize("s", MULTI_SHIFTS + [(0, 0, -47)])
def test_multi_set_equals_one_handle_on_the_fused_scene(gpu, side_frames, s):
    """128^3 over three slabs (43 / 43 / 42 planes): downloads, the mesh (read through the carried flags on both) and one
    more integrated frame -- which reads the halos only if they were marked stale and refreshed."""
    single = fused128(True, side_frames)
    multi, _ = make_volume(128, color=True)
    multi.setDevices([0, 0, 0])
    multi.reset()
    for tr, dep, col in side_frames[:6]:
        multi.integrateCloud(dep, col, tr)
    march(multi, True)  # (refreshes the one-plane halo: the shift has to mark it stale)
    ma, mb = single.shiftVolume(*s), multi.shiftVolume(*s)
    assert np.array_equal(ma, mb)
    assert single.shiftStats()[:3] == multi.shiftStats()[:3] and multi.shiftStats()[2] == 1
    same_volume(multi.download(), single.download(), f"shift {s}")
    m1, st1 = march(single, True)
    m2, st2 = march(multi, True)
    assert len(m1["cells"]) > 0 and np.array_equal(m1["cells"], m2["cells"]) and np.array_equal(m1["rgb"], m2["rgb"])
    assert_same_f32(m1["vertices"], m2["vertices"], "mesh vertices")
    assert st1[3] & 1 == 1
    tr, dep, col = side_frames[6]
    t = np.eye(4)
    t[:3, 3] = -ma
    assert single.integrateCloud(dep, col, t @ tr, count=True) == multi.integrateCloud(dep, col, t @ tr, count=True)
    same_volume(multi.download(), single.download(), f"one more frame after shift {s}")
    m1, _ = march(single, True)
    m2, _ = march(multi, True)
    assert np.array_equal(m1["cells"], m2["cells"])
    assert_same_f32(m1["vertices"], m2["vertices"], "mesh vertices after one more frame")
    pts = np.array([[0.01, 0.02, (z + 0.5) * single._p.size[2] / 128 - single._p.size[2] / 2] for z in (41.7, 42.6, 85.2, 86.4)], np.float32)
    for x, y in zip(single.sample(pts), multi.sample(pts)):  # trilinear samples across the seams: the halo planes
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    single.close()
    multi.close()


# ---- 6. errors and no-ops -------------------------------------------------------------------------------------------------
def test_errors_and_no_ops(gpu):
    lib = gpu
    vol, sc = make_volume(32, 80, 60, color=True)
    vol.reset()
    for i, tr, dep, col in frames(sc, 2, 8):
        vol.integrateCloud(dep, col, tr)
    before = vol.download()
    assert shift_raw(lib, vol, (0, 0, 0)) == capi.OK
    assert lib.tsdf_hip_shift(vol._need(), None) == capi.E_INVALID
    same_volume(vol.download(), before, "zero shift")
    assert np.array_equal(vol.shiftVolume(0, 0, 0), np.zeros(3)) and np.array_equal(vol.getGlobalTransform(), np.eye(4))
    vol.shiftVolume(0, -40, 0)  # |s| >= res: legal, everything is reset
    d, w, rgb = vol.download()
    assert (d == -1).all() and not w.any() and not rgb.any() and vol.shiftStats()[:2] == (0, 32 ** 3)
    vol.close()


def test_z_slab_handle_shifts_along_x_and_y_only(gpu):
    lib = gpu
    slab, sc = make_volume(32, 80, 60, color=True)
    slab.setZSlab(8, 20, halo=2)
    slab.reset()
    for i, tr, dep, col in frames(sc, 2, 8):
        slab.integrateCloud(dep, col, tr)
    rng = np.random.RandomState(2)
    halo = [rng.uniform(-1, 1, (2, 32, 32)).astype(np.float32), rng.randint(0, 5, (2, 32, 32)).astype(np.float32),
            rng.randint(0, 256, (2, 32, 32, 3)).astype(np.uint8)]
    slab.upload(*halo, z0=6)   # something to move in the halo planes too
    slab.upload(*halo, z0=20)
    before = slab.download(z0=6, nz=16)
    assert (before[1][2:14] > 0).sum() > 100
    assert shift_raw(lib, slab, (0, 0, 1)) == capi.E_UNSUPPORTED
    assert shift_raw(lib, slab, (2, 1, -3)) == capi.E_UNSUPPORTED
    same_volume(slab.download(z0=6, nz=16), before, "a refused shift changes nothing")
    slab.shiftVolume(2, 1, 0)
    same_volume(slab.download(z0=6, nz=16), sc_.shifted_volume(*before, (2, 1, 0)), "slab + halo, shift (2, 1, 0)")
    st = slab.shiftStats()
    assert st[0] + st[1] == 32 * 32 * 16 and st[1] == sc_.reset_count((16, 32, 32), (2, 1, 0))
    slab.close()


def test_a_frame_held_back_by_frame_pairing_is_integrated_before_the_shift(gpu):
    got = []
    for pairing in (False, True):
        vol, sc = make_volume(64, color=True)
        vol.setFramePairing(pairing)
        vol.reset()
        for i, tr, dep, col in frames(sc, 3, 8):  # three frames: with pairing the third waits for a partner
            vol.integrateCloud(dep, col, tr, pipelined=True)
        vol.shiftVolume(3, -2, 1)
        got.append(vol.download())
        vol.close()
    assert (got[0][1] > 0).sum() > 1000
    same_volume(got[1], got[0], "pairing on against pairing off")
