"""GPU tier: tsdf_hip_esdf (cpu_tsdf_amd/csrc/tsdf_esdf.hip) -- the exact Euclidean distance transform of the volume's zero
crossing.  Every expectation is tests/esdf_cases.model (numpy: the site rule, three separable int64 passes, the float
formula) applied to the arrays that were uploaded, or to a download taken before the call; d2 is compared with
np.array_equal and dist bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection time, before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi
from tests import esdf_cases as ec
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
PACKED, F32W = capi.LAYOUT_PACKED, capi.LAYOUT_F32W
_u32p = C.POINTER(C.c_uint32)


def volume(res, layout, color=False, content=None, size=1.0, max_weight=3.0, rgb_seed=3):
    vol, _ = make_volume(res, 80, 60, color=color, size=size, max_weight=max_weight)
    vol.setLayout(layout)
    vol.reset()
    assert vol.getLayout() == layout
    if content is not None:
        rgb = np.random.RandomState(rgb_seed).randint(0, 256, content[0].shape + (3,)).astype(np.uint8) if color else None
        vol.upload(content[0], content[1], rgb)
    return vol


def esdf_raw(lib, vol, box=None, r_max=0, min_weight=0.0, n=None):
    b = (C.c_int32 * 6)(*[int(v) for v in box]) if box is not None else None
    return lib.tsdf_hip_esdf(vol._need(), b, int(r_max), C.c_float(min_weight), n)


def fetch_raw(lib, vol, shape):
    d2, dist = np.full(shape, 7, np.uint32), np.full(shape, 7, np.float32)
    rc = lib.tsdf_hip_esdf_fetch(vol._need(), d2.ctypes.data_as(_u32p), capi.as_f32p(dist))
    return rc, d2, dist


def same_field(got, want, what):
    assert got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), (what, "d2", int((got[0] != want[0]).sum()))
    ne = got[1].view(np.uint32) != want[1].view(np.uint32)
    assert not ne.any(), (what, "dist", int(ne.sum()), got[1][ne][:4], want[1][ne][:4], got[0][ne][:4])


def same_planes(a, b, what):
    for x, y in zip(a, b):
        if x is not None:
            assert x.tobytes() == y.tobytes(), what


# ---- 1. every layout, on dense random data ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random24():
    p = make_volume(24, 80, 60, size=1.0, max_weight=3.0)[0]._p
    d, w = ec.random_volume(np.random.RandomState(5), (24, 24, 24))
    want = {}
    for r in (0, 1, 3):
        for mw in (0.0, 1.0):
            want[r, mw] = ec.model(p, d, w, None, r, mw)
            d2, _, n = want[r, mw]
            assert n >= 100, "a field of few sites tests little"
            if r == 1:
                assert (d2 == ec.FAR).any() and (d2 != ec.FAR).any()
    assert np.isnan(d).sum() > 100 and (d == 0).sum() > 100 and (np.abs(d) == 1).sum() > 100
    return d, w, want


@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("layout", [F32W, PACKED], ids=["f32w", "packed"])
def test_layouts_equal_the_model(gpu, random24, layout, color):
    d, w, want = random24
    vol = volume(24, layout, color, (d, w))
    before = vol.download()
    assert before[0].tobytes() == d.tobytes() and before[1].tobytes() == w.tobytes()
    for (r, mw), (d2, dist, n) in want.items():
        assert vol.computeDistanceField(r, mw) == n, (r, mw)
        same_field(vol.getDistanceField(), (d2, dist), f"layout {layout}, colour {color}, r_max {r}, min_weight {mw}")
        st = vol.distanceFieldStats()
        assert st[0] == 24 ** 3 and st[1] == n and st[2] >= 24 ** 3 * 4 and st[3] > 0, st
    same_planes(vol.download(), before, "the volume is unchanged")
    vol.close()


# ---- 2. long lines, one axis at a time --------------------------------------------------------------------------------------
def long_case(n):
    """Sparse data on an n^3 grid and boxes of 12 x 12 x n along each axis (odd starts on the other two axes), which all
    hold the corner cube where the negatives sit; on the 272 grid also a negative voxel and a block far along each axis,
    negatives just outside every box (which must not count), and a box whose rows start and end unaligned."""
    singles = [(5, 6, 7), (8, 11, 9), (13, 13, 12)]
    boxes = {"x": (0, 3, 5, n, 12, 12), "y": (3, 0, 5, 12, n, 12), "z": (3, 5, 0, 12, 12, n)}
    if n > 200:
        singles += [(150, 7, 8), (7, 150, 8), (7, 8, 150)]
        singles += [(152, 2, 8), (8, 152, 17), (2, 9, 152)]  # just outside the x, y and z box
        boxes["x_unaligned"] = (3, 3, 5, 261, 12, 12)
    return ec.sparse((n, n, n), singles, (10, 8, 12, 2)), boxes


@pytest.mark.parametrize("n,layout", [(80, F32W), (272, PACKED)], ids=["80", "272"])
def test_long_lines_along_each_axis(gpu, n, layout):
    (d, w), boxes = long_case(n)
    vol = volume(n, layout, False, (d, w))
    for name, box in boxes.items():
        d2, dist, sites = ec.model(vol._p, d, w, box)
        finite = d2[d2 != ec.FAR]
        assert sites >= 10 and finite.max() >= 64 * 64, (name, sites, finite.max())  # the builder reaches far parabolas
        assert vol.computeDistanceField(box=box) == sites, name
        same_field(vol.getDistanceField(), (d2, dist), f"{n}^3, box along {name}")
    # and a truncated transform on the longest rows
    box = boxes["x"]
    d2, dist, sites = ec.model(vol._p, d, w, box, r_max=7)
    assert vol.computeDistanceField(7, 0.0, box) == sites
    same_field(vol.getDistanceField(), (d2, dist), f"{n}^3, r_max 7")
    vol.close()


# ---- 3. what the box means --------------------------------------------------------------------------------------------------
def test_box_semantics(gpu):
    res = (24, 24, 24)
    d, w = ec.sparse(res, [(10, 10, 10), (0, 0, 0), (23, 5, 23), (23, 17, 4), (0, 18, 4)])
    vol = volume(24, PACKED, False, (d, w))
    # the negative voxel (10, 10, 10) just outside: it does not count, but it makes its neighbour (11, 10, 10) a site
    box = (11, 8, 8, 6, 6, 6)
    d2, dist, n = ec.model(vol._p, d, w, box)
    assert n == 1 and d2[2, 2, 0] == 0 and d2[2, 2, 5] == 25
    assert vol.computeDistanceField(box=box) == 1
    same_field(vol.getDistanceField(), (d2, dist), "a neighbour outside the box")
    # one voxel further: the box holds no site (the site (11, 10, 10) next to it is outside and does not count)
    box = (12, 8, 8, 6, 6, 6)
    d2, dist, n = ec.model(vol._p, d, w, box)
    assert n == 0 and (d2 == ec.FAR).all()
    assert vol.computeDistanceField(box=box) == 0
    same_field(vol.getDistanceField(), (d2, dist), "a site just outside the box")
    # negatives on the grid's border and at row ends: no neighbour beyond the grid, none across a row's end
    d2, dist, n = ec.model(vol._p, d, w)
    assert n == 7 + 4 + 5 + 6 + 6  # a voxel and its neighbours inside the grid: interior, corner, edge, two faces
    assert vol.computeDistanceField() == n
    same_field(vol.getDistanceField(), (d2, dist), "the grid's border")
    vol.close()


# ---- 4. fused data ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [F32W, PACKED], ids=["f32w", "packed"])
def test_fused_volume(gpu, layout):
    lib = gpu
    vol, sc = make_volume(64, 160, 120, color=True)
    vol.setLayout(layout)
    vol.reset()
    for i, tr, dep, col in frames(sc, 3, 8):
        vol.integrateCloud(dep, col, tr)
    h = vol._need()
    idx, od, ow = vol.getOccupiedVoxelIndices(want=("d", "w"))
    assert vol.occupiedStats()[2] == 1  # the band flags are live
    nt = C.c_uint64(0)
    capi.check(lib.tsdf_hip_march(h, 0.5, 0, C.byref(nt)), "march")
    nt = int(nt.value)
    assert nt > 1000 and len(idx) > 1000
    verts = np.empty(nt * 9, np.float32)
    capi.check(lib.tsdf_hip_march_fetch(h, capi.as_f32p(verts), None, None), "march_fetch")
    before = vol.download()
    d2, dist, n = ec.model(vol._p, before[0], before[1])
    assert n > 1000 and (dist < 0).sum() > 100
    assert vol.computeDistanceField() == n
    same_field(vol.getDistanceField(), (d2, dist), f"fused, layout {layout}")
    same_planes(vol.download(), before, "the volume is unchanged")
    verts2 = np.empty(nt * 9, np.float32)
    capi.check(lib.tsdf_hip_march_fetch(h, capi.as_f32p(verts2), None, None), "march_fetch")
    assert verts2.tobytes() == verts.tobytes()
    idx2 = np.empty((len(idx), 3), np.int32)
    od2, ow2 = np.empty(len(idx), np.float32), np.empty(len(idx), np.float32)
    capi.check(lib.tsdf_hip_occupied_fetch(h, idx2.ctypes.data_as(C.POINTER(C.c_int32)), capi.as_f32p(od2), capi.as_f32p(ow2), None), "occupied_fetch")
    assert np.array_equal(idx2, idx) and od2.tobytes() == od.tobytes() and ow2.tobytes() == ow.tobytes()
    vol.getOccupiedVoxelIndices()
    assert vol.occupiedStats()[2] == 1  # and the flags still decide what the scan reads
    vol.close()


def test_empty_volume(gpu):
    vol = volume(24, PACKED)
    assert vol.computeDistanceField() == 0
    d2, dist = vol.getDistanceField()
    assert d2.shape == (24, 24, 24) and (d2 == ec.FAR).all() and (dist == np.inf).all()
    want = ec.model(vol._p, *ec.empty((24, 24, 24)))
    same_field((d2, dist), want[:2], "empty")
    assert vol.distanceFieldStats()[:2] == (24 ** 3, 0)
    vol.close()


# ---- 5. point queries and device buffers ------------------------------------------------------------------------------------
def test_sample_equals_the_voxel_lookup(gpu):
    lib = gpu
    d, w = ec.random_volume(np.random.RandomState(6), (24, 24, 24))
    vol = volume(24, F32W, False, (d, w))
    box = (3, 5, 7, 16, 14, 12)
    d2, dist, n = ec.model(vol._p, d, w, box)
    assert vol.computeDistanceField(box=box) == n
    rng = np.random.RandomState(7)
    pts = rng.uniform(-0.6, 0.6, (1000, 3)).astype(np.float32)
    pts[:4] = [[0.7, 0, 0], [0, -0.51, 0], [0, 0, 5.0], [np.nan, 0, np.nan]]
    got, found = vol.getDistance(pts)
    want, want_found = np.full(1000, np.nan, np.float32), np.zeros(1000, bool)
    for k, pt in enumerate(pts):
        ok, (i, j, kz) = vol.getVoxelIndex(*pt)
        ok = ok and bool(np.all(np.abs(pt) <= 0.5))
        i, j, kz = i - box[0], j - box[1], kz - box[2]
        if ok and 0 <= i < box[3] and 0 <= j < box[4] and 0 <= kz < box[5]:
            want[k], want_found[k] = dist[kz, j, i], True
    assert 50 < want_found.sum() < 500 and not want_found[:4].any()
    assert np.array_equal(found, want_found)
    assert np.array_equal(got.view(np.uint32)[found], want.view(np.uint32)[found]) and np.isnan(got[~found]).all()
    vol.close()


def test_fetch_device_equals_the_host_fetch(gpu):
    lib = gpu
    d, w = ec.random_volume(np.random.RandomState(8), (24, 24, 24))
    vol = volume(24, PACKED, True, (d, w))
    box = (1, 2, 3, 20, 19, 18)
    vol.computeDistanceField(2, 0.0, box)
    d2, dist = vol.getDistanceField()
    n = d2.size
    t_d2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_dist = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    capi.check(lib.tsdf_hip_esdf_fetch_device(vol._need(), C.c_void_p(t_d2.data_ptr()), C.c_void_p(t_dist.data_ptr())), "fetch_device")
    vol.synchronize()
    assert np.array_equal(t_d2.cpu().numpy().view(np.uint32), d2.reshape(-1))
    assert np.array_equal(t_dist.cpu().numpy().view(np.uint32), dist.reshape(-1).view(np.uint32))
    capi.check(lib.tsdf_hip_esdf_fetch_device(vol._need(), None, None), "fetch_device")  # either may be NULL
    vol.close()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------------
def test_lifetime(gpu):
    lib = gpu
    vol, sc = make_volume(32, 160, 120, color=False)
    vol.reset()
    shape = (32, 32, 32)
    pt = np.zeros(3, np.float32)
    one, fnd = np.zeros(1, np.float32), np.zeros(1, np.uint8)

    def sample_rc():
        return lib.tsdf_hip_esdf_sample(vol._need(), capi.as_f32p(pt), 1, capi.as_f32p(one), capi.as_u8p(fnd))
    rc, d2, dist = fetch_raw(lib, vol, shape)
    assert rc == capi.E_INVALID and (d2 == 7).all() and (dist == 7).all(), "a fetch before the first compute"
    assert sample_rc() == capi.E_INVALID
    assert lib.tsdf_hip_esdf_fetch_device(vol._need(), None, None) == capi.E_INVALID
    assert vol.distanceFieldStats() == (0, 0, 0, 0)
    fr = list(frames(sc, 3, 8))
    for i, tr, dep, col in fr[:2]:
        vol.integrateCloud(dep, None, tr)
    first = vol.download()
    want = ec.model(vol._p, first[0], first[1])
    assert want[2] > 200 and vol.computeDistanceField() == want[2]
    same_field(vol.getDistanceField(), want[:2], "after two frames")
    # stale by design: a later integrate changes the volume, not the field -- its sign included
    vol.integrateCloud(fr[2][2], None, fr[2][1])
    second = vol.download()
    assert second[0].tobytes() != first[0].tobytes() and ((second[0] < 0) != (first[0] < 0)).any()
    same_field(vol.getDistanceField(), want[:2], "after a later integrate")
    # two identical computes give identical results, which are the model's of the volume as it is now
    want = ec.model(vol._p, second[0], second[1])
    for k in range(2):
        assert vol.computeDistanceField() == want[2]
        same_field(vol.getDistanceField(), want[:2], f"compute {k} after three frames")
    # a second compute with another box replaces the first
    box = (4, 0, 9, 25, 32, 7)
    wb = ec.model(vol._p, second[0], second[1], box, 5, 1.0)
    assert vol.computeDistanceField(5, 1.0, box) == wb[2] and vol.distanceFieldStats()[0] == 25 * 32 * 7
    same_field(vol.getDistanceField(), wb[:2], "another box")
    # the indices move in a shift: refused until computed again
    vol.shiftVolume(1, 0, 0)
    assert fetch_raw(lib, vol, (7, 32, 25))[0] == capi.E_INVALID and sample_rc() == capi.E_INVALID
    assert lib.tsdf_hip_esdf_fetch_device(vol._need(), None, None) == capi.E_INVALID
    third = vol.download()
    want = ec.model(vol._p, third[0], third[1])
    assert vol.computeDistanceField() == want[2]
    same_field(vol.getDistanceField(), want[:2], "after a shift")
    assert sample_rc() == capi.OK
    # dropped by tsdf_hip_reset (vol.reset() would make a new handle)
    capi.check(lib.tsdf_hip_reset(vol._need()), "reset")
    assert fetch_raw(lib, vol, shape)[0] == capi.E_INVALID and sample_rc() == capi.E_INVALID
    assert vol.distanceFieldStats() == (0, 0, 0, 0)
    vol.close()


def test_a_frame_held_back_by_frame_pairing_is_part_of_the_field(gpu):
    vol, sc = make_volume(32, 160, 120, color=False)
    twin, _ = make_volume(32, 160, 120, color=False)
    vol.reset()
    twin.reset()
    vol.setFramePairing(True)
    for i, tr, dep, col in frames(sc, 3, 8):  # an odd number: the third frame waits for a partner
        vol.integrateCloud(dep, None, tr, pipelined=True)
        twin.integrateCloud(dep, None, tr)
    n = vol.computeDistanceField()
    planes = twin.download()
    want = ec.model(twin._p, planes[0], planes[1])
    assert n == want[2] and n > 200
    same_field(vol.getDistanceField(), want[:2], "frame pairing")
    vol.close()
    twin.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal(gpu):
    lib = gpu
    d, w = ec.random_volume(np.random.RandomState(9), (16, 16, 16))
    vol = volume(16, PACKED, False, (d, w))
    want = ec.model(vol._p, d, w)
    assert vol.computeDistanceField() == want[2]

    def refused(v, box, r_max, min_weight, code, word, what):
        before = v.download()
        n = C.c_uint64(7)
        rc = esdf_raw(lib, v, box, r_max, min_weight, C.byref(n))
        assert rc == code, (what, rc)
        if code == capi.E_UNSUPPORTED:
            msg = lib.tsdf_hip_last_error().decode()
            assert "tsdf_hip_esdf" in msg and word in msg, (what, msg)
        same_planes(v.download(), before, what + ": the volume is unchanged")
        assert n.value == 7, what

    # E_INVALID
    for box, what in [((0, 0, 0, 17, 16, 16), "nx past the grid"), ((1, 0, 0, 16, 16, 16), "x0 + nx past the grid"),
                      ((0, 9, 0, 16, 8, 16), "y0 + ny past the grid"), ((0, 0, 16, 16, 16, 1), "z0 past the grid"),
                      ((-1, 0, 0, 4, 4, 4), "a negative x0"), ((0, 0, -2, 4, 4, 4), "a negative z0"),
                      ((0, 0, 0, 0, 4, 4), "nx == 0"), ((0, 0, 0, 4, -3, 4), "ny < 0"), ((0, 0, 0, 4, 4, 0), "nz == 0"),
                      ((0, 0, 0, 2 ** 31 - 1, 4, 4), "an extent that overflows")]:
        refused(vol, box, 0, 0.0, capi.E_INVALID, "", what)
    refused(vol, None, -1, 0.0, capi.E_INVALID, "", "r_max < 0")
    refused(vol, None, 0, -0.5, capi.E_INVALID, "", "a negative min_weight")
    refused(vol, None, 0, float("nan"), capi.E_INVALID, "", "a NaN min_weight")
    # (a NULL handle: tests/test_esdf_abi.py)

    # E_UNSUPPORTED
    def odd(**kw):
        v, _ = make_volume(16, 80, 60, size=1.0, max_weight=3.0, res3=kw.pop("res3", None), size3=kw.pop("size3", None))
        for name, args in kw.items():
            getattr(v, name)(*args)
        v.reset()
        return v
    for word, v, what in [("multi-GPU", odd(setDevices=([0, 0],)), "a multi-GPU set"),
                          ("part of its grid", odd(setZSlab=(4, 12, 2)), "a Z-slab handle"),
                          ("cubic", odd(res3=(16, 16, 8)), "res not equal on all axes"),
                          ("cubic", odd(res3=(8, 16, 16)), "res not equal on all axes (x)"),
                          ("cubic", odd(size3=(1.0, 1.0, 0.5)), "size not equal on all axes"),
                          ("cubic", odd(size3=(1.0, 0.5, 1.0)), "size not equal on all axes (y)")]:
        refused(v, None, 0, 0.0, capi.E_UNSUPPORTED, word, what)
        assert lib.tsdf_hip_esdf_fetch(v._need(), None, None) != capi.OK, what
        v.close()
    # none of that touched the field this volume holds
    same_field(vol.getDistanceField(), want[:2], "after every refusal")
    vol.close()
