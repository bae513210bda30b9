"""GPU tier: meshNormals on the GPU (tsdf_hip_mesh_normals / tsdf_hip_march_normals) against the numpy model of the rule in
tests/normals_cases.py (which tests/test_normals_oracle.py pins to the host pass that defines the result).  Every comparison
is exact -- the words of the normals, the flags, the counters: no tolerance, no exempt share."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, mesh_normals
from tests import normals_cases as nc
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
U32P = C.POINTER(C.c_uint32)
U64P = C.POINTER(C.c_uint64)
RES, W, H = 48, 160, 120
VOXEL = 2.0 ** -8  # of tests.common.make_volume's scene, whatever the resolution


def stats(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_normals_stats(out) == capi.OK
    return list(out)


def host_array(a, dtype, pinned):
    """(array, keep-alive) with the contents of `a`, in pinned or in pageable memory"""
    a = np.ascontiguousarray(a, dtype)
    if not pinned or a.size == 0:
        return a.copy(), None
    p = capi.PinnedArray(a.shape, dtype)
    p.array[...] = a
    return p.array, p


def run_abi(gpu, verts, faces, n_faces, pinned=False):
    """tsdf_hip_mesh_normals itself, on pinned or pageable arrays; faces None: a soup"""
    alive = []

    def arr(a, dtype):
        out, keep = host_array(a, dtype, pinned)
        alive.append(keep)
        return out

    n = len(verts)
    v = arr(verts, F32)
    # (an array without elements may have no address: an indexed mesh without faces is not a soup)
    f = None if faces is None else arr(faces if len(faces) else np.zeros((1, 3)), U32)
    out, flags = arr(np.full((n, 3), 7), F32), arr(np.full(n, 9), np.uint8)
    rc = gpu.tsdf_hip_mesh_normals(0, capi.as_f32p(v), n, None if f is None else f.ctypes.data_as(U32P), n_faces, capi.as_f32p(out), capi.as_u8p(flags))
    got = {"rc": rc, "normals": out.copy(), "flags": flags.copy()}
    for p in alive:
        if p is not None:
            p.free()
    return got


def assert_equals_model(got, want):
    assert got["normals"].dtype == F32 and got["normals"].shape == want.normals.shape
    assert np.array_equal(got["flags"], want.flags), "flags differ from the model's"
    bad = np.flatnonzero((got["normals"].view(U32) != want.normals.view(U32)).any(1))
    assert len(bad) == 0, f"{len(bad)} of {len(want.normals)} normals differ from the model's, first {bad[:8].tolist()}"


# ---- the cases, through the C ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("name", sorted(nc.cases()))
def test_case_equals_the_model(gpu, name, pinned):
    want = nc.model(name)
    got = run_abi(gpu, *nc.arrays(name), pinned=pinned)
    assert got["rc"] == capi.OK, capi.load().tsdf_hip_last_error()
    assert_equals_model(got, want)
    assert stats(gpu)[:3] == want.stats
    again = run_abi(gpu, *nc.arrays(name), pinned=pinned)
    for k in ("normals", "flags"):
        assert again[k].tobytes() == got[k].tobytes(), f"two calls differ in {k}"


def test_the_python_function_and_a_nullable_flags_argument(gpu):
    v, f, _ = nc.arrays("icosphere_5")
    want = nc.model("icosphere_5")
    assert_equals_model(mesh_normals(v, f), want)
    assert_equals_model(mesh_normals(nc.cases()["random_soup_257"][0]), nc.model("random_soup_257"))
    out = np.full((len(v), 3), 7, F32)
    capi.check(gpu.tsdf_hip_mesh_normals(0, capi.as_f32p(v), len(v), np.ascontiguousarray(f, U32).ctypes.data_as(U32P), len(f), capi.as_f32p(out), None),
               "mesh_normals")
    assert np.array_equal(out.view(U32), want.normals.view(U32))


def test_a_face_beyond_the_vertices_is_refused_and_nothing_is_written(gpu):
    v, f = nc.sc.random_mesh()
    f = f.copy()
    f[4321, 1] = len(v)
    assert run_abi(gpu, v, nc.cases()["random"][1], 6000)["rc"] == capi.OK
    before = stats(gpu)
    for pinned in (False, True):
        got = run_abi(gpu, v, f, len(f), pinned=pinned)
        assert got["rc"] == capi.E_INVALID and ">= n_verts" in capi.load().tsdf_hip_last_error().decode()
        assert (got["normals"] == 7).all() and (got["flags"] == 9).all()
    assert stats(gpu) == before
    with pytest.raises(capi.TsdfHipError) as e:
        mesh_normals(v, f)
    assert e.value.code == capi.E_INVALID


def test_empty_inputs(gpu):
    for faces in (nc.NO_FACES, None):
        got = mesh_normals(np.empty((0, 3), F32), faces)
        assert got["normals"].shape == (0, 3) and got["flags"].shape == (0,)
        assert stats(gpu) == [0, 0, 0, 0]
    v = nc.sc.grid_patch()[0]
    got = mesh_normals(v, nc.NO_FACES)  # no face: no vertex is named
    assert not got["normals"].any() and not np.signbit(got["normals"]).any() and (got["flags"] == 3).all()
    assert stats(gpu)[:3] == [len(v), 0, len(v)]


# ---- on a volume -----------------------------------------------------------------------------------------------------------
def fused_volume(devices=None, res=RES):
    vol, scene = make_volume(res, W, H, color=True)
    if devices:
        vol.setDevices(devices)
    vol.reset()
    for _, tr, dep, col in frames(scene, 3, 8):
        vol.integrateCloud(dep, col, tr)
    return vol


def fetch_indexed(gpu, h, m, k):
    out = {"vertices": np.empty((m, 3), F32), "rgb": np.empty((m, 3), np.uint8), "faces": np.empty((k, 3), U32), "cells": np.empty(k, np.uint64)}
    capi.check(gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(out["vertices"]), capi.as_u8p(out["rgb"]), out["faces"].ctypes.data_as(U32P),
                                                out["cells"].ctypes.data_as(U64P)), "march_fetch_indexed")
    return out


def fetch_soup(gpu, h, n):
    out = {"vertices": np.empty((3 * n, 3), F32), "rgb": np.empty((3 * n, 3), np.uint8), "cells": np.empty(n, np.uint64)}
    capi.check(gpu.tsdf_hip_march_fetch(h, capi.as_f32p(out["vertices"]), capi.as_u8p(out["rgb"]), out["cells"].ctypes.data_as(U64P)), "march_fetch")
    return out


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def normals_of(gpu, h, n_expected):
    """tsdf_hip_march_normals and the fetch: (normals, n_zero)"""
    n, zero = C.c_uint64(0), C.c_uint64(77)
    capi.check(gpu.tsdf_hip_march_normals(h, C.byref(n), C.byref(zero)), "march_normals")
    assert n.value == n_expected, "n_verts does not say which mesh it was"
    out = np.full((n_expected, 3), 7, F32)
    capi.check(gpu.tsdf_hip_march_fetch_normals(h, capi.as_f32p(out)), "march_fetch_normals")
    return out, zero.value


ROOM = np.zeros((1 << 21, 3), F32)  # more rows than any mesh of these tests has vertices: a fetch that succeeds stays inside


def no_normals(gpu, h):
    return gpu.tsdf_hip_march_fetch_normals(h, capi.as_f32p(ROOM)) == capi.E_INVALID


@pytest.fixture(scope="module")
def volume(gpu):
    vol = fused_volume()
    yield vol
    vol.close()


def check_stage(gpu, h, mesh, faces, soup):
    """normals of the handle's current mesh == the model on the mesh fetched now; neither mesh changes"""
    want = nc.Model(mesh["vertices"], faces)
    got, zero = normals_of(gpu, h, len(mesh["vertices"]))
    assert np.array_equal(got.view(U32), want.normals.view(U32)), "normals differ from the model's"
    assert zero == want.n_zero and stats(gpu)[:3] == want.stats and stats(gpu)[3] > 0
    assert same(fetch_soup(gpu, h, len(soup["cells"])), soup), "the soup changed"
    if faces is not None:
        assert same(fetch_indexed(gpu, h, len(mesh["vertices"]), len(mesh["faces"])), mesh), "the indexed mesh changed"
    assert not no_normals(gpu, h)
    return want


def test_march_normals_follows_the_handles_mesh(gpu, volume):
    h = volume._need()
    fresh, _ = make_volume(RES, W, H)
    fresh.reset()
    assert gpu.tsdf_hip_march_normals(fresh._need(), None, None) == capi.E_INVALID  # no march has run
    assert no_normals(gpu, fresh._need())
    fresh.close()
    n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    assert no_normals(gpu, h) and n.value > 1000
    soup = fetch_soup(gpu, h, n.value)
    flat = check_stage(gpu, h, soup, None, soup)  # the soup: flat normals
    assert flat.n_zero < len(flat.normals) // 10
    capi.check(gpu.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
    assert no_normals(gpu, h) and 1000 < m.value < 3 * n.value
    mesh = fetch_indexed(gpu, h, m.value, k.value)
    smooth_normals = check_stage(gpu, h, mesh, mesh["faces"], soup)
    assert smooth_normals.valence.max() >= 6 and not (smooth_normals.flags & 1).any()
    capi.check(gpu.tsdf_hip_march_smooth(h, 0.5, -0.53, 3, 1, None), "march_smooth")
    assert no_normals(gpu, h)
    moved = fetch_indexed(gpu, h, m.value, k.value)
    assert not np.array_equal(moved["vertices"], mesh["vertices"])
    check_stage(gpu, h, moved, moved["faces"], soup)
    capi.check(gpu.tsdf_hip_march_decimate(h, 2 * VOXEL, C.byref(m), C.byref(k)), "march_decimate")
    assert no_normals(gpu, h) and m.value > 500
    coarse = fetch_indexed(gpu, h, m.value, k.value)
    check_stage(gpu, h, coarse, coarse["faces"], soup)
    capi.check(gpu.tsdf_hip_march_cleanup(h, 0.01, 0, C.byref(n)), "march_cleanup")  # drops the indexed mesh as well: the soup again
    assert no_normals(gpu, h)
    soup = fetch_soup(gpu, h, n.value)
    check_stage(gpu, h, soup, None, soup)
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    assert no_normals(gpu, h)
    normals_of(gpu, h, 3 * n.value)
    # a second call gives the same normals
    a, _ = normals_of(gpu, h, 3 * n.value)
    b, _ = normals_of(gpu, h, 3 * n.value)
    assert a.tobytes() == b.tobytes()


def reconstruct(vol, decimate=None, flatten=None, smooth=False, normals=True):
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if decimate:
        mc.setDecimate(decimate)
    if flatten:
        mc.setFlatten(flatten)
    if smooth:
        mc.setSmooth(3)
    mc.setNormals(normals)
    return mc.reconstruct(want_cells=True)


VARIANTS = [dict(), dict(flatten=1e-4), dict(decimate=2 * VOXEL), dict(smooth=True), dict(decimate=2 * VOXEL, smooth=True)]


def assert_reconstructed(got, plain):
    """`got` is `plain` (the same settings without setNormals) plus the model's normals on its own vertices and faces"""
    for key in ("vertices", "polygons", "rgb", "cells"):
        assert np.array_equal(got[key], plain[key]), f"{key} changed with setNormals"
    assert "normals" not in plain
    soup = len(got["polygons"]) * 3 == len(got["vertices"]) and np.array_equal(got["polygons"].ravel(), np.arange(len(got["vertices"])))
    want = nc.Model(got["vertices"], None if soup else got["polygons"])
    assert got["normals"].dtype == F32 and np.array_equal(got["normals"].view(U32), want.normals.view(U32))
    return want


@pytest.fixture(scope="module")
def plains(gpu, volume):
    return [reconstruct(volume, normals=False, **kw) for kw in VARIANTS]


def test_reconstruct_with_set_normals(gpu, volume, plains):
    for kw, plain in zip(VARIANTS, plains):
        want = assert_reconstructed(reconstruct(volume, **kw), plain)
        assert len(want.normals) > 500 and want.n_zero < len(want.normals) // 10


def test_normals_on_a_multi_gpu_set_equal_one_handle(gpu, plains):
    vol = fused_volume(devices=[0, 0])
    try:
        for kw, plain in zip(VARIANTS, plains):
            assert_reconstructed(reconstruct(vol, **kw), plain)
        h = vol._need()
        assert not no_normals(gpu, h)
        capi.check(gpu.tsdf_hip_reset(h), "reset")  # (the entry point itself: the Python reset() makes a new handle)
        assert no_normals(gpu, h)
    finally:
        vol.close()


def test_reset_drops_the_normals(gpu):
    vol = fused_volume()
    try:
        h = vol._need()
        n = C.c_uint64(0)
        capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
        normals_of(gpu, h, 3 * n.value)
        capi.check(gpu.tsdf_hip_reset(h), "reset")  # (the entry point itself: the Python reset() makes a new handle)
        assert no_normals(gpu, h)
    finally:
        vol.close()


# ---- orientation -------------------------------------------------------------------------------------------------------------
def test_normals_of_a_marched_sphere_point_out_of_the_surface(gpu):
    """The sphere of tests/test_normals_oracle.py, uploaded: march -> flatten -> normals on the device.  The normals equal the
    model on the fetched mesh, no vertex is flagged, and every normal is within 8.1 degrees of the radial direction, outwards."""
    vol, _ = make_volume(nc.SPHERE_RES)
    vol.reset()
    try:
        d, w, centre = nc.sphere_field(vol._p)
        vol.upload(d=d, w=w)
        h = vol._need()
        n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(gpu.tsdf_hip_march(h, 1.0, 0, C.byref(n)), "march")
        capi.check(gpu.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
        assert n.value > 3000 and 1500 < m.value < 3 * n.value
        verts, faces = np.empty((m.value, 3), F32), np.empty((k.value, 3), U32)
        capi.check(gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(verts), None, faces.ctypes.data_as(U32P), None), "march_fetch_indexed")
        got, zero = normals_of(gpu, h, m.value)
        want = nc.Model(verts, faces)
        assert np.array_equal(got.view(U32), want.normals.view(U32))
        radial = verts.astype(np.float64) - centre
        dots = (got.astype(np.float64) * radial / np.linalg.norm(radial, axis=1, keepdims=True)).sum(1)
        print(f"{k.value} faces, {m.value} vertices, {zero} zero normals, minimum dot {dots.min():.4f}")
        assert zero == 0 and not want.flags.any()
        assert dots.min() >= 0.99
    finally:
        vol.close()
