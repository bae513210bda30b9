"""GPU tier: smoothMesh on the GPU (tsdf_hip_mesh_smooth / tsdf_hip_march_smooth) against the numpy model of the rule in
tests/smooth_cases.py (which tests/test_smooth_oracle.py pins to the host pass that defines the result).  Every comparison is
exact -- the words of the output vertices, the fixed bits, the degrees, the counters: no tolerance, no exempt share."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, smooth_mesh
from tests import smooth_cases as sc
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
U32P = C.POINTER(C.c_uint32)
U64P = C.POINTER(C.c_uint64)
RES, W, H = 48, 160, 120
VOXEL = 2.0 ** -8  # of tests.common.make_volume's scene, whatever the resolution
ARGS = (0.5, -0.53, 3, 1)  # the handle route: lambda, mu, iterations, keep_boundary


def stats(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_smooth_stats(out) == capi.OK
    return list(out)


def host_array(a, dtype, pinned):
    """(array, keep-alive) with the contents of `a`, in pinned or in pageable memory"""
    a = np.ascontiguousarray(a, dtype)
    if not pinned or a.size == 0:
        return a.copy(), None
    p = capi.PinnedArray(a.shape, dtype)
    p.array[...] = a
    return p.array, p


def run_abi(gpu, verts, faces, lam, mu, iterations, keep_boundary, pinned=False, alias=False):
    """tsdf_hip_mesh_smooth itself, on pinned or pageable arrays; alias: out_verts is `verts`"""
    alive = []

    def arr(a, dtype):
        out, keep = host_array(a, dtype, pinned)
        alive.append(keep)
        return out

    n = len(verts)
    v, f = arr(verts, F32), arr(faces, U32)
    out = v if alias else arr(np.full((n, 3), 7), F32)
    fixed, degree = arr(np.full(n, 9), np.uint8), arr(np.full(n, 9), U32)
    rc = gpu.tsdf_hip_mesh_smooth(0, capi.as_f32p(v), n, f.ctypes.data_as(U32P), len(f), float(F32(lam)), float(F32(mu)), int(iterations),
                                  int(keep_boundary), capi.as_f32p(out), capi.as_u8p(fixed), degree.ctypes.data_as(U32P))
    got = {"rc": rc, "vertices": out.copy(), "fixed": fixed.copy(), "degree": degree.copy()}
    for p in alive:
        if p is not None:
            p.free()
    return got


def assert_equals_model(got, want):
    assert got["vertices"].dtype == F32 and got["vertices"].shape == want.vertices.shape
    assert np.array_equal(got["degree"], want.degree), "degrees differ from the model's"
    assert np.array_equal(got["fixed"], want.fixed), "fixed bits differ from the model's"
    bad = np.flatnonzero((got["vertices"].view(U32) != want.vertices.view(U32)).any(1))
    assert len(bad) == 0, f"{len(bad)} of {len(want.vertices)} output vertices differ from the model's, first {bad[:8].tolist()}"


# ---- the cases, through the C ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("name", sorted(sc.cases()))
def test_case_equals_the_model(gpu, name, pinned, alias):
    want = sc.model(name)
    got = run_abi(gpu, *sc.cases()[name], pinned=pinned, alias=alias)
    assert got["rc"] == capi.OK, capi.load().tsdf_hip_last_error()
    assert_equals_model(got, want)
    st = stats(gpu)
    assert st[:3] == [len(want.vertices), want.n_edges, want.n_fixed]
    assert st[3] > 0 or want.steps == 0
    again = run_abi(gpu, *sc.cases()[name], pinned=pinned, alias=alias)
    for k in ("vertices", "fixed", "degree"):
        assert again[k].tobytes() == got[k].tobytes(), f"two calls differ in {k}"


def test_a_mesh_above_the_pinned_copy_threshold(gpu):
    """64 KiB and more of pinned memory is copied without staging: the icosphere of the property check, 2562 vertices, with
    vertices and faces above that size when subdivided once more."""
    v, f = sc.icosphere(5)
    rng = np.random.default_rng(5)
    x = (v * (0.5 * (1.0 + rng.normal(0, 0.01, len(v))))[:, None] + 1.0).astype(F32)
    assert x.nbytes >= 64 << 10 and f.nbytes >= 64 << 10
    want = sc.Model(x, f, 0.5, -0.53, 10, 1)
    assert not want.fixed.any() and want.degree.min() == 5 and want.degree.max() == 6
    for pinned in (False, True):
        for alias in (False, True):
            got = run_abi(gpu, x, f, 0.5, -0.53, 10, 1, pinned=pinned, alias=alias)
            assert got["rc"] == capi.OK, capi.load().tsdf_hip_last_error()
            assert_equals_model(got, want)
    got = smooth_mesh(x, f)  # the defaults are these arguments
    assert_equals_model(got, want)
    assert stats(gpu)[:3] == [len(x), want.n_edges, 0]


def test_a_face_beyond_the_vertices_is_refused_and_nothing_is_written(gpu):
    v, f = sc.random_mesh()
    f = f.copy()
    f[4321, 1] = len(v)
    before = stats(gpu)
    for alias in (False, True):
        got = run_abi(gpu, v, f, 0.5, -0.53, 3, 1, alias=alias)
        assert got["rc"] == capi.E_INVALID and ">= n_verts" in capi.load().tsdf_hip_last_error().decode()
        assert (got["fixed"] == 9).all() and (got["degree"] == 9).all()
        assert np.array_equal(got["vertices"].view(U32), v.view(U32)) if alias else (got["vertices"] == 7).all()
    assert stats(gpu) == before
    with pytest.raises(capi.TsdfHipError) as e:
        smooth_mesh(v, f)
    assert e.value.code == capi.E_INVALID


def test_empty_inputs(gpu):
    got = smooth_mesh(np.empty((0, 3), F32), sc.NO_FACES)
    assert got["vertices"].shape == (0, 3) and got["fixed"].shape == (0,) and got["degree"].shape == (0,)
    assert stats(gpu) == [0, 0, 0, 0]
    v = sc.grid_patch()[0]
    got = smooth_mesh(v, sc.NO_FACES)  # no face: every vertex is without a neighbour and stays
    assert np.array_equal(got["vertices"].view(U32), v.view(U32)) and (got["fixed"] == 2).all() and not got["degree"].any()
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


def indexed(gpu, h, decimate):
    """march, then flatten or decimate: (the soup, the indexed mesh)"""
    n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    soup = fetch_soup(gpu, h, n.value)
    if decimate:
        capi.check(gpu.tsdf_hip_march_decimate(h, decimate, C.byref(m), C.byref(k)), "march_decimate")
    else:
        capi.check(gpu.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
    assert 1000 < m.value < 3 * n.value and k.value > 1000
    return soup, fetch_indexed(gpu, h, m.value, k.value)


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.fixture(scope="module")
def volume(gpu):
    vol = fused_volume()
    yield vol
    vol.close()


@pytest.fixture(scope="module")
def wants(gpu, volume):
    """decimate cell (None: flatten) -> (soup, indexed mesh before smoothing, the model of one and of two march_smooth calls)"""
    out = {}
    for decimate in (None, 2 * VOXEL):
        soup, mesh = indexed(gpu, volume._need(), decimate)
        once = sc.Model(mesh["vertices"], mesh["faces"], *ARGS)
        assert 0 < once.n_fixed < len(once.fixed) and once.degree.max() >= 6  # the mesh ends at the volume's faces: it has a boundary
        out[decimate] = soup, mesh, once, sc.Model(once.vertices, mesh["faces"], *ARGS)
    return out


@pytest.mark.parametrize("decimate", [None, 2 * VOXEL], ids=["flatten", "decimate"])
def test_march_smooth_is_the_model_on_the_indexed_mesh_fetched_before(gpu, volume, wants, decimate):
    soup, mesh, once, twice = wants[decimate]
    h = volume._need()
    soup_now, mesh_now = indexed(gpu, h, decimate)
    assert same(soup_now, soup) and same(mesh_now, mesh)
    m, k = len(mesh["vertices"]), len(mesh["faces"])
    n_fixed = C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march_smooth(h, *ARGS, C.byref(n_fixed)), "march_smooth")
    got = fetch_indexed(gpu, h, m, k)
    assert np.array_equal(got["vertices"].view(U32), once.vertices.view(U32))
    assert not np.array_equal(got["vertices"], mesh["vertices"])
    for key in ("rgb", "faces", "cells"):
        assert np.array_equal(got[key], mesh[key]), f"{key} changed"
    assert n_fixed.value == once.n_fixed and stats(gpu)[:3] == [m, once.n_edges, once.n_fixed] and stats(gpu)[3] > 0
    assert same(fetch_soup(gpu, h, len(soup["cells"])), soup), "the soup changed"
    # a second call smooths further
    capi.check(gpu.tsdf_hip_march_smooth(h, *ARGS, None), "march_smooth")
    got = fetch_indexed(gpu, h, m, k)
    assert np.array_equal(got["vertices"].view(U32), twice.vertices.view(U32))
    # a refused call leaves the mesh as it is
    assert gpu.tsdf_hip_march_smooth(h, 0.0, -0.53, 3, 1, None) == capi.E_INVALID
    assert np.array_equal(fetch_indexed(gpu, h, m, k)["vertices"].view(U32), twice.vertices.view(U32))


def test_march_smooth_needs_an_indexed_mesh(gpu, volume):
    fresh, _ = make_volume(RES, W, H)
    fresh.reset()
    assert gpu.tsdf_hip_march_smooth(fresh._need(), *ARGS, None) == capi.E_INVALID
    fresh.close()
    h = volume._need()
    n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    assert gpu.tsdf_hip_march_smooth(h, *ARGS, None) == capi.E_INVALID  # a soup: nothing has flattened it
    assert "flatten or decimate first" in gpu.tsdf_hip_last_error().decode()
    capi.check(gpu.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
    capi.check(gpu.tsdf_hip_march_smooth(h, *ARGS, None), "march_smooth")
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")  # a new march invalidates the indexed mesh
    assert gpu.tsdf_hip_march_smooth(h, *ARGS, None) == capi.E_INVALID
    capi.check(gpu.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
    capi.check(gpu.tsdf_hip_march_cleanup(h, 0.01, 0, C.byref(n)), "march_cleanup")  # so does a cleanup
    assert gpu.tsdf_hip_march_smooth(h, *ARGS, None) == capi.E_INVALID


def reconstruct(vol, decimate=None, flatten=None, smooth=True):
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if decimate:
        mc.setDecimate(decimate)
    if flatten:
        mc.setFlatten(flatten)
    if smooth:
        mc.setSmooth(ARGS[2], ARGS[0], ARGS[1], bool(ARGS[3]))
    return mc.reconstruct(want_cells=True)


def assert_reconstructed(got, mesh, model):
    assert np.array_equal(got["vertices"].view(U32), model.vertices.view(U32))
    assert np.array_equal(got["polygons"], mesh["faces"].astype(np.int32)) and np.array_equal(got["rgb"], mesh["rgb"])
    assert np.array_equal(got["cells"], mesh["cells"])


def test_reconstruct_with_set_smooth(gpu, volume, wants):
    for decimate in wants:
        _, mesh, once, _ = wants[decimate]
        assert_reconstructed(reconstruct(volume, decimate=decimate), mesh, once)
    # with setFlatten as well it is the same mesh as with setSmooth alone, which flattens at the default distance
    assert_reconstructed(reconstruct(volume, flatten=1e-4), wants[None][1], wants[None][2])
    # clearSmooth gives the flattened mesh back
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(volume)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    mc.setFlatten(1e-4)
    mc.setSmooth(5)
    mc.clearSmooth()
    got = mc.reconstruct()
    assert np.array_equal(got["vertices"].view(U32), wants[None][1]["vertices"].view(U32))


def test_smooth_on_a_multi_gpu_set_equals_one_handle(gpu, wants):
    vol = fused_volume(devices=[0, 0])
    try:
        for decimate in wants:
            _, mesh, once, twice = wants[decimate]
            assert_reconstructed(reconstruct(vol, decimate=decimate), mesh, once)
            capi.check(gpu.tsdf_hip_march_smooth(vol._need(), *ARGS, None), "march_smooth")  # a second call, on the host-held mesh
            got = fetch_indexed(gpu, vol._need(), len(mesh["vertices"]), len(mesh["faces"]))
            assert np.array_equal(got["vertices"].view(U32), twice.vertices.view(U32))
            assert np.array_equal(got["faces"], mesh["faces"]) and np.array_equal(got["rgb"], mesh["rgb"])
    finally:
        vol.close()
