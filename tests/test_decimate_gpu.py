"""GPU tier: decimateMesh on the GPU (tsdf_hip_mesh_decimate / tsdf_hip_march_decimate) against the numpy restatement of the
SEQUENTIAL host pass in tests/decimate_cases.py (which tests/test_decimate_oracle.py pins to the host pass itself).  Every
comparison is exact -- remap, output vertex bits, colours, member counts, polygons: no tolerance, no exempt share -- and every
case is one on which the model alone keeps clusters of one and of several members (and drops a degenerate face, drops a
duplicate face and keeps a face where faces take part)."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, decimate_mesh
from tests import decimate_cases as dc
from tests.common import make_volume
from tests.test_meshpost_gpu import H, RES, V_FD, W, fused_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
U32P = C.POINTER(C.c_uint32)
NO_FACES = np.empty((0, 3), np.uint32)
VOXEL = 0.25 / RES  # the fused volume is 0.25 m across
CELLS = (1, 2, 4)   # cell sizes of the handle path, in voxels
# On the CPU oracle's mesh of that volume the model finds duplicate faces at 1 and at 2 voxels (2 and 6) and none at 4:
# the cell sizes that must show the duplicate rule.
CELLS_WITH_DUPLICATES = (1, 2)


def stats(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_decimate_stats(out) == capi.OK
    return list(out)


def host_array(a, dtype, pinned):
    """(array, keep-alive) with the contents of `a`, in pinned or in pageable memory"""
    a = np.ascontiguousarray(a, dtype)
    if not pinned or a.size == 0:
        return a.copy(), None
    p = capi.PinnedArray(a.shape, dtype)
    p.array[...] = a
    return p.array, p


def run_abi(gpu, verts, faces, rgb, cell, pinned=False, alias=False):
    """tsdf_hip_mesh_decimate itself, on pinned or pageable arrays; alias: out_faces is `faces`"""
    keep = []

    def arr(a, dtype):
        out, alive = host_array(a, dtype, pinned)
        keep.append(alive)
        return out

    n = len(verts)
    nf = n // 3 if faces is None else len(faces)
    v = arr(verts, F32)
    c = arr(rgb, np.uint8) if rgb is not None else None
    f = arr(faces, np.uint32) if faces is not None else None
    remap, counts = arr(np.zeros(n), np.uint32), arr(np.zeros(n), np.uint32)
    out_v = arr(np.zeros((n, 3)), F32)
    out_c = arr(np.zeros((n, 3)), np.uint8) if rgb is not None else None
    out_f = f if alias else arr(np.zeros((nf, 3)), np.uint32)
    m, k = C.c_uint64(0), C.c_uint64(0)
    rc = gpu.tsdf_hip_mesh_decimate(0, capi.as_f32p(v), capi.as_u8p(c) if c is not None else None, n, f.ctypes.data_as(U32P) if f is not None else None,
                                    nf, float(F32(cell)), remap.ctypes.data_as(U32P), capi.as_f32p(out_v),
                                    capi.as_u8p(out_c) if out_c is not None else None, counts.ctypes.data_as(U32P), C.byref(m),
                                    out_f.ctypes.data_as(U32P) if nf else None, C.byref(k))
    m, k = int(m.value), int(k.value)
    got = {"rc": rc, "remap": remap.copy(), "vertices": out_v[:m].copy(), "rgb": out_c[:m].copy() if out_c is not None else None,
           "counts": counts[:m].copy(), "polygons": out_f[:k].astype(np.int32) if nf else np.empty((0, 3), np.int32)}
    for p in keep:
        if p is not None:
            p.free()
    return got


def assert_equals_model(got, want, with_faces):
    assert got["remap"].dtype == np.uint32 and got["counts"].dtype == np.uint32 and got["polygons"].dtype == np.int32
    bad = np.flatnonzero(got["remap"] != want.remap) if got["remap"].shape == want.remap.shape else None
    assert bad is not None and len(bad) == 0, f"{len(bad)} of {len(want.remap)} remap entries differ, first {bad[:8].tolist()}"
    assert got["vertices"].dtype == F32 and got["vertices"].shape == want.vertices.shape
    bad = np.flatnonzero((got["vertices"].view(np.uint32) != want.vertices.view(np.uint32)).any(1))
    assert len(bad) == 0, f"{len(bad)} of {len(want.vertices)} output vertices differ, first {bad[:8].tolist()}"
    assert np.array_equal(got["counts"], want.counts)
    if want.rgb is None:
        assert got["rgb"] is None
    else:
        assert np.array_equal(got["rgb"], want.rgb)
    if with_faces:
        assert np.array_equal(got["polygons"], want.polygons)
    else:
        assert got["polygons"].shape == (0, 3)


# ---- the cases, through the C ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("name", sorted(dc.cases()))
def test_case_equals_the_model(gpu, name, pinned):
    verts, faces, rgb, cell, with_faces = dc.cases()[name]
    want = dc.model(name)
    got = run_abi(gpu, verts, faces if with_faces else NO_FACES, rgb, cell, pinned=pinned)
    assert got["rc"] == capi.OK, capi.load().tsdf_hip_last_error()
    assert_equals_model(got, want, with_faces)
    st = stats(gpu)
    assert st[0] == len(verts) and st[1] == len(want.counts)
    assert st[2] == (int(want.duplicate.sum()) if with_faces else 0)


def test_python_wrapper_and_faces_written_over_the_input(gpu):
    verts, faces, rgb, cell, _ = dc.cases()["snapped_indexed"]
    want = dc.model("snapped_indexed")
    got = decimate_mesh(verts, faces, rgb, cell_size=cell)
    assert_equals_model(got, want, True)
    n_in = len(faces)
    st = stats(gpu)
    # degenerate drops are faces in - faces out - duplicates
    assert n_in - len(got["polygons"]) - st[2] == int(want.degenerate.sum()) and st[2] == int(want.duplicate.sum())
    for pinned in (False, True):
        got = run_abi(gpu, verts, faces, rgb, cell, pinned=pinned, alias=True)
        assert got["rc"] == capi.OK
        assert_equals_model(got, want, True)
    # without colours, and as a soup through the wrapper
    verts, _, rgb, cell, _ = dc.cases()["snapped_soup"]
    got = decimate_mesh(verts, None, None, cell_size=cell)
    assert got["rgb"] is None and np.array_equal(got["polygons"], dc.model("snapped_soup").polygons)
    with pytest.raises(ValueError):
        decimate_mesh(verts)


def test_refusals_that_need_the_device(gpu):
    before = stats(gpu)
    got = run_abi(gpu, dc.extent_refused(), NO_FACES, None, 1.0)
    assert got["rc"] == capi.E_INVALID and "1048576" in capi.load().tsdf_hip_last_error().decode()
    assert not got["remap"].any() and len(got["vertices"]) == 0  # nothing was written
    assert stats(gpu) == before
    with pytest.raises(capi.TsdfHipError) as e:
        decimate_mesh(dc.extent_refused(), NO_FACES, cell_size=1.0)
    assert e.value.code == capi.E_INVALID
    pool, faces = dc.snapped_mesh()
    faces = faces.copy()
    faces[123, 1] = len(pool)  # a face that names a vertex beyond the array
    with pytest.raises(capi.TsdfHipError) as e:
        decimate_mesh(pool, faces, cell_size=dc.SNAP_CELL)
    assert e.value.code == capi.E_INVALID


def test_empty_inputs(gpu):
    got = decimate_mesh(np.empty((0, 3), F32), None, cell_size=1.0)
    assert got["vertices"].shape == (0, 3) and got["polygons"].shape == (0, 3) and got["remap"].shape == (0,) and got["counts"].shape == (0,)
    assert stats(gpu) == [0, 0, 0, 0]
    got = decimate_mesh(dc.extent_edges(), NO_FACES, cell_size=1.0)
    assert got["polygons"].shape == (0, 3) and len(got["counts"]) == 4


# ---- on a volume -----------------------------------------------------------------------------------------------------------
def reconstruct(vol, cleanup=None, decimate=None, flatten=None):
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if cleanup:
        mc.setCleanup(*cleanup)
    if flatten:
        mc.setFlatten(flatten)
    if decimate:
        mc.setDecimate(decimate)
    return mc.reconstruct(want_cells=True)


def model_of(mesh, cells):
    want = dc.Dec(mesh["vertices"], None, mesh["rgb"], cells * VOXEL).check_mixed(faces=False)
    assert want.degenerate.any() and want.keep.any()
    if cells in CELLS_WITH_DUPLICATES:
        assert want.duplicate.any()
    return want


@pytest.fixture(scope="module")
def plain(gpu):
    vol = fused_volume()
    mesh = reconstruct(vol)
    cleaned = reconstruct(vol, cleanup=(V_FD, 40))
    assert 0 < len(cleaned["cells"]) < len(mesh["cells"])
    wants = {(tag, k): model_of(m, k) for tag, m in (("plain", mesh), ("cleaned", cleaned)) for k in CELLS}
    yield vol, {"plain": mesh, "cleaned": cleaned}, wants
    vol.close()


def assert_indexed(got, soup, want):
    assert np.array_equal(got["vertices"].view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(got["polygons"], want.polygons)
    assert np.array_equal(got["rgb"], want.rgb)
    assert np.array_equal(got["cells"], soup["cells"][want.keep])
    assert len(got["vertices"]) < len(soup["vertices"])


def fetch_indexed(gpu, h, m, k):
    out = {"vertices": np.empty((m, 3), F32), "rgb": np.empty((m, 3), np.uint8), "faces": np.empty((k, 3), np.uint32), "cells": np.empty(k, np.uint64)}
    capi.check(gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(out["vertices"]), capi.as_u8p(out["rgb"]), out["faces"].ctypes.data_as(U32P),
                                                out["cells"].ctypes.data_as(C.POINTER(C.c_uint64))), "march_fetch_indexed")
    out["polygons"] = out.pop("faces").astype(np.int32)
    return out


@pytest.mark.parametrize("cells", CELLS)
def test_march_decimate_fetch_indexed_is_the_model_on_the_fetched_soup(gpu, plain, cells):
    vol, meshes, wants = plain
    mesh, want = meshes["plain"], wants[("plain", cells)]
    h = vol._need()
    n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    assert n.value == len(mesh["cells"])
    capi.check(gpu.tsdf_hip_march_decimate(h, cells * VOXEL, C.byref(m), C.byref(k)), "march_decimate")
    assert (m.value, k.value) == (len(want.counts), len(want.polygons))
    assert_indexed(fetch_indexed(gpu, h, m.value, k.value), mesh, want)
    st = stats(gpu)
    assert st[:3] == [len(mesh["vertices"]), len(want.counts), int(want.duplicate.sum())]
    # the soup is still fetched unchanged
    verts, rgb = np.empty_like(mesh["vertices"]), np.empty_like(mesh["rgb"])
    capi.check(gpu.tsdf_hip_march_fetch(h, capi.as_f32p(verts), capi.as_u8p(rgb), None), "march_fetch")
    assert np.array_equal(verts.view(np.uint32), mesh["vertices"].view(np.uint32)) and np.array_equal(rgb, mesh["rgb"])


@pytest.mark.parametrize("cells", CELLS)
def test_the_same_after_a_cleanup_that_removes_something(gpu, plain, cells):
    vol, meshes, wants = plain
    assert_indexed(reconstruct(vol, cleanup=(V_FD, 40), decimate=cells * VOXEL), meshes["cleaned"], wants[("cleaned", cells)])
    verts = np.empty_like(meshes["cleaned"]["vertices"])
    capi.check(gpu.tsdf_hip_march_fetch(vol._need(), capi.as_f32p(verts), None, None), "march_fetch")
    assert np.array_equal(verts.view(np.uint32), meshes["cleaned"]["vertices"].view(np.uint32))


def test_a_later_march_cleanup_or_flatten_invalidates_or_replaces_the_indexed_mesh(gpu, plain):
    vol, meshes, wants = plain
    mesh, want = meshes["plain"], wants[("plain", 2)]
    h = vol._need()
    n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    again = np.empty((len(want.counts), 3), F32)

    def decimate():
        capi.check(gpu.tsdf_hip_march_decimate(h, 2 * VOXEL, C.byref(m), C.byref(k)), "march_decimate")
        assert (m.value, k.value) == (len(want.counts), len(want.polygons))
        capi.check(gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None), "march_fetch_indexed")
        assert np.array_equal(again.view(np.uint32), want.vertices.view(np.uint32))

    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    decimate()
    capi.check(gpu.tsdf_hip_march_cleanup(h, V_FD, 0, C.byref(n)), "march_cleanup")  # (min_neighbors 0 removes nothing)
    assert n.value == len(mesh["cells"])
    assert gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None) == capi.E_INVALID
    decimate()
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    assert gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None) == capi.E_INVALID
    decimate()
    # flatten replaces it: the indexed mesh is then flatten's (more vertices: it only merges the exact copies), and back
    capi.check(gpu.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
    assert m.value > len(want.counts)
    flat = fetch_indexed(gpu, h, m.value, k.value)
    assert len(flat["vertices"]) == m.value and len(np.unique(flat["vertices"], axis=0)) == m.value
    decimate()
    # a bad cell size is refused
    assert gpu.tsdf_hip_march_decimate(h, 0.0, C.byref(m), C.byref(k)) == capi.E_INVALID


def test_decimate_before_the_first_march_is_refused(gpu):
    vol, _ = make_volume(RES, W, H)
    vol.reset()
    m, k = C.c_uint64(0), C.c_uint64(0)
    assert gpu.tsdf_hip_march_decimate(vol._need(), VOXEL, C.byref(m), C.byref(k)) == capi.E_INVALID
    assert gpu.tsdf_hip_march_fetch_indexed(vol._need(), None, None, None, None) == capi.E_INVALID
    vol.close()


def test_decimate_on_a_multi_gpu_set_equals_one_handle(gpu, plain):
    _, meshes, wants = plain
    mesh = meshes["plain"]
    vol = fused_volume(devices=[0, 0, 0])
    try:
        soup = reconstruct(vol)
        assert np.array_equal(soup["cells"], mesh["cells"])
        for cells in CELLS:
            assert_indexed(reconstruct(vol, decimate=cells * VOXEL), mesh, wants[("plain", cells)])
        assert_indexed(reconstruct(vol, cleanup=(V_FD, 40), decimate=2 * VOXEL), meshes["cleaned"], wants[("cleaned", 2)])
    finally:
        vol.close()


def test_reconstruct_with_set_decimate(gpu, plain):
    vol, meshes, wants = plain
    for cells in CELLS:
        assert_indexed(reconstruct(vol, decimate=cells * VOXEL), meshes["plain"], wants[("plain", cells)])
    # with setFlatten as well, decimate runs and flatten is skipped
    assert_indexed(reconstruct(vol, decimate=2 * VOXEL, flatten=1e-4), meshes["plain"], wants[("plain", 2)])
    assert_indexed(reconstruct(vol, cleanup=(V_FD, 40), decimate=2 * VOXEL, flatten=1e-4), meshes["cleaned"], wants[("cleaned", 2)])
    # clearDecimate gives the soup back
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    mc.setDecimate(VOXEL)
    mc.clearDecimate()
    soup = mc.reconstruct(want_cells=True)
    assert np.array_equal(soup["vertices"].view(np.uint32), meshes["plain"]["vertices"].view(np.uint32))
    assert np.array_equal(soup["polygons"], meshes["plain"]["polygons"]) and np.array_equal(soup["cells"], meshes["plain"]["cells"])
