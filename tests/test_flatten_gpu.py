"""GPU tier: flattenVertices on the GPU (tsdf_hip_mesh_flatten / tsdf_hip_march_flatten) against the numpy restatement of
the SEQUENTIAL host loop in tests/flatten_cases.py (which tests/test_flatten_oracle.py pins to the host pass itself).  Every
comparison is exact -- remap, seeds, output vertex bits, polygons: no tolerance, no exempt share -- and every case is one
on which the oracle alone merges at least one vertex and keeps at least two (and drops and keeps a face where faces exist)."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, flatten_mesh
from tests import flatten_cases as fc
from tests.common import make_volume
from tests.test_meshpost_gpu import H, RES, V_FD, W, fused_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
MD = fc.MD
NO_FACES = np.empty((0, 3), np.uint32)


def stats(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_flatten_stats(out) == capi.OK
    return list(out)


def assert_equals_oracle(got, want, with_faces):
    assert got["remap"].dtype == np.uint32 and got["seeds"].dtype == np.uint32 and got["polygons"].dtype == np.int32
    bad = np.flatnonzero(got["remap"] != want.remap) if got["remap"].shape == want.remap.shape else None
    assert bad is not None and len(bad) == 0, f"{len(bad)} of {len(want.remap)} remap entries differ, first {bad[:8].tolist()}"
    assert np.array_equal(got["seeds"], want.seeds)
    assert got["vertices"].dtype == F32 and np.array_equal(got["vertices"].view(np.uint32), want.vertices.view(np.uint32))
    if with_faces:
        assert np.array_equal(got["polygons"], want.polygons)
    else:
        assert got["polygons"].shape == (0, 3)


def check(gpu, name):
    verts, faces, md, with_faces = fc.cases()[name]
    want = fc.oracle(name)
    got = flatten_mesh(verts, faces if with_faces else NO_FACES, md)
    assert_equals_oracle(got, want, with_faces)
    st = stats(gpu)
    assert st[0] == len(verts) and st[1] == len(want.seeds)
    return want, got, st


# ---- vertices --------------------------------------------------------------------------------------------------------------
def test_dense_cloud_shows_the_last_writer_rule(gpu):
    want, _, st = check(gpu, "dense_cloud")
    is_seed = np.zeros(len(want.remap), bool)
    is_seed[want.seeds] = True
    differ = 0
    for j in np.flatnonzero(~is_seed)[:400]:
        nb = want.neighbours(j)
        differ += int(want.remap[j] != want.remap[nb[is_seed[nb]].min()])
    assert differ > 0  # a merged vertex whose remap is not its lowest seed neighbour's
    assert st[2] >= 3


def test_exact_duplicates(gpu):
    want, _, _ = check(gpu, "exact_duplicates")
    assert len(want.seeds) == 800


def test_chains_depth_and_visiting_order(gpu):
    want, _, st = check(gpu, "chain_index")
    assert want.seeds.tolist() == list(range(0, 500, 2))
    assert st[2] >= 250  # depth is the point: vertex k waits for vertex k - 1
    check(gpu, "chain_shuffled")
    rev, _, _ = check(gpu, "chain_reversed")
    # the visiting order changes the seeds: the reversed chain keeps the other half of the positions
    assert not np.array_equal(np.sort(rev.vertices[:, 0]), np.sort(want.vertices[:, 0]))


def test_the_neighbour_test_is_strict_and_squared_once_more(gpu):
    md = F32(MD)
    v = fc.strict_pairs()
    e = v[1] - v[0]
    assert (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] == fc.threshold(MD)  # equal in float32: not below
    assert v[3, 0] - v[2, 0] == np.nextafter(md, F32(0))
    want, _, _ = check(gpu, "strict_pairs")
    assert want.remap.tolist() == [0, 1, 2, 2]
    assert fc.threshold(2.0) == F32(2.0)
    want, _, _ = check(gpu, "strict_pairs_2")
    assert want.remap.tolist() == [0, 1, 2, 2]  # 1.5 apart: 2.25 >= 2 stays; 1.4 apart: 1.96 < 2 merges


def test_cell_borders_negative_coordinates_and_diagonal_cells(gpu):
    v = fc.cell_borders()
    cell, _ = fc.cells_of(v, MD)
    assert (cell[0] - cell[1]).tolist() == [-1, 0, 0] and cell[0, 0] < 0
    assert (cell[3] - cell[2]).tolist() == [1, 1, 1]
    assert (cell[5] - cell[4]).tolist() == [1, 1, 1] and (cell[4] == -1).all()
    want, _, _ = check(gpu, "cell_borders")
    assert want.remap.tolist() == [0, 0, 1, 1, 2, 2, 3, 4, 5]


def test_a_bucket_larger_than_a_block(gpu):
    v = fc.big_bucket()
    cell, _ = fc.cells_of(v[:3000], MD)
    assert (cell == cell[0]).all()
    want, _, _ = check(gpu, "big_bucket")
    assert np.isin(np.arange(3000, 3004), want.seeds).all()


def test_a_nan_or_inf_vertex_is_a_seed_of_its_own(gpu):
    want, got, _ = check(gpu, "nan_cloud")
    base = flatten_mesh(fc.nan_cloud(with_bad=False), NO_FACES, MD)
    for at in fc.NAN_AT:
        assert at in got["seeds"] and int((got["remap"] == got["remap"][at]).sum()) == 1
    others = np.setdiff1d(np.arange(len(got["remap"])), fc.NAN_AT)
    # up to renumbering: the same seeds, and every vertex lands on the same position
    seeds = got["seeds"][~np.isin(got["seeds"], fc.NAN_AT)].astype(np.int64)
    assert np.array_equal(np.where(seeds > fc.NAN_AT[-1], seeds - len(fc.NAN_AT), seeds), base["seeds"])
    assert np.array_equal(got["vertices"][got["remap"][others]].view(np.uint32), base["vertices"][base["remap"]].view(np.uint32))


# ---- faces -----------------------------------------------------------------------------------------------------------------
def test_faces_are_reindexed_dropped_and_keep_their_order(gpu):
    want, got, _ = check(gpu, "snapped_indexed")
    assert 0 < len(got["polygons"]) < len(want.keep)
    check(gpu, "snapped_soup")
    # with a min_dist below the lattice step only the soup's exact copies merge: it gives the indexed mesh's vertices back
    pool, faces = fc.snapped_mesh()
    soup = np.ascontiguousarray(pool[faces.astype(np.int64)].reshape(-1, 3))
    back = flatten_mesh(soup, None, MD)
    assert np.array_equal(np.unique(back["vertices"], axis=0).view(np.uint32), pool.view(np.uint32)) and len(back["vertices"]) == len(pool)
    distinct = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])
    assert np.array_equal(back["vertices"][back["polygons"]].view(np.uint32), pool[faces[distinct].astype(np.int64)].view(np.uint32))
    # a face that names a vertex beyond the array is refused
    faces = faces.copy()
    faces[123, 1] = len(pool)
    with pytest.raises(capi.TsdfHipError) as e:
        flatten_mesh(pool, faces, fc.SNAP_MD)
    assert e.value.code == capi.E_INVALID


def test_empty_inputs(gpu):
    got = flatten_mesh(np.empty((0, 3), F32), None, MD)
    assert got["vertices"].shape == (0, 3) and got["polygons"].shape == (0, 3) and got["remap"].shape == (0,) and got["seeds"].shape == (0,)
    assert stats(gpu) == [0, 0, 0, 0]
    got = flatten_mesh(fc.strict_pairs(), NO_FACES, MD)
    assert got["polygons"].shape == (0, 3) and len(got["seeds"]) == 3


# ---- on a volume -----------------------------------------------------------------------------------------------------------
def reconstruct(vol, cleanup=None, flatten=None):
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if cleanup:
        mc.setCleanup(*cleanup)
    if flatten:
        mc.setFlatten(flatten)
    return mc.reconstruct(want_cells=True)


@pytest.fixture(scope="module")
def plain(gpu):
    vol = fused_volume()
    mesh = reconstruct(vol)
    want = fc.Flat(mesh["vertices"], None, MD).check_mixed()
    yield vol, mesh, want
    vol.close()


def assert_indexed(got, soup, want):
    assert np.array_equal(got["vertices"].view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(got["polygons"], want.polygons)
    assert np.array_equal(got["rgb"], soup["rgb"][want.seeds.astype(np.int64)])
    assert np.array_equal(got["cells"], soup["cells"][want.keep])
    assert len(got["vertices"]) < len(soup["vertices"])


def test_reconstruct_with_flatten_is_the_oracle_on_the_plain_soup(gpu, plain):
    vol, mesh, want = plain
    got = reconstruct(vol, flatten=MD)
    assert_indexed(got, mesh, want)
    st = stats(gpu)
    assert st[0] == len(mesh["vertices"]) and st[1] == len(want.seeds) and st[2] >= 2
    # the soup is still there
    h = vol._need()
    verts = np.empty_like(mesh["vertices"])
    capi.check(gpu.tsdf_hip_march_fetch(h, capi.as_f32p(verts), None, None), "march_fetch")
    assert np.array_equal(verts.view(np.uint32), mesh["vertices"].view(np.uint32))
    # a second fetch of the indexed mesh gives the same; a cleanup or a march makes it stale
    again = np.empty_like(got["vertices"])
    capi.check(gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None), "march_fetch_indexed")
    assert np.array_equal(again.view(np.uint32), got["vertices"].view(np.uint32))
    n = C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march_cleanup(h, V_FD, 0, C.byref(n)), "march_cleanup")  # (min_neighbors 0 removes nothing)
    assert n.value == len(mesh["cells"])
    assert gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None) == capi.E_INVALID
    m, k = C.c_uint64(0), C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march_flatten(h, MD, C.byref(m), C.byref(k)), "march_flatten")
    assert (m.value, k.value) == (len(want.seeds), len(want.polygons))
    capi.check(gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None), "march_fetch_indexed")
    capi.check(gpu.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    assert gpu.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(again), None, None, None) == capi.E_INVALID
    # clearFlatten gives the soup back
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    mc.setFlatten(MD)
    mc.clearFlatten()
    soup = mc.reconstruct(want_cells=True)
    assert np.array_equal(soup["vertices"].view(np.uint32), mesh["vertices"].view(np.uint32))
    assert np.array_equal(soup["polygons"], mesh["polygons"]) and np.array_equal(soup["cells"], mesh["cells"])


def test_cleanup_runs_first_and_flatten_second(gpu, plain):
    vol, mesh, _ = plain
    cleaned = reconstruct(vol, cleanup=(V_FD, 40))
    assert 0 < len(cleaned["cells"]) < len(mesh["cells"])
    want = fc.Flat(cleaned["vertices"], None, MD).check_mixed()
    assert_indexed(reconstruct(vol, cleanup=(V_FD, 40), flatten=MD), cleaned, want)


def test_flatten_on_a_multi_gpu_set_equals_one_handle(gpu, plain):
    _, mesh, want = plain
    vol = fused_volume(devices=[0, 0, 0])
    try:
        soup = reconstruct(vol)
        assert np.array_equal(soup["cells"], mesh["cells"])
        assert_indexed(reconstruct(vol, flatten=MD), mesh, want)
        # the set's soup stays too
        verts = np.empty_like(mesh["vertices"])
        capi.check(gpu.tsdf_hip_march_fetch(vol._need(), capi.as_f32p(verts), None, None), "march_fetch")
        assert np.array_equal(verts.view(np.uint32), mesh["vertices"].view(np.uint32))
    finally:
        vol.close()


def test_flatten_before_the_first_march_is_refused(gpu):
    vol, _ = make_volume(RES, W, H)
    vol.reset()
    m, k = C.c_uint64(0), C.c_uint64(0)
    assert gpu.tsdf_hip_march_flatten(vol._need(), MD, C.byref(m), C.byref(k)) == capi.E_INVALID
    assert gpu.tsdf_hip_march_fetch_indexed(vol._need(), None, None, None, None) == capi.E_INVALID
    vol.close()
