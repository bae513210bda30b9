"""GPU tier: cleanupMesh on the GPU (tsdf_hip_mesh_cleanup / tsdf_hip_march_cleanup) against a pure numpy restatement of
cpu_tsdf::mesh_post::cleanupMesh (csrc/prog/mesh_post.h:116-166): a dict grid of cell face_dist, links from the 27 cells
around a face's own with the float32 test (ex*ex + ey*ey) + ez*ez < r2, groups by BFS, a group of at most min_neighbors
faces goes.  The keep mask must equal the oracle's for EVERY face: no tolerance, no exempt share.  Every expectation is
derived from the centroids the float32 formula ((v0 + v1) + v2) / 3 gives, never from the positions a case intended.

Every case is built so that the oracle alone removes at least one face and keeps at least one (checked here), with one
exception the definition forces: min_neighbors = 0 keeps everything."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, cleanup_mesh
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
FD = 0.02
F32 = np.float32


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def centroids(verts, faces=None):
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    tri = v.reshape(-1, 3, 3) if faces is None else v[np.asarray(faces, np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        return ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / F32(3)


def oracle_groups(cen, face_dist):
    """Group label per face (BFS over the links) and the group sizes."""
    cen = np.ascontiguousarray(cen, F32)
    n = len(cen)
    fd = F32(face_dist)
    r2 = F32(np.float64(fd) * np.float64(fd))
    fin = np.isfinite(cen).all(1)
    cell = np.zeros((n, 3), np.int64)
    cell[fin] = np.floor(cen[fin].astype(np.float64) / np.float64(fd)).astype(np.int64)
    grid = {}
    for i in np.flatnonzero(fin):
        grid.setdefault((cell[i, 0], cell[i, 1], cell[i, 2]), []).append(i)
    grid = {k: np.asarray(v, np.int64) for k, v in grid.items()}
    around = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]

    def links(i):
        if not fin[i]:
            return np.empty(0, np.int64)
        cx, cy, cz = cell[i]
        cand = [grid[k] for k in ((cx + dx, cy + dy, cz + dz) for dx, dy, dz in around) if k in grid]
        cand = np.concatenate(cand)
        e = cen[cand] - cen[i]
        with np.errstate(over="ignore"):
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        return cand[d2 < r2]

    label = np.full(n, -1, np.int64)
    sizes = []
    for s in range(n):
        if label[s] >= 0:
            continue
        g = len(sizes)
        label[s] = g
        todo, size = [s], 1
        while todo:
            for j in links(todo.pop()):
                if label[j] < 0:
                    label[j] = g
                    size += 1
                    todo.append(j)
        sizes.append(size)
    return label, np.asarray(sizes, np.int64)


def oracle_keep(cen, face_dist, min_neighbors, mixed=True):
    label, sizes = oracle_groups(cen, face_dist)
    keep = sizes[label] > min_neighbors
    if mixed:  # the case says something only if the oracle alone removes a face and keeps a face
        assert keep.any() and not keep.all(), (int(keep.sum()), len(keep))
    return keep


def soup(cen):
    """Degenerate triangles: all three vertices at one point (the centroid is then whatever the float32 formula makes of it)."""
    return np.repeat(np.ascontiguousarray(cen, F32).reshape(-1, 3), 3, axis=0)


def vertex_for(c):
    """A float32 x with ((x + x) + x) / 3 == c exactly."""
    c = F32(c)
    x = c
    for _ in range(8):
        for cand in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))):
            if ((cand + cand) + cand) / F32(3) == c:
                return cand
        x = np.nextafter(x, F32(np.inf))
    raise AssertionError(f"no vertex value reproduces the centroid {c!r}")


def check(gpu, verts, faces, face_dist, min_neighbors, mixed=True):
    cen = centroids(verts, faces)
    want = oracle_keep(cen, face_dist, min_neighbors, mixed)
    got = cleanup_mesh(verts, faces, face_dist, min_neighbors)
    assert got.dtype == bool and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} of {len(want)} faces differ, first {bad[:8].tolist()}: got {got[bad[:8]].tolist()}"
    out = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_cleanup_stats(out) == capi.OK
    assert out[0] == len(want) and out[0] - out[1] == int(want.sum())
    return want, cen


# ---- cases -----------------------------------------------------------------------------------------------------------------
def random_centroids(seed=7, n=20000, side=0.63):
    return (np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 3)) * side).astype(F32)


def test_random_cloud_has_groups_on_both_sides_of_the_threshold(gpu):
    verts = soup(random_centroids())
    cen = centroids(verts)
    _, sizes = oracle_groups(cen, FD)
    assert (sizes == 5).any() and (sizes == 6).any()
    keep, _ = check(gpu, verts, None, FD, 5)
    assert 0.1 < 1.0 - keep.mean() < 0.5
    out = (C.c_uint64 * 4)()
    gpu.tsdf_hip_mesh_cleanup_stats(out)
    assert out[2] > 0


def test_chains_are_kept_by_the_transitive_closure_alone(gpu):
    """Spacing 0.9 face_dist: a face links to its two chain neighbours at most, so no face reaches min_neighbors links and
    only the group size can keep the chains of 6 and of 2000."""
    parts = []
    for k, length in enumerate((5, 6, 2000)):
        c = np.zeros((length, 3), F32)
        c[:, 0] = (np.arange(length) * (0.9 * FD) - 7.0).astype(F32)
        c[:, 1] = F32(k)
        parts.append(c)
    verts = soup(np.concatenate(parts))
    keep, cen = check(gpu, verts, None, FD, 5)
    label, sizes = oracle_groups(cen, FD)
    assert sorted(sizes.tolist()) == [5, 6, 2000]
    assert not keep[:5].any() and keep[5:].all()


def test_light_tail_of_a_heavy_blob_is_kept(gpu):
    blob = np.tile(np.asarray([[0.105, -0.033, 0.27]], F32), (50, 1))
    tail = blob[:3].copy()
    tail[:, 0] += (np.arange(1, 4) * (0.9 * FD)).astype(F32)
    singles = np.asarray([[1.0, 1.0, 1.0], [-1.0, 0.5, 0.25], [0.105, -0.033, 0.37]], F32)
    verts = soup(np.concatenate([blob, tail, singles]))
    keep, cen = check(gpu, verts, None, FD, 5)
    _, sizes = oracle_groups(cen, FD)
    assert sorted(sizes.tolist()) == [1, 1, 1, 53]
    assert keep[:53].all() and not keep[53:].any()


def test_the_link_test_is_strict(gpu):
    fd = F32(FD)
    below = np.nextafter(fd, F32(0))
    cen = np.asarray([[0, 0, 0], [fd, 0, 0], [0, 1, 0], [below, 1, 0]], F32)
    verts = np.repeat(np.asarray([[vertex_for(v) for v in row] for row in cen], F32), 3, axis=0)
    got_cen = centroids(verts)
    assert np.array_equal(got_cen, cen)
    assert got_cen[1, 0] - got_cen[0, 0] == fd and got_cen[3, 0] - got_cen[2, 0] == below
    keep, _ = check(gpu, verts, None, FD, 1)
    assert keep.tolist() == [False, False, True, True]


def test_cell_borders_negative_coordinates_and_diagonal_cells(gpu):
    cen = np.asarray([[-0.021, -0.5, -0.3], [-0.019, -0.5, -0.3],        # one border, negative side
                      [0.219, 0.219, 0.219], [0.221, 0.221, 0.221],      # diagonal cells
                      [-0.0005, -0.0005, -0.0005], [0.0005, 0.0005, 0.0005],  # across the origin on all three axes
                      [0.5, 0.5, 0.5], [-0.7, 0.1, 0.1], [0.05, -0.5, -0.3]], F32)
    verts = soup(cen)
    got_cen = centroids(verts)
    cell = np.floor(got_cen.astype(np.float64) / np.float64(F32(FD))).astype(np.int64)
    assert (cell[0] - cell[1]).tolist() == [-1, 0, 0] and cell[0, 0] < 0
    assert (cell[3] - cell[2]).tolist() == [1, 1, 1]
    assert (cell[5] - cell[4]).tolist() == [1, 1, 1] and (cell[4] == -1).all()
    keep, _ = check(gpu, verts, None, FD, 1)
    assert keep.tolist() == [True] * 6 + [False] * 3


@pytest.mark.parametrize("min_neighbors", [5, 2999])
def test_a_bucket_larger_than_a_block(gpu, min_neighbors):
    """3000 centroids in ONE cell.  With min_neighbors 5 all of them are heavy at once; with 2999 none is (no face links to
    all the others: the cell's diagonal is longer than face_dist) and the union-find carries the whole group."""
    rng = np.random.RandomState(11)
    base = np.asarray([3, -4, 7], np.float64) * FD
    bucket = (base + rng.uniform(0.1, 0.9, (3000, 3)) * FD).astype(F32)
    singles = (base + np.asarray([[5, 0, 0], [0, 5, 0], [0, 0, -5], [9, 9, 9]], np.float64) * FD + 0.5 * FD).astype(F32)
    verts = soup(np.concatenate([bucket, singles]))
    keep, cen = check(gpu, verts, None, FD, min_neighbors)
    cell = np.floor(cen[:3000].astype(np.float64) / np.float64(F32(FD))).astype(np.int64)
    assert (cell == cell[0]).all()
    assert keep[:3000].all() and not keep[3000:].any()


def test_a_nan_vertex_removes_its_face_and_nothing_else(gpu):
    cen = random_centroids(seed=3, n=2000, side=0.3)
    verts = soup(cen)
    base, _ = check(gpu, verts, None, FD, 5)
    with_nan = np.concatenate([verts[:300], np.asarray([[0.01, np.nan, 0.02], [0.01, 0.0, 0.02], [0.01, 0.0, 0.02]], F32), verts[300:]])
    keep, _ = check(gpu, with_nan, None, FD, 5)
    assert not keep[100]
    assert np.array_equal(np.delete(keep, 100), base)


def test_min_neighbors_zero_keeps_everything_and_no_face_is_accepted(gpu):
    verts = soup(random_centroids(seed=5, n=500, side=0.3))
    verts[3 * 17, 2] = np.nan
    keep, _ = check(gpu, verts, None, FD, 0, mixed=False)
    assert keep.all() and len(keep) == 500
    assert cleanup_mesh(np.empty((0, 3), F32), None, FD, 5).shape == (0,)
    assert cleanup_mesh(verts, np.empty((0, 3), np.uint32), FD, 5).shape == (0,)


def indexed_random_mesh(seed=7, n=20000):
    """The random cloud as small triangles whose corners are snapped to a 1 cm lattice and merged: faces share vertices."""
    rng = np.random.RandomState(seed)
    cen = random_centroids(seed, n)
    corners = cen[:, None, :].astype(np.float64) + rng.uniform(-0.01, 0.01, (n, 3, 3))
    snapped = (np.round(corners / 0.01) * 0.01).astype(F32).reshape(-1, 3)
    pool, inverse = np.unique(snapped, axis=0, return_inverse=True)
    faces = inverse.reshape(n, 3).astype(np.uint32)
    assert len(pool) < 0.95 * 3 * n
    return np.ascontiguousarray(pool), faces


def test_indexed_faces_give_the_mask_of_their_soup(gpu):
    pool, faces = indexed_random_mesh()
    keep, _ = check(gpu, pool, faces, FD, 5)
    as_soup = pool[faces.astype(np.int64)].reshape(-1, 3)
    assert np.array_equal(cleanup_mesh(as_soup, None, FD, 5), keep)
    # a face that names a vertex beyond the array is refused
    faces[123, 1] = len(pool)
    with pytest.raises(capi.TsdfHipError) as e:
        cleanup_mesh(pool, faces, FD, 5)
    assert e.value.code == capi.E_INVALID


# ---- on a volume -----------------------------------------------------------------------------------------------------------
RES, W, H = 64, 160, 120
# links of up to 1.5 voxels.  The four blobs leave islands of 2, 2, 4 and 4 triangles (each is about a voxel across), so
# min_neighbors 3 cuts between them and 40 takes them all; the sphere's cap and the walls are thousands of faces.
V_FD, V_MINS = 1.5 * 2.0 ** -8, (3, 40)


def fused_volume(devices=None):
    """Scene A at 64^3 with floaters: frame 0 carries isolated 2 x 2-pixel blobs in front of the far wall.  (The volume is
    0.25 m across, so the blobs stand 0.3 volume edges = 7.5 cm in front of the wall, not 0.3 m.)  Only that frame is
    fused: any other frame sees the blobs' voxels as free space, and the running mean of one in-band distance and one
    free-space 1 is never negative -- the blobs would leave no surface at all."""
    vol, sc = make_volume(RES, W, H, color=True)
    if devices:
        vol.setDevices(devices)
    vol.reset()
    for i, tr, dep, col in frames(sc, 1, 8):
        dep = dep.copy()
        for (v, u) in ((40, 60), (40, 97), (78, 61), (79, 98)):
            dep[v:v + 2, u:u + 2] -= F32(0.3 * sc.size)
        vol.integrateCloud(dep, col, tr)
    return vol


def reconstruct(vol, cleanup):
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if cleanup:
        mc.setCleanup(*cleanup)
    return mc.reconstruct(want_cells=True)


@pytest.fixture(scope="module")
def plain_mesh(gpu):
    vol = fused_volume()
    mesh = reconstruct(vol, None)
    label, sizes = oracle_groups(centroids(mesh["vertices"]), V_FD)
    keeps = {}
    for m in V_MINS:
        keeps[m] = sizes[label] > m
        assert 1 <= int((~keeps[m]).sum()) <= len(label) // 2
    assert int(keeps[3].sum()) > int(keeps[40].sum())
    yield vol, mesh, keeps
    vol.close()


def assert_filtered(got, mesh, keep):
    k3 = np.repeat(keep, 3)
    assert len(got["cells"]) == int(keep.sum())
    assert np.array_equal(got["vertices"].view(np.uint32), mesh["vertices"][k3].view(np.uint32))
    assert np.array_equal(got["rgb"], mesh["rgb"][k3])
    assert np.array_equal(got["cells"], mesh["cells"][keep])
    assert np.array_equal(got["polygons"], np.arange(3 * int(keep.sum()), dtype=np.int32).reshape(-1, 3))


@pytest.mark.parametrize("V_MIN", V_MINS)
def test_reconstruct_with_cleanup_is_the_plain_mesh_filtered_by_the_oracle(gpu, plain_mesh, V_MIN):
    vol, mesh, keeps = plain_mesh
    keep = keeps[V_MIN]
    got = reconstruct(vol, (V_FD, V_MIN))
    assert_filtered(got, mesh, keep)
    out = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_cleanup_stats(out) == capi.OK
    assert out[0] == len(keep) and out[0] - out[1] == int(keep.sum()) and out[2] > 0
    # a second cleanup with the same arguments removes nothing, and the fetch still gives the cleaned mesh
    n = C.c_uint64(0)
    capi.check(gpu.tsdf_hip_march_cleanup(vol._need(), V_FD, V_MIN, C.byref(n)), "march_cleanup")
    assert n.value == int(keep.sum())
    assert gpu.tsdf_hip_mesh_cleanup_stats(out) == capi.OK and out[0] == n.value and out[1] == 0
    verts = np.empty((3 * n.value, 3), F32)
    capi.check(gpu.tsdf_hip_march_fetch(vol._need(), capi.as_f32p(verts), None, None), "march_fetch")
    assert np.array_equal(verts.view(np.uint32), got["vertices"].view(np.uint32))
    # clearCleanup gives the plain mesh back
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    mc.setCleanup(V_FD, V_MIN)
    mc.clearCleanup()
    again = mc.reconstruct(want_cells=True)
    assert np.array_equal(again["cells"], mesh["cells"])


def test_cleanup_on_a_multi_gpu_set_equals_one_handle(gpu, plain_mesh):
    _, mesh, keeps = plain_mesh
    V_MIN = 40
    keep = keeps[V_MIN]
    vol = fused_volume(devices=[0, 0, 0])
    try:
        assert np.array_equal(reconstruct(vol, None)["cells"], mesh["cells"])
        got = reconstruct(vol, (V_FD, V_MIN))
        assert_filtered(got, mesh, keep)
        n = C.c_uint64(0)
        capi.check(gpu.tsdf_hip_march_cleanup(vol._need(), V_FD, V_MIN, C.byref(n)), "march_cleanup")
        assert n.value == int(keep.sum())
    finally:
        vol.close()


def test_cleanup_before_the_first_march_is_refused(gpu):
    vol, _ = make_volume(RES, W, H)
    vol.reset()
    n = C.c_uint64(0)
    assert gpu.tsdf_hip_march_cleanup(vol._need(), 0.02, 5, C.byref(n)) == capi.E_INVALID
    vol.close()
