"""GPU tier: the host-array entry points of the three mesh passes on a mesh LARGER than their pinned staging buffer.

Pageable caller memory goes through two pinned slots of 4 MiB (MP_STAGE; MpCall::upload / download in csrc/tsdf_meshgrid.h,
on the library's one PinnedStage); every other mesh of the suite fits one slot.  Here the vertices are 12.6 MB -- four chunks on the way in, so both slots are
used twice and the wait for a slot's earlier copy runs -- and remap is 4.2 MB: two chunks on the way back.  The soup is a
lattice on which every result is known by construction (no model runs at this size):
  vertex v = (v % 1024, (v / 1024) % 1024, v / 1048576), face f = vertices 3f, 3f+1, 3f+2
Integer coordinates, so at a cell of 0.5 every vertex has a cell of its own and at a distance of 0.25 none has a neighbour;
the face centroids are distinct integer points, except the 684 faces that straddle two rows, which lie 0.745 from the
nearest other centroid: at a face distance of 0.5 no face has a link."""
import ctypes as C

import numpy as np
import pytest

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import cleanup_mesh, flatten_mesh
from tests.test_decimate_gpu import run_abi

pytestmark = pytest.mark.gpu
F32 = np.float32
N_FACES = 350_000
N_VERTS = 3 * N_FACES
SOUP_FACES = np.arange(N_VERTS, dtype=np.int32).reshape(-1, 3)


@pytest.fixture(scope="module")
def lattice():
    v = np.arange(N_VERTS)
    verts = np.stack([v % 1024, (v // 1024) % 1024, v // 1048576], 1).astype(F32)
    verts.setflags(write=False)
    assert verts.nbytes > 3 * (4 << 20) and 4 * N_VERTS > (4 << 20)  # more than three chunks in, more than one out
    return verts


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_decimate_with_a_cell_per_vertex_is_the_identity(gpu, lattice):
    got = run_abi(gpu, lattice, None, None, 0.5)
    assert got["rc"] == capi.OK
    assert np.array_equal(got["remap"], np.arange(N_VERTS, dtype=np.uint32))
    assert same_bits(got["vertices"], lattice)
    assert got["counts"].shape == (N_VERTS,) and (got["counts"] == 1).all()
    assert np.array_equal(got["polygons"], SOUP_FACES)


def test_flatten_without_neighbours_is_the_identity_in_one_round(gpu, lattice):
    got = flatten_mesh(lattice, None, 0.25)
    assert np.array_equal(got["remap"], np.arange(N_VERTS, dtype=np.uint32))
    assert np.array_equal(got["seeds"], np.arange(N_VERTS, dtype=np.uint32))
    assert np.array_equal(got["polygons"], SOUP_FACES)
    st = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_flatten_stats(st) == capi.OK
    assert st[0] == N_VERTS and st[1] == N_VERTS and st[2] == 1


@pytest.mark.parametrize("min_neighbors, kept", [(0, True), (1, False)])
def test_cleanup_without_links_keeps_all_faces_or_none(gpu, lattice, min_neighbors, kept):
    keep = cleanup_mesh(lattice, None, 0.5, min_neighbors)
    assert keep.shape == (N_FACES,) and (keep == kept).all()
    st = (C.c_uint64 * 4)()
    assert gpu.tsdf_hip_mesh_cleanup_stats(st) == capi.OK
    assert st[0] == N_FACES and st[1] == (0 if kept else N_FACES)


def test_decimate_that_averages_is_the_same_from_pageable_and_from_pinned_memory(gpu, lattice):
    cell = np.floor(lattice.astype(np.float64) / 2.0).astype(np.int64)
    n_clusters = len(np.unique((cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]))
    # (the two z planes share a cell: clusters of 2 x 2 x 2 vertices where the second plane reaches, of 2 x 2 elsewhere)
    pageable = run_abi(gpu, lattice, None, None, 2.0, pinned=False)
    pinned = run_abi(gpu, lattice, None, None, 2.0, pinned=True)
    assert pageable["rc"] == capi.OK and pinned["rc"] == capi.OK
    assert len(pageable["vertices"]) == n_clusters and int(pageable["counts"].sum()) == N_VERTS and pageable["counts"].max() == 8
    for name in ("remap", "vertices", "counts", "polygons"):
        assert same_bits(pageable[name], pinned[name]), name
