"""Shared by the flattenVertices tests: the oracle and the cases.

The oracle is a pure numpy restatement of the SEQUENTIAL host loop of cpu_tsdf::mesh_post::flattenVertices
(csrc/prog/mesh_post.h:92-118): a dict grid of cell min_dist keyed as PointGrid::key does (21-bit masks included), vertices
visited in index order, an unassigned vertex opens an output vertex and overwrites the entry of every vertex that passes the
float32 test (ex*ex + ey*ey) + ez*ez < thr against it, assigned or not.  It is never the three rules the GPU pass is derived
from (include/tsdf_hip.h): a wrong derivation cannot agree with itself.

Every case is built so that the oracle alone merges at least one vertex and keeps at least two, and, where faces exist,
drops at least one face and keeps at least one (Flat.check_mixed)."""
import numpy as np

F32 = np.float32
MD = 1e-4
MASK = 0x1fffff
AROUND = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def threshold(min_dist):
    md = F32(min_dist)
    r2 = F32(np.float64(md) * np.float64(md))
    return r2 if r2 < md else md  # mesh_post.h:103: the squared distance is also compared with min_dist itself


def cells_of(verts, min_dist):
    """floor((double)v / (double)min_dist) per axis, from the float32 values (finite vertices only; others get 0)."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    fin = np.isfinite(v).all(1)
    cell = np.zeros((len(v), 3), np.int64)
    cell[fin] = np.floor(v[fin].astype(np.float64) / np.float64(F32(min_dist))).astype(np.int64)
    return cell, fin


class Flat:
    """Result of the sequential loop: remap (n,), seeds (m,), polygons (k, 3), keep (faces,), and the grid for questions."""

    def __init__(self, verts, faces=None, min_dist=MD):
        self.v = v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        self.thr = threshold(min_dist)
        n = len(v)
        self.cell, self.fin = cells_of(v, min_dist)
        grid = {}
        for i in np.flatnonzero(self.fin):
            grid.setdefault(tuple(int(c) & MASK for c in self.cell[i]), []).append(i)
        self.grid = {k: np.asarray(b, np.int64) for k, b in grid.items()}
        remap = np.full(n, -1, np.int64)
        seeds = []
        for i in range(n):
            if remap[i] >= 0:
                continue
            idx = len(seeds)
            remap[i] = idx
            remap[self.neighbours(i)] = idx
            seeds.append(i)
        self.remap = remap.astype(np.uint32)
        self.seeds = np.asarray(seeds, np.uint32)
        if faces is None:
            faces = np.arange(n - n % 3, dtype=np.int64).reshape(-1, 3)
        mapped = self.remap[np.asarray(faces, np.int64).reshape(-1, 3)]
        self.keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0])
        self.polygons = mapped[self.keep].astype(np.int32)
        self.vertices = v[self.seeds.astype(np.int64)]

    def neighbours(self, i):
        """PointGrid::forNeighbours without i itself, in any order."""
        if not self.fin[i]:
            return np.empty(0, np.int64)
        cx, cy, cz = (int(c) for c in self.cell[i])
        cand = [self.grid[k] for k in (((cx + dx) & MASK, (cy + dy) & MASK, (cz + dz) & MASK) for dx, dy, dz in AROUND) if k in self.grid]
        cand = np.concatenate(cand)
        e = self.v[cand] - self.v[i]
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        return cand[(d2 < self.thr) & (cand != i)]

    def check_mixed(self, faces=True):
        n, m = len(self.remap), len(self.seeds)
        assert 2 <= m < n, (m, n)
        if faces:
            assert 1 <= int(self.keep.sum()) < len(self.keep), (int(self.keep.sum()), len(self.keep))
        return self


# ---- cases: name -> (vertices, faces or None, min_dist, faces take part) -------------------------------------------------------
def dense_cloud():
    return (np.random.RandomState(1).uniform(0.0, 12.0 * MD, (4000, 3))).astype(F32)


def exact_duplicates():
    rng = np.random.RandomState(2)
    pts = rng.uniform(-0.5, 0.5, (800, 3)).astype(F32)
    return np.ascontiguousarray(np.repeat(pts, 5, axis=0)[rng.permutation(4000)])


def chain(order="index"):
    c = np.zeros((500, 3), F32)
    c[:, 0] = (np.arange(500) * (0.9 * MD)).astype(F32)
    c[:, 1], c[:, 2] = F32(0.25), F32(-0.125)
    if order == "shuffled":
        c = c[np.random.RandomState(3).permutation(500)]
    elif order == "reversed":
        c = c[::-1]
    return np.ascontiguousarray(c)


def strict_pairs():
    md = F32(MD)
    return np.asarray([[0, 0, 0], [md, 0, 0], [0, 1, 0], [np.nextafter(md, F32(0)), 1, 0]], F32)


def strict_pairs_2():
    """min_dist 2.0: the threshold is 2.0, not 4.0."""
    return np.asarray([[0, 0, 0], [1.5, 0, 0], [0, 10, 0], [1.4, 10, 0]], F32)


def cell_borders():
    u = np.float64(MD)
    return (np.asarray([[-1.05, -25, -15], [-0.95, -25, -15],        # one border, negative side
                        [10.95, 10.95, 10.95], [11.05, 11.05, 11.05],  # diagonal cells
                        [-0.05, -0.05, -0.05], [0.05, 0.05, 0.05],     # across the origin on all three axes
                        [25, 25, 25], [-35, 5, 5], [2.5, -25, -15]], np.float64) * u).astype(F32)


def big_bucket():
    rng = np.random.RandomState(11)
    base = np.asarray([3, -4, 7], np.float64) * MD
    bucket = (base + rng.uniform(0.1, 0.9, (3000, 3)) * MD).astype(F32)
    singles = (base + np.asarray([[5, 0, 0], [0, 5, 0], [0, 0, -5], [9, 9, 9]], np.float64) * MD + 0.5 * MD).astype(F32)
    return np.concatenate([bucket, singles])


def nan_cloud(with_bad=True):
    base = np.random.RandomState(5).uniform(0.0, 10.0 * MD, (2000, 3)).astype(F32)
    if not with_bad:
        return base
    bad = np.asarray([[base[7, 0], np.nan, base[7, 2]], [np.inf, base[9, 1], base[9, 2]]], F32)
    return np.concatenate([base[:300], bad, base[300:]])


NAN_AT = (300, 301)
SNAP_MD = 0.0101  # lattice neighbours of the snapped mesh (0.01 apart) merge, diagonal ones do not


def snapped_mesh():
    """The random cloud of tests/test_meshpost_gpu.py as small triangles with corners on a 1 cm lattice, shared between
    faces.  Flattened with SNAP_MD, corners one lattice step apart merge: many faces become degenerate."""
    from tests.test_meshpost_gpu import indexed_random_mesh
    return indexed_random_mesh(seed=7, n=4000)


def cases():
    pool, faces = snapped_mesh()
    return {
        "dense_cloud": (dense_cloud(), None, MD, False),
        "exact_duplicates": (exact_duplicates(), None, MD, False),
        "chain_index": (chain("index"), None, MD, False),
        "chain_shuffled": (chain("shuffled"), None, MD, False),
        "chain_reversed": (chain("reversed"), None, MD, False),
        "strict_pairs": (strict_pairs(), None, MD, False),
        "strict_pairs_2": (strict_pairs_2(), None, 2.0, False),
        "cell_borders": (cell_borders(), None, MD, False),
        "big_bucket": (big_bucket(), None, MD, False),
        "nan_cloud": (nan_cloud(), None, MD, False),
        "snapped_indexed": (pool, faces, SNAP_MD, True),
        "snapped_soup": (np.ascontiguousarray(pool[faces.astype(np.int64)].reshape(-1, 3)), None, SNAP_MD, True),
    }


_ORACLES = {}


def oracle(name):
    """The oracle of a named case, computed once per process and left unchanged."""
    if name not in _ORACLES:
        verts, faces, md, with_faces = cases()[name]
        _ORACLES[name] = Flat(verts, faces, md).check_mixed(with_faces)
    return _ORACLES[name]
