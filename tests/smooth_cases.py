"""The cases of the smoothMesh tests and a numpy model of the rule (include/tsdf_hip.h, tsdf_hip_mesh_smooth), written
without looking at cpu_tsdf::mesh_post::smoothArrays: np.unique on the directed edge keys gives the neighbour lists and the
edge multiplicities, np.add.at -- which adds one element at a time, in index order -- gives the sums in the rule's order,
the step is float64 element operations, and a `where` on the fixed mask keeps the words of a fixed vertex.
tests/test_smooth_oracle.py pins the host pass to this model on the CPU tier; tests/test_smooth_gpu.py the GPU pass."""
import functools

import numpy as np

F32 = np.float32
U32 = np.uint32
NAN_BITS = 0x7FC12345  # a quiet NaN with a payload
NO_FACES = np.empty((0, 3), U32)


class Model:
    """The rule on (verts n x 3 float32, faces k x 3).  descending: the sums take the neighbours in DESCENDING index, which
    is not the rule -- only there to show that a case can tell the orders apart."""

    def __init__(self, verts, faces, lam=0.5, mu=-0.53, iterations=10, keep_boundary=1, descending=False):
        verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.uint64).reshape(-1, 3)
        n = len(verts)
        assert not len(f) or int(f.max()) < n
        a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
        b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
        a, b = a[a != b], b[a != b]
        # a directed key (a, b) appears once per corner pair that names {a, b}, in whichever direction
        keys, mult = np.unique(np.concatenate([(a << np.uint64(32)) | b, (b << np.uint64(32)) | a]), return_counts=True)
        src, dst = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if descending:
            order = np.lexsort((-dst, src))
            src, dst = src[order], dst[order]
        self.src, self.dst = src, dst
        self.n_edges = len(keys) // 2
        self.degree = np.bincount(src, minlength=n).astype(U32)
        self.boundary = np.zeros(n, bool)
        self.boundary[src[mult == 1]] = True
        bad = ~np.isfinite(verts).all(1)
        bad_nbr = np.zeros(n, bool)
        bad_nbr[src[bad[dst]]] = True
        self.fixed = ((bad | bad_nbr) * 1 + (self.degree == 0) * 2 + (self.boundary & (keep_boundary != 0)) * 4).astype(np.uint8)
        x = verts.copy()
        self.steps = 0
        for _ in range(int(iterations)):
            x = self._step(x, F32(lam))
            if F32(mu) != 0:
                x = self._step(x, F32(mu))
        self.vertices = x
        self.n_fixed = int((self.fixed != 0).sum())

    def _step(self, x, f):
        self.steps += 1
        p = x.astype(np.float64)
        s = np.zeros_like(p)  # +0.0
        np.add.at(s, self.src, p[self.dst])
        with np.errstate(all="ignore"):
            m = s / self.degree.astype(np.float64)[:, None]
            new = (p + np.float64(f) * (m - p)).astype(F32)
        return np.where((self.fixed != 0)[:, None], x.view(U32), new.view(U32)).view(F32)


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.asarray([[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0.1], [0.3, 0.2, 1]], F32)
    return v, np.asarray([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], U32)


def grid_patch(w=5, seed=1):
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(w), np.arange(w), indexing="ij"), -1).reshape(-1, 2)
    v = np.concatenate([ij * 0.1 + rng.normal(0, 0.01, ij.shape), rng.normal(0, 0.03, (len(ij), 1))], 1).astype(F32)
    faces = []
    for i in range(w - 1):
        for j in range(w - 1):
            q = i * w + j
            faces += [[q, q + 1, q + w], [q + 1, q + w + 1, q + w]]
    return v, np.asarray(faces, U32)


def fan(rim=300, hubs=1, seed=2):
    """hubs == 1: a disc, hub 0 of degree `rim` over a boundary rim.  hubs == 2: closed, two hubs over one rim."""
    rng = np.random.default_rng(seed)
    t = np.arange(rim) * (2 * np.pi / rim)
    ring = np.stack([np.cos(t), np.sin(t), rng.normal(0, 0.05, rim)], 1)
    tops = [[0.1, -0.2, 0.7], [-0.05, 0.1, -0.6]][:hubs]
    v = np.concatenate([np.asarray(tops), ring]).astype(F32)
    r = hubs + np.arange(rim)
    nxt = hubs + (np.arange(rim) + 1) % rim
    faces = [np.stack([np.zeros(rim, int), r, nxt], 1)]
    if hubs == 2:
        faces.append(np.stack([np.ones(rim, int), nxt, r], 1))
    return v, np.concatenate(faces).astype(U32)


def strip(n, seed=3):
    rng = np.random.default_rng(seed + n)
    i = np.arange(n)
    v = np.stack([i * 0.05, (i & 1) * 0.05 + rng.normal(0, 0.005, n), rng.normal(0, 0.01, n)], 1).astype(F32)
    faces = np.stack([i[:-2], i[1:-1], i[2:]], 1).astype(U32) if n >= 3 else NO_FACES
    return v, faces


def unreferenced():
    """12 vertices; 0, 5 and 11 are in no face, the highest referenced one is 10 = n - 2"""
    v, _ = strip(12, seed=4)
    used = [1, 2, 3, 4, 6, 7, 8, 9, 10]
    faces = np.asarray([[used[k], used[k + 1], used[k + 2]] for k in range(len(used) - 2)], U32)
    return v, faces


def odd_faces():
    """a face given twice (edges of multiplicity 2: no boundary), three faces on the edge 4-5, degenerate faces"""
    rng = np.random.default_rng(6)
    v = rng.normal(0, 1, (14, 3)).astype(F32)
    faces = [[0, 1, 2], [0, 1, 2],              # twice: 0, 1, 2 are on no boundary edge
             [4, 5, 6], [4, 5, 7], [5, 4, 8],   # 4-5 has multiplicity 3; 4-6, 5-6 .. are boundary
             [9, 9, 10],                        # contributes 9-10 with multiplicity 2 (the pairs 9-10 and 10-9)
             [11, 11, 11],                      # contributes nothing: 11 stays without a neighbour
             [12, 13, 13], [12, 3, 13]]
    return v, np.asarray(faces, U32)


def non_finite():
    """a strip of 24: vertex 5 is NaN with a payload, 15 has an infinite component, 6 (a neighbour of 5) a -0.0"""
    v, faces = strip(24, seed=7)
    v = v.copy()
    v.view(U32)[5, 1] = NAN_BITS
    v[15, 2] = np.inf
    v[6, 2] = -0.0
    return v, faces


def random_mesh():
    rng = np.random.default_rng(11)
    n = 2000
    v = (10.0 ** rng.uniform(-3, 3, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F32)
    return v, rng.integers(0, n, (6000, 3)).astype(U32)


def add_order():
    """vertex 0 has the neighbours 1, 2, 3, 4 with x = 1, 1, 2^60, -2^60: ascending, the sum is ((1 + 1) + 2^60) - 2^60 = 0 (the
    2 is below the double's last bit at 2^60); descending, ((-2^60 + 2^60) + 1) + 1 = 2"""
    v = np.asarray([[0, 0, 0], [1, 1, 0], [1, -1, 0], [2.0 ** 60, 0, 1], [-2.0 ** 60, 0, -1]], F32)
    return v, np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], U32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (verts, faces, lambda, mu, iterations, keep_boundary)"""
    out = {}
    out["tetrahedron"] = tetrahedron() + (0.5, -0.53, 4, 1)
    out["tetrahedron_range_ends"] = tetrahedron() + (1.0, -1.0, 3, 1)
    for kb in (0, 1):
        out[f"grid_keep{kb}"] = grid_patch() + (0.5, -0.53, 5, kb)
    out["grid_range_ends"] = grid_patch() + (1.0, -1.0, 2, 1)
    for it, mu in ((1, 0.0), (1, -0.53), (2, 0.0), (3, -0.53), (0, -0.53)):
        out[f"grid_steps_{it}_{'mu' if mu else 'nomu'}"] = grid_patch(6, seed=8) + (0.5, mu, it, 1)
    out["fan_300"] = fan(300, 1) + (0.5, -0.53, 3, 1)
    out["fan_300_free_rim"] = fan(300, 1) + (0.5, -0.53, 2, 0)
    out["double_fan_300"] = fan(300, 2) + (0.5, -0.53, 3, 1)
    for n in (1, 255, 256, 257):
        out[f"strip_{n}"] = strip(n) + (0.5, -0.53, 3, 0)
    out["strip_257_keep"] = strip(257) + (0.5, -0.53, 1, 1)
    out["unreferenced"] = unreferenced() + (0.5, -0.53, 3, 0)
    for kb in (0, 1):
        out[f"odd_faces_keep{kb}"] = odd_faces() + (0.5, -0.53, 3, kb)
    out["non_finite"] = non_finite() + (0.5, -0.53, 3, 0)
    out["add_order"] = add_order() + (0.5, 0.0, 1, 0)
    out["random"] = random_mesh() + (0.5, -0.53, 3, 0)
    out["random_keep"] = random_mesh() + (0.6, 0.0, 2, 1)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(*cases()[name])


def icosphere(subdivisions):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.asarray(v), np.asarray(f, U32)
