"""Shared by the decimateMesh tests: the model and the cases.

The model is a pure numpy / Python restatement of the SEQUENTIAL host pass cpu_tsdf::mesh_post::decimateArrays
(csrc/prog/mesh_post.h): one loop over the vertices in index order with a dict keyed by the cell triple, float64 adds one at
a time in that order, and a set of sorted corner triples for the duplicate faces.  It is never the sort-and-scan derivation
the GPU pass uses (csrc/tsdf_decimate.hip): a wrong derivation cannot agree with itself.

Every case is built so that the model alone keeps at least two clusters, at least one of one member and at least one of
several, and, where faces take part, drops at least one degenerate face, drops at least one duplicate face and keeps at
least one (Dec.check_mixed)."""
import numpy as np

F32 = np.float32
LIMIT = 1 << 20  # cell indices live in [-LIMIT, LIMIT)


class ExtentError(ValueError):
    """A finite vertex lies in a cell outside [-2^20, 2^20): the call is refused."""


def cells_of(verts, cell_size):
    """floor((double)v / (double)cell_size) per axis, from the float32 values (finite vertices only; others get 0)."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    fin = np.isfinite(v).all(1)
    cell = np.zeros((len(v), 3), np.float64)
    with np.errstate(over="ignore"):
        cell[fin] = np.floor(v[fin].astype(np.float64) / np.float64(F32(cell_size)))
    return cell, fin


class Dec:
    """Result of the sequential pass: remap (n,), vertices (m, 3), rgb (m, 3) or None, counts (m,), polygons (k, 3), and per
    input face `degenerate`, `duplicate`, `keep`."""

    def __init__(self, verts, faces=None, colors=None, cell_size=1.0):
        self.v = v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        n = len(v)
        cell, fin = cells_of(v, cell_size)
        if ((cell < -LIMIT) | (cell >= LIMIT))[fin].any():
            raise ExtentError("a vertex lies in a cell outside [-2^20, 2^20)")
        self.cell, self.fin = cell.astype(np.int64), fin
        rgb = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        cluster_of = {}
        sums, csums, counts, first = [], [], [], []
        remap = np.zeros(n, np.int64)
        for i in range(n):
            o = len(counts)
            if fin[i]:
                o = cluster_of.setdefault((int(self.cell[i, 0]), int(self.cell[i, 1]), int(self.cell[i, 2])), o)
            if o == len(counts):
                sums.append([np.float64(0.0), np.float64(0.0), np.float64(0.0)])
                csums.append([0, 0, 0])
                counts.append(0)
                first.append(i)
            for k in range(3):
                sums[o][k] = sums[o][k] + np.float64(v[i, k])  # one float64 add per member, in index order
                if rgb is not None:
                    csums[o][k] += int(rgb[i, k])
            counts[o] += 1
            remap[i] = o
        m = len(counts)
        out = np.zeros((m, 3), F32)
        with np.errstate(over="ignore", invalid="ignore"):
            for o in range(m):
                if counts[o] == 1:
                    out[o] = v[first[o]]  # the bits themselves: no arithmetic
                else:
                    for k in range(3):
                        out[o, k] = F32(sums[o][k] / np.float64(counts[o]))  # one rounding to float
        self.remap = remap.astype(np.uint32)
        self.vertices = out
        self.counts = np.asarray(counts, np.uint32)
        self.first = np.asarray(first, np.int64)
        self.rgb = None
        if rgb is not None:
            self.rgb = np.asarray([[(2 * c + counts[o]) // (2 * counts[o]) for c in csums[o]] for o in range(m)], np.uint8).reshape(-1, 3)
        if faces is None:
            faces = np.arange(n - n % 3, dtype=np.int64).reshape(-1, 3)
        mapped = remap[np.asarray(faces, np.int64).reshape(-1, 3)]
        nf = len(mapped)
        self.degenerate, self.duplicate = np.zeros(nf, bool), np.zeros(nf, bool)
        seen = set()
        for f in range(nf):
            a, b, c = (int(x) for x in mapped[f])
            if a == b or b == c or c == a:
                self.degenerate[f] = True
                continue
            t = tuple(sorted((a, b, c)))
            if t in seen:
                self.duplicate[f] = True
            seen.add(t)
        self.keep = ~self.degenerate & ~self.duplicate
        self.polygons = mapped[self.keep].astype(np.int32).reshape(-1, 3)

    def check_mixed(self, faces=True):
        assert len(self.counts) >= 2, len(self.counts)
        assert (self.counts == 1).any() and (self.counts > 1).any()
        if faces:
            assert self.degenerate.any() and self.duplicate.any() and self.keep.any(), \
                (int(self.degenerate.sum()), int(self.duplicate.sum()), int(self.keep.sum()))
        return self


# ---- cases: name -> (vertices, faces or None, colours or None, cell_size, faces take part) -----------------------------------
def colours(seed, n):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


SINGLES = np.asarray([[100.5, 0.5, 0.5], [0.5, 100.5, 0.5], [0.5, 0.5, -100.5], [-77.5, 55.5, 33.5]], F32)


def random_cloud():
    """4000 vertices in 8 x 8 x 8 cells of edge 1: 7.8 per cell; four far singles."""
    return np.concatenate([np.random.RandomState(1).uniform(0.0, 8.0, (4000, 3)).astype(F32), SINGLES])


def exact_duplicates():
    rng = np.random.RandomState(2)
    pts = rng.uniform(-0.5, 0.5, (800, 3)).astype(F32)
    v = np.repeat(pts, 5, axis=0)[rng.permutation(4000)]
    return np.ascontiguousarray(np.concatenate([v[:1000], SINGLES[:2], v[1000:], SINGLES[2:]]))


BORDER_CELL = 0.25  # exact in binary: k * cell is exact too


def cell_borders():
    c = BORDER_CELL
    return np.asarray([[-1.05 * c, -25 * c, -15 * c], [-0.95 * c, -25 * c, -15 * c],  # 0, 1: one border, negative side: two cells
                       [-1.5 * c, -25 * c, -15 * c],                                  # 2: with 0
                       [10.95 * c, 10.95 * c, 10.95 * c], [11.05 * c, 11.05 * c, 11.05 * c],  # 3, 4: diagonal cells
                       [-0.05 * c, -0.05 * c, -0.05 * c], [0.05 * c, 0.05 * c, 0.05 * c],     # 5, 6: across the origin: cells -1 and 0
                       [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.5 * c, 0.5 * c, 0.5 * c],      # 7, 8, 9: +0 and -0 are in cell 0, with 6
                       [3 * c, 3 * c, 3 * c], [np.nextafter(F32(3 * c), F32(0)), 3 * c, 3 * c],  # 10, 11: exactly on k * cell, and just below
                       [3.5 * c, 3.5 * c, 3.5 * c],                                           # 12: with 10
                       [-0.0, 40 * c, 40 * c],                                                # 13: alone: its -0.0 survives
                       [-3 * c, -3 * c, -3 * c], [-2.5 * c, -2.5 * c, -2.5 * c]], np.float64).astype(F32)  # 14, 15: -k * cell opens cell -k


def big_bucket():
    rng = np.random.RandomState(11)
    bucket = (np.asarray([3, -4, 7], np.float64) + rng.uniform(0.1, 0.9, (3000, 3))).astype(F32)
    return np.concatenate([bucket[:1500], SINGLES[:2], bucket[1500:], SINGLES[2:]])


ORDER_CELL = 2.0
ORDER_ROWS = {"ascending": 0.5, "descending": 2.5, "shuffled": 4.5}  # the y of each copy: three cells


def order_series():
    """x values of one cluster, ascending, spanning 2^-52 .. 1: four of 2^-52, three of 1 and 1 + 2^-22.  Exactly, sum / 8 =
    0.5 + 2^-25 + 2^-53: just above the middle between the floats 0.5 and 0.5 + 2^-24.  Added in ascending order the float64
    sum is exact (the four small ones make 2^-50, which 4 + 2^-22 still holds) and the mean rounds UP; in descending order
    each 2^-52 is less than half an ulp of the running sum 4 + 2^-22 and is lost, the mean is the exact middle and rounds to
    even, DOWN."""
    return np.asarray([2.0 ** -52] * 4 + [1.0] * 3 + [1.0 + 2.0 ** -22], np.float64).astype(F32)


def add_order():
    x = order_series()
    rows = []
    for name, xs in (("ascending", x), ("descending", x[::-1]), ("shuffled", x[np.random.RandomState(4).permutation(len(x))])):
        r = np.full((len(x), 3), 0.5, F32)
        r[:, 0], r[:, 1] = xs, F32(ORDER_ROWS[name])
        rows.append(r)
    # more of the same kind: random values over 40 binades, in the three orders, in cells of their own
    rng = np.random.RandomState(5)
    for k in range(40):
        xs = (rng.uniform(1.0, 2.0, 48) * 2.0 ** rng.randint(-40, 0, 48)).astype(F32)
        for j, order in enumerate((np.argsort(xs), np.argsort(xs)[::-1], rng.permutation(48))):
            r = np.full((48, 3), 0.5, F32)
            r[:, 0], r[:, 1], r[:, 2] = xs[order], F32(10.5 + 2 * j), F32(10.5 + 2 * k)
            rows.append(r)
    return np.ascontiguousarray(np.concatenate(rows + [SINGLES]))


NAN_AT = (100, 101, 102)
NAN_BITS = (0x7fc12345, 0xff800001)  # a quiet NaN with a payload, a signalling one with the sign set


def nan_mesh():
    """300 vertices in 3 x 3 x 3 cells, three bad ones among them, and faces that name them."""
    rng = np.random.RandomState(6)
    base = rng.uniform(0.0, 3.0, (300, 3)).astype(F32)
    bad = np.zeros((3, 3), F32)
    bad[:] = base[7]
    bad.view(np.uint32)[0, 1] = NAN_BITS[0]
    bad.view(np.uint32)[1, 0] = NAN_BITS[1]
    bad[2, 2] = np.inf
    verts = np.concatenate([base[:100], bad, base[100:], SINGLES])
    faces = rng.randint(0, 303, (600, 3)).astype(np.uint32)
    extra = np.asarray([[100, 5, 9], [9, 100, 5],      # the same bad vertex and the same two clusters: a duplicate
                        [101, 101, 12],                # twice the same bad vertex: degenerate
                        [100, 101, 102],               # three bad vertices: three clusters: kept
                        [303, 304, 305]], np.uint32)   # the singles
    return np.ascontiguousarray(verts), np.concatenate([faces[:300], extra, faces[300:]])


SNAP_CELL = 0.03  # 3 lattice steps: of 20000 faces the model drops 35 as duplicates


def snapped_mesh():
    """The random cloud of tests/test_meshpost_gpu.py as small triangles with corners on a 1 cm lattice, shared between
    faces, and one large face of three far vertices (clusters of one)."""
    from tests.test_meshpost_gpu import indexed_random_mesh
    pool, faces = indexed_random_mesh(seed=7, n=20000)  # dense enough for faces to share their three cells
    n = len(pool)
    return np.concatenate([pool, SINGLES[:3]]), np.concatenate([faces, np.asarray([[n, n + 1, n + 2]], np.uint32)])


def opposite_faces():
    """Clusters A (0, 1), B (2, 3), C (4, 5), D (6): faces 0 and 1 name A, B, C in opposite orientation through different
    members; 2 is degenerate; 3 and 4 name A, B, D, rotated."""
    verts = np.asarray([[0.2, 0.2, 0.2], [0.7, 0.3, 0.4], [5.1, 0.2, 0.2], [5.8, 0.9, 0.1], [0.3, 5.5, 0.5], [0.6, 5.2, 0.9], [9.5, 9.5, 9.5]], F32)
    faces = np.asarray([[0, 2, 4], [5, 3, 1], [0, 1, 2], [6, 1, 3], [2, 6, 0]], np.uint32)
    return verts, faces


def colour_rounding():
    """Clusters of 2 and of 4 whose channel sums land on .5, on 0 and on 255; one single."""
    verts = np.asarray([[0.5, 0.5, 0.5]] * 2 + [[1.5, 0.5, 0.5]] * 4 + [[2.5, 0.5, 0.5]] * 2 + [[3.5, 0.5, 0.5]], F32)
    verts[:, 1] += (np.arange(len(verts)) * 0.01).astype(F32)
    rgb = np.asarray([[10, 0, 255], [11, 1, 254],                                # 10.5 -> 11, 0.5 -> 1, 254.5 -> 255
                      [1, 255, 0], [2, 255, 0], [2, 255, 0], [1, 255, 1],        # 6 / 4 = 1.5 -> 2, 255, 0.25 -> 0
                      [255, 0, 7], [255, 0, 8],                                  # 255, 0, 7.5 -> 8
                      [9, 8, 7]], np.uint8)
    return verts, rgb


def extent_edges():
    """Cell indices -2^20 and 2^20 - 1 are the outermost accepted (cell size 1)."""
    return np.asarray([[-1048576.0, 0.5, 0.5], [1048575.5, 0.5, 0.5], [0.5, 1048575.0, -1048575.5], [3.5, 3.5, 3.5], [3.25, 3.75, 3.5]], F32)


def extent_refused():
    """The same with one vertex at cell index 2^20."""
    v = extent_edges()
    v[3, 2] = 1048576.0
    return v


def cases():
    pool, faces = snapped_mesh()
    nan_v, nan_f = nan_mesh()
    opp_v, opp_f = opposite_faces()
    col_v, col_c = colour_rounding()
    soup = np.ascontiguousarray(pool[faces.astype(np.int64)].reshape(-1, 3))
    return {
        "random_cloud": (random_cloud(), None, colours(21, 4004), 1.0, False),
        "exact_duplicates": (exact_duplicates(), None, None, 1e-3, False),
        "cell_borders": (cell_borders(), None, colours(23, 16), BORDER_CELL, False),
        "big_bucket": (big_bucket(), None, colours(24, 3004), 1.0, False),
        "add_order": (add_order(), None, None, ORDER_CELL, False),
        "nan_mesh": (nan_v, nan_f, colours(26, len(nan_v)), 1.0, True),
        "snapped_indexed": (pool, faces, colours(27, len(pool)), SNAP_CELL, True),
        "snapped_soup": (soup, None, colours(28, len(soup)), SNAP_CELL, True),
        "opposite_faces": (opp_v, opp_f, None, 1.0, True),
        "colour_rounding": (col_v, None, col_c, 1.0, False),
        "extent_edges": (extent_edges(), None, None, 1.0, False),
    }


_MODELS = {}


def model(name):
    """The model of a named case, computed once per process and left unchanged."""
    if name not in _MODELS:
        verts, faces, rgb, cell, with_faces = cases()[name]
        _MODELS[name] = Dec(verts, faces, rgb, cell).check_mixed(with_faces)
    return _MODELS[name]
