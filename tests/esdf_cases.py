"""Shared by the computeDistanceField tests: a numpy restatement of what tsdf_hip_esdf is declared to compute
(include/tsdf_hip.h) -- the site rule, the exact squared Euclidean distance transform as three separable passes in int64, the
float field -- and the volumes the GPU tests upload.  No GPU, no SciPy.  Arrays are [z][y][x] as download() returns them;
a box is (x0, y0, z0, nx, ny, nz) as the C ABI takes it."""
import numpy as np

FAR = 0xFFFFFFFF
_INF = np.int64(1) << 40  # above every squared distance of a grid the library accepts


def whole(res3):
    nx, ny, nz = (int(v) for v in res3)
    return (0, 0, 0, nx, ny, nz)


def voxel_edge(p):
    """The fp32 voxel edge getFxn uses: size[0] / res[0], one float32 division."""
    return np.float32(p.size[0]) / np.float32(p.res[0])


# ---- the model --------------------------------------------------------------------------------------------------------------
def classes(d, w, min_weight):
    """0 not valid, 1 valid and not negative, 2 valid and negative."""
    with np.errstate(invalid="ignore"):
        valid = (w > np.float32(min_weight)) & ~np.isnan(d)
        return np.where(valid, np.where(d < 0, 2, 1), 0).astype(np.int8)


def sites(p, d, w, box, min_weight):
    """(site, neg), each of the box's shape (nz, ny, nx): v in the box is a site iff valid(v) and some 6-neighbour u inside
    the GRID (p.res; u may lie outside the box) has valid(u) and neg(u) != neg(v).  d, w: the whole grid."""
    x0, y0, z0, nx, ny, nz = (int(v) for v in box)
    rx, ry, rz = (int(v) for v in p.res)
    assert d.shape == (rz, ry, rx) and w.shape == d.shape
    assert 0 <= x0 and 0 <= y0 and 0 <= z0 and nx > 0 and ny > 0 and nz > 0 and x0 + nx <= rx and y0 + ny <= ry and z0 + nz <= rz
    # the box and one voxel around it, clipped to the grid; what lies beyond the grid is class 0 (no neighbour there)
    lo = (max(z0 - 1, 0), max(y0 - 1, 0), max(x0 - 1, 0))
    hi = (min(z0 + nz + 1, rz), min(y0 + ny + 1, ry), min(x0 + nx + 1, rx))
    c = np.zeros((nz + 2, ny + 2, nx + 2), np.int8)
    sub = classes(d[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], w[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], min_weight)
    o = (lo[0] - (z0 - 1), lo[1] - (y0 - 1), lo[2] - (x0 - 1))
    c[o[0]:o[0] + sub.shape[0], o[1]:o[1] + sub.shape[1], o[2]:o[2] + sub.shape[2]] = sub
    me = c[1:-1, 1:-1, 1:-1]
    site = np.zeros(me.shape, bool)
    for axis in range(3):
        for s in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[axis] = slice(s, s + me.shape[axis])
            u = c[tuple(sl)]
            site |= (me != 0) & (u != 0) & (u != me)
    return site, me == 2


def _pass(f, axis):
    """g[j] = min_i f[i] + (i - j)^2 along `axis`, int64."""
    f = np.moveaxis(f, axis, -1)
    n = f.shape[-1]
    j = np.arange(n, dtype=np.int64)
    g = np.full(f.shape, _INF, np.int64)
    for i in range(n):
        np.minimum(g, f[..., i:i + 1] + (i - j) ** 2, out=g)
    return np.moveaxis(g, -1, axis)


def edt2(site_mask, r_max=0):
    """uint32 (nz, ny, nx): the squared distance to the nearest True voxel; FAR where there is none, and above r_max^2 when
    r_max > 0.  Three separable exact passes, x then y then z."""
    g = np.where(site_mask, np.int64(0), _INF)
    for axis in (2, 1, 0):
        g = np.minimum(_pass(g, axis), _INF)
    far = g >= _INF
    if r_max > 0:
        far |= g > int(r_max) ** 2
    return np.where(far, FAR, g).astype(np.uint32)


def dist(d2, neg, voxel):
    """float32: sgn * voxel * sqrt((float)d2), FAR -> sgn * inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        m = np.sqrt(d2.astype(np.float32)) * np.float32(voxel)
    m = np.where(d2 == FAR, np.float32(np.inf), m).astype(np.float32)
    return np.where(neg, -m, m).astype(np.float32)


def model(p, d, w, box=None, r_max=0, min_weight=0.0):
    """(d2, dist, number of sites) of the box."""
    box = whole(p.res) if box is None else box
    site, neg = sites(p, d, w, box, min_weight)
    d2 = edt2(site, r_max)
    return d2, dist(d2, neg, voxel_edge(p)), int(site.sum())


def brute_force(site_mask):
    """The same as edt2(site_mask, 0), literally: over all pairs of voxels."""
    pts = np.argwhere(np.ones(site_mask.shape, bool)).astype(np.int64)
    s = np.argwhere(site_mask).astype(np.int64)
    if not len(s):
        return np.full(site_mask.shape, FAR, np.uint32)
    out = np.empty(len(pts), np.int64)
    for k, v in enumerate(pts):
        out[k] = ((s - v) ** 2).sum(axis=1).min()
    return out.reshape(site_mask.shape).astype(np.uint32)


# ---- volumes ----------------------------------------------------------------------------------------------------------------
def random_volume(rng, res3, wmax=3):
    """d random in [-1, 1] with some NaN, +0.0, -0.0 and exact +-1; w random in {0, 1, 2, wmax}: sites are dense, with many
    ties between them."""
    nx, ny, nz = res3
    shape = (nz, ny, nx)
    d = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    pick = rng.rand(*shape)
    d[pick < 0.03] = np.nan
    d[(pick >= 0.03) & (pick < 0.06)] = 0.0
    d[(pick >= 0.06) & (pick < 0.09)] = -0.0
    d[(pick >= 0.09) & (pick < 0.12)] = 1.0
    d[(pick >= 0.12) & (pick < 0.15)] = -1.0
    w = np.array([0, 1, 2, wmax], np.float32)[rng.randint(0, 4, shape)]
    return d, w


def sparse(res3, singles, block=None):
    """All valid (w = 1) and positive (d = 0.5), except single negative voxels at `singles` ((x, y, z) each) and one small
    negative block (x0, y0, z0, edge): few sites, long distances, far parabolas."""
    nx, ny, nz = res3
    d = np.full((nz, ny, nx), 0.5, np.float32)
    w = np.ones((nz, ny, nx), np.float32)
    for x, y, z in singles:
        d[z, y, x] = -0.25
    if block is not None:
        x, y, z, e = block
        d[z:z + e, y:y + e, x:x + e] = -0.75
    return d, w


def empty(res3):
    """The reset state: d = -1, w = 0."""
    nx, ny, nz = res3
    return np.full((nz, ny, nx), -1.0, np.float32), np.zeros((nz, ny, nx), np.float32)
