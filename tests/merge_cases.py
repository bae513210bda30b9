"""Shared by the mergeVolume tests: a numpy restatement of what tsdf_hip_merge is declared to compute (include/tsdf_hip.h),
float32 step by step, built from pieces other tests already pin to the reference -- the ORACLE's centre tables, getFxn
(OracleVolume.sample) and getContainingVoxel (oracle_containing), not the product's -- plus the volumes and geometries of
tests/test_merge_gpu.py.  Arrays are [z][y][x] as download() returns them."""
import ctypes as C

import numpy as np

from oracle import oracle
from oracle.oracle import OracleVolume
from tests.align_cases import se3_exp, transform_f32


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def rigid(axis, angle, translation=(0.0, 0.0, 0.0)):
    """4 x 4: a turn by `angle` about `axis` (normalised here), then `translation`."""
    a = np.asarray(axis, np.float64)
    T = se3_exp(np.concatenate([a / np.linalg.norm(a) * angle, [0.0, 0.0, 0.0]])) if angle else np.eye(4)
    T[:3, 3] = translation
    return T


QUARTER_X = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])

# (name, src res, src size, dst res, dst size, dst_from_src, merged voxels a CPU model gave when the feature was specified:
# the tests assert at least half of it, so that none can pass on an empty merge; this model gives 675, 676, 241, 10768.
# The identity case depends on src's weights alone and is reproduced exactly; the other three also depend on which voxels the
# 3 % random zeros hit relative to the transformed centres, i.e. on the order and shapes of random_volume's draws (d, w, zeros,
# rgb; src before dst), which the specification does not fix -- the counts agree within 8 %, as different draws of it would.
# The fused-data cases of tests/test_merge_gpu.py, which have no random input, reproduce their quoted figures digit for digit.)
GEOMETRIES = [
    ("identity", 16, 1.0, 16, 1.0, np.eye(4), 675),
    ("turn_0.4", 16, 1.0, 16, 1.0, rigid((1, 2, 3), 0.4, (0.07, -0.05, 0.03)), 712),
    ("24_into_16", 24, 1.0, 16, 1.5, rigid((0, 1, 0.2), 1.1, (0.3, 0.1, -0.2)), 245),
    ("quarter_into_32", 16, 1.0, 32, 0.8, QUARTER_X, 11629),
]
FAR = rigid((1, 0, 0), 0.0, (2.0, 0.0, 0.0))  # a translation by 2 m: nothing of a 1 m src reaches a 1 m dst


def src_from_dst(dst_from_src):
    """The 12 doubles the C ABI takes: the first three rows of the inverse."""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(dst_from_src, np.float64))[:3, :4])


def random_volume(rng, res3, size, color, wmax=3, p_max=0.0, ball=True):
    """d uniform in [-1.2, 1.2]; integer weights 1..wmax inside a ball of radius 0.42 * size around the grid's centre, zero
    outside, plus 3 % random zeros (fully random weights pass the eight-neighbour gate in about 10 % of places).  p_max:
    that share of the weights is raised to wmax (a gate at min_weight just below wmax then still opens somewhere).
    ball=False: observed up to the faces of the grid, for cases about the edge of src."""
    nx, ny, nz = res3
    shape = (nz, ny, nx)
    d = rng.uniform(-1.2, 1.2, shape).astype(np.float32)
    w = rng.randint(1, int(wmax) + 1, shape).astype(np.float32)
    if p_max:
        w[rng.rand(*shape) < p_max] = wmax
    c = [(np.arange(n) + 0.5) * size / n - size / 2 for n in (nz, ny, nx)]
    r2 = c[0][:, None, None] ** 2 + c[1][None, :, None] ** 2 + c[2][None, None, :] ** 2
    if ball:
        w[r2 > (0.42 * size) ** 2] = 0
    w[rng.rand(*shape) < 0.03] = 0
    rgb = rng.randint(0, 256, shape + (3,)).astype(np.uint8) if color else None
    return d, w, rgb


# ---- the model --------------------------------------------------------------------------------------------------------------
def dst_centres(p_dst):
    """(n, 3) float32: the centre of every dst voxel, [z][y][x] order, from the oracle's centre tables."""
    tab = [_centres(p_dst, a) for a in range(3)]
    nx, ny, nz = p_dst.res
    c = np.empty((nz, ny, nx, 3), np.float32)
    c[..., 0] = tab[0][None, None, :]
    c[..., 1] = tab[1][None, :, None]
    c[..., 2] = tab[2][:, None, None]
    return c.reshape(-1, 3)


def _centres(p, axis):
    """OracleVolume.centers without the voxel arrays: the octree's node centres, or the closed form (node_size's rule)."""
    r = p.res[0]
    cubic_pow2 = r > 0 and (r & (r - 1)) == 0 and p.res[1] == r and p.res[2] == r
    out = np.empty(p.res[axis], np.float32)
    oracle.lib().oracle_centers(p.res[axis], p.size[0] if cubic_pow2 else p.size[axis], out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def lower_corner(p, q):
    """getNeighbors' lower corner (tsdf_volume_octree.cpp:796-828) restated from getVoxelIndex / getVoxelCenter (:553-574):
    ok = the voxel of q and its seven upper neighbours exist; idx (n, 3) = x, y, z of the lower corner."""
    n = len(q)
    idx = np.empty((n, 3), np.int64)
    ok = np.ones(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            size, res = np.float64(np.float32(p.size[a])), np.float64(p.res[a])
            f = np.floor((q[:, a].astype(np.float64) + size / 2.0) / size * res)
            i = np.where(np.isfinite(f) & (np.abs(f) < 2.0 ** 31), f, -2.0 ** 31).astype(np.int64)
            ok &= (i >= 0) & (i < p.res[a])
            off = np.float32(size / 2.0)
            ctr = ((np.clip(i, 0, None).astype(np.float64) + 0.5) * size / res - np.float64(off)).astype(np.float32)
            idx[:, a] = i - (q[:, a] < ctr)
    for a in range(3):
        ok &= (idx[:, a] >= 0) & (idx[:, a] < p.res[a] - 1)
    return ok, idx


def containing(ov, q, where):
    """Octree::getContainingVoxel for the points q[where]: found (n,) bool, idx (n, 3) x, y, z."""
    found = np.zeros(len(q), bool)
    idx = np.zeros((len(q), 3), np.int64)
    L, out = oracle.lib(), (C.c_int * 3)()
    for t in np.flatnonzero(where):
        if L.oracle_containing(C.byref(ov.p), float(q[t, 0]), float(q[t, 1]), float(q[t, 2]), out):
            found[t] = True
            idx[t] = out[0], out[1], out[2]
    return found, idx


def merge_model(p_dst, dst, p_src, src, dst_from_src, min_weight=0.0):
    """The declared result of tsdf_hip_merge(dst, src, rows of dst_from_src^-1, min_weight).  dst, src = (d, w, rgb or
    None).  Returns d, w, rgb (None without a dst colour plane) and the merged mask, all [z][y][x]."""
    d0, w0, rgb0 = dst
    ds, ws_, rgbs = (np.ascontiguousarray(src[0], np.float32), np.ascontiguousarray(src[1], np.float32), src[2])
    shape = d0.shape
    q = transform_f32(src_from_dst(dst_from_src), dst_centres(p_dst))                   # steps 1, 2
    ov = OracleVolume(p_src, adopt=(ds, ws_, rgbs))
    ok, val, _, _ = ov.sample(q)                                                        # step 3
    ok_r, idx = lower_corner(p_src, q)
    assert np.array_equal(ok, ok_r), "the restated lower corner disagrees with the oracle's getFxn"
    gate = ok & (val == val)                                                            # step 4
    i = np.where(ok[:, None], idx, 0)
    mw = np.float32(min_weight)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                gate &= ws_[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx] > mw
    found, ci = containing(ov, q, gate)                                                 # step 5
    off = ci - i
    assert np.all((off[found] >= 0) & (off[found] <= 1)), "the containing voxel is not one of the eight neighbours"
    m = gate & found
    w_s = ws_[ci[:, 2], ci[:, 1], ci[:, 0]][m]
    d, w = d0.reshape(-1).copy(), w0.reshape(-1).copy()
    rgb = rgb0.reshape(-1, 3).copy() if rgb0 is not None else None
    w_old = w[m]
    wsum = w_old + w_s                                                                  # step 6, every operation in float32
    assert w_s.dtype == np.float32 and wsum.dtype == np.float32 and np.all(wsum > 0)
    if rgb is not None and rgbs is not None:
        c_s = rgbs[ci[:, 2], ci[:, 1], ci[:, 0]][m].astype(np.float32)
        c_old = rgb[m].astype(np.float32)
        qv = (w_old[:, None] * c_old + w_s[:, None] * c_s) / wsum[:, None]
        assert qv.dtype == np.float32
        rgb[m] = (qv.astype(np.int32) & 255).astype(np.uint8)
    d[m] = (d[m] * w_old + val[m] * w_s) / wsum
    wmax = np.float32(p_dst.max_weight)
    w[m] = np.where(wsum > wmax, wmax, wsum)
    return d.reshape(shape), w.reshape(shape), (rgb.reshape(shape + (3,)) if rgb is not None else None), m.reshape(shape)
