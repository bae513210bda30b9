"""Shared by the castRays tests: the reference for ONE arbitrary ray (the oracle's renderView on a 1 x 1 image), pixel
directions in ray_direction's operation order, the admission rule of include/tsdf_hip.h in float64, the table of rays the
admission tests run, and the two ray families of tests/test_castrays_gpu.py."""
import numpy as np

from oracle.oracle import OracleVolume

CAP_MAX = 2 ** 24


class OneRayOracle:
    """The reference's 8 floats for the ray (o, u) over [tmin, tmax]: OracleVolume.raycast with image_width = image_height = 1
    and cx = cy = 0 -- the centre pixel's direction is (0, 0, 1) exactly, so a `trans` whose rotation block has zero first
    and second columns and third column u rotates it into u itself --, translation o, min / max_sensor_dist = tmin / tmax."""

    def __init__(self, params, d, w, rgb=None):
        self.ov = OracleVolume(params, adopt=(d, w, rgb))
        p = self.ov.p
        p.image_width = p.image_height = 1
        p.cx = p.cy = 0.0
        self.zmin, self.zmax = float(p.min_sensor_dist), float(p.max_sensor_dist)

    def ray(self, o, u, tmin=None, tmax=None):
        p = self.ov.p
        p.min_sensor_dist = self.zmin if tmin is None else float(tmin)
        p.max_sensor_dist = self.zmax if tmax is None else float(tmax)
        T = np.zeros((4, 4))
        T[:3, 2] = np.asarray(u, np.float32)
        T[:3, 3] = np.asarray(o, np.float32)
        T[3, 3] = 1.0
        return self.ov.raycast(T, 1).reshape(8).copy()

    def rays(self, org, dirs, t_range=None):
        out = np.empty((len(org), 8), np.float32)
        for i in range(len(org)):
            out[i] = self.ray(org[i], dirs[i], *(t_range[i] if t_range is not None else (None, None)))
        return out


def pixel_directions(p, trans, ds=1):
    """du of every pixel of renderView(trans, ds), (H/ds * W/ds, 3) float32, in ray_direction's operation order
    (tsdf_volume_octree.cpp:316-319): the pixel in double, cast to float, Eigen's normalize, R * du as p0 + (p1 + p2)."""
    trans = np.asarray(trans, np.float64)
    rot = trans[:3, :3].astype(np.float32)
    nw, nh = p.image_width // ds, p.image_height // ds
    x = np.tile(np.arange(nw, dtype=np.float64), nh)
    y = np.repeat(np.arange(nh, dtype=np.float64), nw)
    a = ((x - p.cx / ds) / (p.fx / ds)).astype(np.float32)
    b = ((y - p.cy / ds) / (p.fy / ds)).astype(np.float32)
    c = np.ones_like(a)
    n = np.sqrt(a * a + (b * b + c * c))
    a, b, c = a / n, b / n, c / n
    return np.stack([rot[k, 0] * a + (rot[k, 1] * b + rot[k, 2] * c) for k in range(3)], axis=1).astype(np.float32)


def admit_rule(o, u, tmin, tmax, leaf):
    """(admitted, cap) by the rule of include/tsdf_hip.h, in float64."""
    vals = np.array(list(o) + list(u) + [tmin, tmax], np.float32).astype(np.float64)
    if not np.isfinite(vals).all():
        return False, 0
    rng = np.float64(np.float32(tmax)) - np.float64(np.float32(tmin))
    quarter = np.float64(np.float32(leaf)) / 4.0
    trips = np.ceil(rng / quarter) if rng > 0 else 0.0
    cap = 16.0 + 2.0 * trips
    if not cap <= CAP_MAX:
        return False, 0
    return True, int(cap)


def bound_range(leaf):
    """The range at which cap = 2^24 exactly: (2^24 - 16) / 2 quarter-leaves."""
    return (CAP_MAX - 16) / 2 * (np.float64(np.float32(leaf)) / 4.0)


def admit_table():
    """(o, u, tmin, tmax, leaf) rows: NaN and +-inf in each of the 8 inputs, tmax = inf (covered by those), ranges just
    below and just above the 2^24 bound for the leaf sizes 1/256 and 3.3/64, tmax < tmin, tmax == tmin, and a far ray whose
    t makes no float progress."""
    rows = []
    base = ([0.01, -0.02, -0.4], [0.0, 0.0, 1.0], 0.0, 0.75)
    for leaf in (1.0 / 256, 3.3 / 64):
        for slot in range(8):
            for bad in (np.nan, np.inf, -np.inf):
                o, u, tmin, tmax = list(base[0]), list(base[1]), base[2], base[3]
                if slot < 3:
                    o[slot] = bad
                elif slot < 6:
                    u[slot - 3] = bad
                elif slot == 6:
                    tmin = bad
                else:
                    tmax = bad
                rows.append((o, u, tmin, tmax, leaf))
        r = bound_range(leaf)
        for f in (1 - 1e-3, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-3, 4.0):
            rows.append((base[0], base[1], 0.0, float(np.float32(r * f)), leaf))
            rows.append((base[0], base[1], 0.5, float(np.float32(0.5 + r * f)), leaf))
        rows.append((base[0], base[1], 0.5, 0.25, leaf))
        rows.append((base[0], base[1], 0.5, 0.5, leaf))
        rows.append((base[0], base[1], 0.0, 0.75, leaf))
        rows.append((base[0], base[1], 1e6, 1e6 + 1, leaf))
        rows.append((base[0], base[1], -3.0e38, 3.0e38, leaf))
    return rows


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def family_outside_in(rng, size, n):
    """n rays from a sphere of radius `size` toward points uniform in +-0.2 size."""
    org = (unit(rng.normal(size=(n, 3))).astype(np.float64) * size).astype(np.float32)
    tgt = rng.uniform(-0.2, 0.2, (n, 3)) * size
    return org, unit(tgt - org)


def family_inside_out(rng, size, n):
    """n rays from origins uniform in +-0.45 size with uniform directions."""
    org = (rng.uniform(-0.45, 0.45, (n, 3)) * size).astype(np.float32)
    return org, unit(rng.normal(size=(n, 3)))
