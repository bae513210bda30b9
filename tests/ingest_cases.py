"""Helper of tests/test_oracle_ingest.py (CPU) and tests/test_ingest_gpu.py (GPU): the clouds that frame ingest
(tsdf_hip_organize, cpu_tsdf_amd/csrc/tsdf_ingest.hip = the `integrate` program's per-cloud loop) is held to, a plain
serial model of that loop, and the coverage floors of the clouds.  Pure numpy: no GPU, no library load.

  scene(W, H)             (W, H, fx, fy, cx, cy) of the program's default camera for that image size
  pixel_edges ... strides the case builders; each takes the scene and returns (xyz, bgra, kwargs):
                          xyz float32 (n, stride), bgra uint8 (n, cstride) or None, kwargs of OracleVolume.organize
  cases(s)                every case of every builder for one scene, as Case tuples
  model_organize(...)     the loop, point by point, in np.float32 scalars; with detail=True also what happened to every point
  edge_stats / check_edge_floors, one_pixel_stats / check_one_pixel_floors
                          the conditions the clouds must meet, counted from the model alone

The model is written from the program's description, not from oracle/tsdf_oracle.c: units, (0,0,0) -> NaN, the
world -> camera transform in double (x*c0 + (y*c1 + (z*c2 + c3)), rounded once, non-finite points untouched), the
all-float projection (x*fx/z)+cx, the conversion to int that truncates toward zero inside [-2^31, 2^31) and gives INT_MIN
outside and for NaN, and a z-buffer in which `old.z > new.z` replaces -- so the earliest of equal depths stays."""
import collections

import numpy as np

SIZES = [(160, 120), (7, 5), (65, 3), (1, 1), (257, 1)]
Z_EDGES = (0.5, 1.0, 0.37)
Z_ORDINARY = 0.28          # inside a 32^3 Scene-A volume seen from the turntable radius (0.2125 .. 0.3375)
INT_MIN = -2 ** 31
F32 = np.float32

Case = collections.namedtuple("Case", "name group xyz bgra kw color")


def scene(W, H):
    """src/prog/integrate.cpp:350-353 (cpu_tsdf_amd.synth.cli_intrinsics), restated so that nothing is imported here."""
    f = 525.0 * W / 640.0
    return W, H, f, f, W / 2.0 - 0.5, H / 2.0 - 0.5


# ---- the model ---------------------------------------------------------------------------------------------------------
def to_int(f):
    """float -> int as the program's compiler does it (cvttss2si)."""
    if f >= F32(-2147483648.0) and f < F32(2147483648.0):
        return int(f)   # truncates toward zero
    return INT_MIN      # out of range, and NaN (both comparisons false)


def model_organize(xyz, bgra, s, units=1.0, zero_nans=False, world_to_cam=None, detail=False):
    """(depth (H, W) float32 with NaN = empty, bgra (H, W, 4) uint8, filled) and, with `detail`, a dict of per-point
    arrays: fu, fv (float32), u, v (int64), ok (passed reprojectPoint), and per-pixel `winner` (point index or -1)."""
    W, H, fx, fy, cx, cy = s
    fx, fy, cx, cy = F32(fx), F32(fy), F32(cx), F32(cy)
    units = F32(units)
    zero = F32(0)
    nan = F32(np.nan)
    tf = None if world_to_cam is None else np.asarray(world_to_cam, np.float64)[:3, :4]
    n = len(xyz)
    depth = np.full((H, W), np.nan, np.float32)
    out_c = np.zeros((H, W, 4), np.uint8)
    out_c[..., 3] = 255
    winner = np.full((H, W), -1, np.int64)
    d_fu, d_fv = np.zeros(n, np.float32), np.zeros(n, np.float32)
    d_u, d_v, d_ok = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    filled = 0
    with np.errstate(all="ignore"):
        for j in range(n):
            x, y, z = F32(xyz[j, 0]), F32(xyz[j, 1]), F32(xyz[j, 2])
            if units != 1:
                x, y, z = x * units, y * units, z * units
            if zero_nans and x == zero and y == zero and z == zero:
                x = y = z = nan
            if tf is not None and np.isfinite(x) and np.isfinite(y) and np.isfinite(z):
                dx, dy, dz = np.float64(x), np.float64(y), np.float64(z)
                x, y, z = (F32(dx * r[0] + (dy * r[1] + (dz * r[2] + r[3]))) for r in tf)
            fu = (x * fx / z) + cx
            fv = (y * fy / z) + cy
            u, v = to_int(fu), to_int(fv)
            ok = (not np.isnan(z)) and z > zero and 0 <= u < W and 0 <= v < H
            d_fu[j], d_fv[j], d_u[j], d_v[j], d_ok[j] = fu, fv, u, v, ok
            if not ok:
                continue
            old = depth[v, u]
            if np.isnan(old) or old > z:
                if np.isnan(old):
                    filled += 1
                depth[v, u] = z
                winner[v, u] = j
                if bgra is not None:
                    out_c[v, u] = bgra[j, :4]
    if detail:
        return depth, out_c, filled, dict(fu=d_fu, fv=d_fv, u=d_u, v=d_v, ok=d_ok, winner=winner)
    return depth, out_c, filled


# ---- building blocks ---------------------------------------------------------------------------------------------------
def colours(n, cstride=4, salt=0):
    """n different b,g,r,a quadruples (an odd multiplier permutes the 32-bit words), padded to `cstride` bytes with junk."""
    words = ((np.arange(n, dtype=np.uint64) + 1 + salt) * 2654435761) % (1 << 32)
    out = np.empty((n, cstride), np.uint8)
    out[:, :4] = words.astype("<u4").view(np.uint8).reshape(n, 4)
    if cstride > 4:
        out[:, 4:] = np.random.RandomState(99 + salt).randint(0, 256, (n, cstride - 4))
    return out


def neighbours(a):
    """The float32 values of `a` and their three neighbours on either side: shape (7,) + a.shape."""
    a = np.asarray(a, np.float32)
    out, lo, hi = [a], a, a
    for _ in range(3):
        lo = np.nextafter(lo, F32(-np.inf))
        hi = np.nextafter(hi, F32(np.inf))
        out = [lo] + out + [hi]
    return np.stack(out)


def edge_coords(n_px, c, f, z):
    """For every pixel boundary k in [-2, n_px + 2]: float32((float32(k) - c) * z / f), all in float32."""
    k = np.arange(-2, n_px + 3).astype(np.float32)
    return (k - F32(c)) * F32(z) / F32(f)


def ordinary(s, n=40, z=Z_ORDINARY, seed=5, skip_centre=False):
    """Points in the middle of n pixels of the image (clear of every pixel boundary), depths around `z`."""
    W, H, fx, fy, cx, cy = s
    rng = np.random.RandomState(seed)
    u, v = rng.randint(0, W, n), rng.randint(0, H, n)
    if skip_centre:   # (leaves nothing on a 1 x 1 image)
        keep = ~((u == int(cx)) & (v == int(cy)))
        u, v = u[keep], v[keep]
    zz = z * rng.uniform(0.9, 1.1, u.size)
    return np.stack([(u + rng.uniform(0.3, 0.7, u.size) - cx) / fx * zz, (v + rng.uniform(0.3, 0.7, u.size) - cy) / fy * zz, zz], 1).astype(np.float32)


def pad(pts, stride=3, junk=np.nan):
    """(n, 3) -> (n, stride) float32; the floats between the points hold `junk` (never read by a correct loop)."""
    out = np.full((len(pts), stride), junk, np.float32)
    out[:, :3] = pts
    return out


# ---- the builders ------------------------------------------------------------------------------------------------------
def edge_points(s):
    """pixel_edges before shuffling: the u set (y = 0), the v set (x = 0), the diagonal set; and which set a point is of."""
    W, H, fx, fy, cx, cy = s
    pts, which = [], []
    for z in Z_EDGES:
        xs = neighbours(edge_coords(W, cx, fx, z)).reshape(-1)
        pts.append(np.stack([xs, np.zeros_like(xs), np.full_like(xs, z)], 1))
        which.append(np.zeros(xs.size, np.int8))
        ys = neighbours(edge_coords(H, cy, fy, z)).reshape(-1)
        pts.append(np.stack([np.zeros_like(ys), ys, np.full_like(ys, z)], 1))
        which.append(np.ones(ys.size, np.int8))
        # diagonal: column boundary i with row boundary i mod (H + 5); neighbour t in x goes with neighbour 3 t mod 7 in y
        xn, yn = neighbours(edge_coords(W, cx, fx, z)), neighbours(edge_coords(H, cy, fy, z))
        i = np.arange(xn.shape[1])
        t = np.arange(7)
        dx = xn[t][:, i].reshape(-1)
        dy = yn[(3 * t) % 7][:, i % yn.shape[1]].reshape(-1)
        pts.append(np.stack([dx, dy, np.full_like(dx, z)], 1))
        which.append(np.full(dx.size, 2, np.int8))
    return np.concatenate(pts).astype(np.float32), np.concatenate(which)


def pixel_edges(s, seed=1):
    pts, _ = edge_points(s)
    order = np.random.RandomState(seed).permutation(len(pts))   # the three depths interleave: winners and losers in any order
    return pad(pts[order]), colours(len(pts)), {}


def edge_sets(s, seed=1):
    """Which set (0 u, 1 v, 2 diagonal) every point of pixel_edges(s, seed) belongs to."""
    _, which = edge_points(s)
    return which[np.random.RandomState(seed).permutation(len(which))]


def int_limit_points(s):
    """Points whose fu (y = 0) or fv (x = 0) is 2^31, -2^31, or a float next to them: a huge coordinate, z = 1 (a depth
    of 1/2 or 1/4, which only doubles the products exactly, where no float32 coordinate reaches the limit itself at z = 1)."""
    W, H, fx, fy, cx, cy = s
    out = []
    with np.errstate(all="ignore"):
        for axis, (f, c) in enumerate(((fx, cx), (fy, cy))):
            for lim in (2147483648.0, -2147483648.0):
                best = None
                for z in (1.0, 0.5, 0.25):
                    cand = neighbours(F32(lim * z / f))
                    for _ in range(2):   # +- 9 floats around the quotient
                        cand = np.unique(neighbours(cand))
                    fuv = (cand * F32(f) / F32(z)) + F32(c)
                    best = best or (z, cand)
                    if (fuv == F32(lim)).any():
                        best = (z, cand)
                        break
                z, cand = best
                p = np.zeros((cand.size, 3), np.float32)
                p[:, axis], p[:, 2] = cand, z
                out.append(p)
    return np.concatenate(out)


def extreme_points(s, denormal=True):
    """denormal=False leaves out the three finite points on the optical axis: (0, 0, 1e-45), (0, 0, 1e-39), (0, 0, 3e38)."""
    axis = ([(0, 0, 1e-45), (0, 0, 1e-39)], [(0, 0, 3e38)]) if denormal else ([], [])
    pts = axis[0] + [(1e-45, 0, 1e-45), (0, 0, np.inf), (1, 1, np.inf), (np.inf, 0, np.inf), (3e38, 0, 1)] + axis[1] + [
        (0, 0, -0.0), (-0.0, -0.0, 0.0), (0, 0, -1.0), (0.01, 0.01, -0.5), (np.nan, 0, 1), (0, np.nan, 1), (0, 0, np.nan)]
    with np.errstate(all="ignore"):
        return np.concatenate([np.array(pts, np.float64).astype(np.float32), int_limit_points(s)])


def extremes(s, denormal=True):
    """The list, then the list again with ordinary points in between.  Every z = +inf point and every finite (0, 0, z)
    project to (cx, cy), so the pixel there holds a denormal depth with denormal=True and +inf without; no ordinary
    point is put on that pixel."""
    ext = extreme_points(s, denormal)
    o = ordinary(s, n=len(ext), skip_centre=True)
    mixed = np.zeros((len(ext) + len(o), 3), np.float32)
    pos = np.sort(np.random.RandomState(3).choice(len(mixed), len(o), replace=False))
    mask = np.zeros(len(mixed), bool)
    mask[pos] = True
    mixed[mask], mixed[~mask] = o, ext
    pts = np.concatenate([ext, mixed])
    return pad(pts), colours(len(pts), salt=1000), {}


UNITS = (("1e-30", 1e-30, False), ("1e30", 1e30, False), ("-1", -1.0, False), ("0_zero_nans", 0.0, True), ("0", 0.0, False))


def units(s, cloud, variant):
    """`cloud` ("extremes" / "pixel_edges") under cloud_units of UNITS[variant].  For -1 every second point is negated
    first, so that half the cloud moves from behind the camera to the front and half the other way."""
    name, scale, zn = UNITS[variant]
    xyz, bgra, _ = extremes(s) if cloud == "extremes" else pixel_edges(s)
    if scale == -1.0:
        xyz = xyz.copy()
        xyz[::2, :3] = -xyz[::2, :3]
    return xyz, bgra, dict(units=scale, zero_nans=zn)


def _turn180():
    return np.diag([-1.0, 1.0, -1.0, 1.0])


def _scale1e20():
    m = np.diag([1e20, 1e20, 1e20, 1.0])
    m[2, 3] = 3e18   # (pulls every point a tenth of the way toward the optical axis)
    return m


def _nan_entry():
    m = np.eye(4)
    m[0, 1] = np.nan   # x of every finite point becomes NaN
    return m


def _inf_entry():
    m = np.eye(4)
    m[2, 3] = np.inf   # z of every finite point becomes +inf: the whole cloud lands on (cx, cy), all depths equal
    return m


TRANSFORMS = (("turn180", _turn180), ("scale1e20", _scale1e20), ("nan_entry", _nan_entry), ("inf_entry", _inf_entry))


def transforms(s, variant):
    """world_to_cam of TRANSFORMS[variant] on ordinary points mixed with the non-finite ones of `extremes` (and its
    zeros, negatives and overflowing products; no finite point on the optical axis).  The non-finite points are left as
    they are, so (0, 0, +inf) lands on (cx, cy) under every matrix; the 180-degree turn and the NaN entry fill no other
    pixel, and the inf entry puts every finite point on that pixel too, at the same depth."""
    xyz, bgra, _ = extremes(s, denormal=False)
    return xyz, bgra, dict(world_to_cam=TRANSFORMS[variant][1]())


ONE_PIXEL_N = 20000


def one_pixel_depths():
    a, b = F32(0.25), F32(0.27)
    return np.array([a, np.nextafter(a, F32(1)), 0.26, b, np.nextafter(b, F32(1)), 0.3, 0.31, 0.35], np.float32)   # [0] = the minimum


def one_pixel(s, seed=11):
    """ONE_PIXEL_N points on the centre pixel (where z = +inf lands too) and as many over the four pixels left and right
    of it, depths from eight values (two pairs 1 ulp apart); the minimum is drawn from index 300 on only, so its first
    occurrence -- the winner -- lies in a later block of 256 than the first loser."""
    W, H, fx, fy, cx, cy = s
    rng = np.random.RandomState(seed)
    n = ONE_PIXEL_N
    zs = one_pixel_depths()
    pick = rng.randint(0, 8, 2 * n)
    pick[:300] = rng.randint(1, 8, 300)
    z = zs[pick].astype(np.float64)
    u = np.full(2 * n, int(cx))
    u[1::2] += rng.choice([-2, -1, 1, 2], n)   # outside a 1-pixel-wide image: dropped there
    v = int(cy)
    pts = np.stack([(u + rng.uniform(0.2, 0.8, 2 * n) - cx) / fx * z, (v + rng.uniform(0.2, 0.8, 2 * n) - cy) / fy * z, z], 1).astype(np.float32)
    pts[:, 2] = zs[pick]   # (exactly the eight values)
    pts = np.concatenate([pts[:1000], np.array([[0, 0, np.inf]], np.float32), pts[1000:]])
    return pad(pts), colours(len(pts), salt=5000), {}


SIZES_N = (1, 63, 64, 65, 255, 256, 257, 4097)


def sizes(s, n):
    xyz, bgra, kw = pixel_edges(s)
    return xyz[:n], bgra[:n], kw


STRIDES = (("xyz3_c4", 3, 4), ("xyz4_c7", 4, 7), ("xyz5_c32", 5, 32), ("xyz8_c4", 8, 4), ("xyz8_none", 8, None), ("xyz3_c4_plain_volume", 3, 4))


def strides(s, variant):
    """Point and colour strides; no colours at all on a colour volume (every pixel (0,0,0,255)); colours handed to a
    volume without colour (variant 5: Case.color is False)."""
    _, xs, cs = STRIDES[variant]
    pe, _, _ = pixel_edges(s)
    pts = np.concatenate([pe[:1500, :3], ordinary(s, 60, seed=8)])
    pts = pts[np.random.RandomState(21).permutation(len(pts))]
    return pad(pts, xs, junk=1e30 if xs == 4 else np.nan), (colours(len(pts), cs, salt=9000) if cs else None), {}


def cases(s):
    """Every case for scene `s`, in a fixed order."""
    out = [Case("pixel_edges", "pixel_edges", *pixel_edges(s), True),
           Case("extremes", "extremes", *extremes(s, True), True),
           Case("extremes_no_denormal", "extremes", *extremes(s, False), True)]
    for cloud in ("extremes", "pixel_edges"):
        for i, (name, _, _) in enumerate(UNITS):
            out.append(Case(f"units_{name}_{cloud}", "units", *units(s, cloud, i), True))
    for i, (name, _) in enumerate(TRANSFORMS):
        out.append(Case(f"transform_{name}", "transforms", *transforms(s, i), True))
    out.append(Case("one_pixel", "one_pixel", *one_pixel(s), True))
    for n in SIZES_N:
        out.append(Case(f"n{n}", "sizes", *sizes(s, n), True))
    for i, (name, _, _) in enumerate(STRIDES):
        out.append(Case(f"stride_{name}", "strides", *strides(s, i), "plain_volume" not in name))
    return out


GROUPS = ("pixel_edges", "extremes", "units", "transforms", "one_pixel", "sizes", "strides")


def feeds_integrate(depth, max_sensor_dist):
    """The cases whose frame is also integrated by the GPU test: those with at least one pixel inside the volume's view,
    that is with a finite depth in front of the camera and no farther than the sensor's range."""
    with np.errstate(invalid="ignore"):
        return bool((np.isfinite(depth) & (depth > 0) & (depth <= max_sensor_dist)).any())


# ---- coverage floors ---------------------------------------------------------------------------------------------------
# Conditions, not measurements: what a case must contain to be worth running.  Per axis of pixel_edges: points whose fu / fv
# is an exact integer, points with fu / fv in (-1, 0) that are KEPT (in column / row 0: the conversion truncates toward
# zero), points with fu == W / fv == H exactly (dropped).  The 1 x 1 image has 6 boundaries per axis where the others have
# dozens: its exact-integer floor is what the builder gives there (162 per axis: every second point of the three sets).
FLOOR_EXACT, FLOOR_NEG, FLOOR_AT_END = 50, 10, 3
FLOOR_EXACT_1X1 = 162
FLOOR_TIES, FLOOR_WINNER = 500, 256


def edge_stats(s, det):
    """Per axis counts of the pixel_edges cloud from the model's per-point record."""
    W, H = s[0], s[1]
    st = {}
    with np.errstate(invalid="ignore"):
        for ax, f, n_px in (("u", det["fu"], W), ("v", det["fv"], H)):
            fin = np.isfinite(f)
            st[f"exact_{ax}"] = int((fin & (f == np.trunc(f))).sum())
            coord = det["u"] if ax == "u" else det["v"]
            st[f"neg_kept_{ax}"] = int((det["ok"] & (f > -1) & (f < 0) & (coord == 0)).sum())
            st[f"at_end_{ax}"] = int(((f == F32(n_px)) & ~det["ok"]).sum())
    return st


def check_edge_floors(s, st):
    W, H = s[0], s[1]
    exact = FLOOR_EXACT_1X1 if (W, H) == (1, 1) else FLOOR_EXACT
    assert st["exact_u"] >= exact and st["exact_v"] >= exact, st
    assert st["neg_kept_u"] >= FLOOR_NEG and st["neg_kept_v"] >= FLOOR_NEG, st
    assert st["at_end_u"] >= FLOOR_AT_END and st["at_end_v"] >= FLOOR_AT_END, st


def one_pixel_stats(s, xyz, depth, det):
    cx, cy = int(s[4]), int(s[5])
    w = int(det["winner"][cy, cx])
    here = det["ok"] & (det["u"] == cx) & (det["v"] == cy)
    z = xyz[:, 2]
    return dict(winner=w, ties=int((here & (z == depth[cy, cx])).sum()), on_pixel=int(here.sum()), first_on_pixel=int(np.argmax(here)),
                inf_on_pixel=int((here & np.isinf(z)).sum()), ulp_pairs=int((np.diff(np.unique(z[here & np.isfinite(z)]).view(np.int32)) == 1).sum()))


def check_one_pixel_floors(st):
    assert st["winner"] >= FLOOR_WINNER and st["ties"] >= FLOOR_TIES, st
    assert st["first_on_pixel"] < 256 <= st["winner"], st   # the first loser and the winner in different blocks of 256
    assert st["on_pixel"] >= ONE_PIXEL_N and st["inf_on_pixel"] == 1 and st["ulp_pairs"] == 2, st


def is_denormal(a):
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore"):
        return (a != 0) & (np.abs(a) < np.finfo(np.float32).tiny)
