"""Shared by tests/test_oracle_lattice.py and tests/test_lattice_gpu.py: volumes whose voxels sit ON the comparisons the
readers decide by -- exact zeros of either sign, denormals, +-1 and its neighbours below, NaN and +-Inf, weights at and
around the thresholds -- instead of the smooth or uniform-random content of every other test.

Builders return (d, w, rgb) as [z][y][x] arrays for a grid res3 = (nx, ny, nz); they are deterministic.  tally() computes,
from the oracle alone, the quantities whose floors (FLOORS) keep a comparison from passing on nothing.  Nothing here needs
a GPU, and nothing is loaded through ctypes before a function is called."""
import numpy as np

F32 = np.float32
ONE_DOWN = np.nextafter(F32(1), F32(0))
TINY, TINIEST = F32(1e-40), F32(1e-45)   # a denormal that survives * 0.03 and the smallest one, which does not
FINITE = np.array([-1, -0.5, -0.25, -TINY, -0.0, 0.0, TINY, -TINIEST, TINIEST, 0.25, 0.5, 1, ONE_DOWN, -ONE_DOWN], F32)
NONFINITE = np.array([np.nan, np.inf, -np.inf], F32)
VALUES = np.concatenate([FINITE, NONFINITE])
QUIET_NANS = ((0x7fc00001, (3, 5, 7)), (0xffc00000, (11, 2, 9)))   # (bits, (x, y, z)): planted for the storage tests only
MAX_WEIGHT = 100.0
W_PACKED = np.array([0, 1, 2, 3, 99, 100], F32)
W_F32W = np.concatenate([W_PACKED, np.array([0.5, np.nextafter(F32(2), F32(0)), np.nextafter(F32(2), F32(3))], F32)])
SEED = 5
FAMILIES = ("random_nonfinite", "random_finite", "zero_sheet", "zero_sheet_tilted", "denormal_shell", "denormal_shell_neg1")
# per family the truncation limits (max_dist_pos, max_dist_neg) of the volume that holds it
TRUNC = {name: (0.03, 0.03) for name in FAMILIES}
TRUNC["denormal_shell_neg1"] = (0.03, 1.0)
W_MINS = ((0.0, 2), (2.0, 1), (2.5, 0))   # (w_min, colour mode; mode 1 falls back to 0 on a volume without colour)


def _shape(res3):
    return (res3[2], res3[1], res3[0])


def weights(res3, seed, f32w=False):
    """Half the voxels at 100; of the rest most at 2, 3 and 99, a few below 2: nineteen corners in twenty pass w_min 2.0,
    four in five pass 2.5, so that cells with eight passing corners stay common at either threshold."""
    rng = np.random.RandomState(1000 + seed)
    if f32w:   # 0, 1, 2, 3, 99, 100, 0.5, nextafter(2, 0), nextafter(2, 3)
        pool, prob = W_F32W, [0.02, 0.02, 0.07, 0.13, 0.15, 0.5, 0.02, 0.02, 0.07]
    else:
        pool, prob = W_PACKED, [0.025, 0.025, 0.15, 0.15, 0.15, 0.5]
    return pool[rng.choice(len(pool), size=_shape(res3), p=prob)].astype(F32)


def colours(res3, seed):
    return np.random.RandomState(2000 + seed).randint(0, 256, _shape(res3) + (3,)).astype(np.uint8)


def random(res3, seed, nonfinite):
    """Every voxel an independent draw from VALUES: the twelve values inside (-1, 1) share 90 %, +-1 the rest -- with
    `nonfinite` all but 2 % of it, which NaN and +-Inf take together.  (A cell is meshed only if none of its eight corners
    is at or beyond +-1: a uniform draw would leave a quarter of the cells.)"""
    rng = np.random.RandomState(seed)
    inner = np.abs(FINITE) < 1
    prob = np.where(inner, 0.90 / inner.sum(), (0.08 if nonfinite else 0.10) / (~inner).sum())
    pool = FINITE
    if nonfinite:
        pool, prob = VALUES, np.concatenate([prob, np.full(len(NONFINITE), 0.02 / len(NONFINITE))])
    return pool[rng.choice(len(pool), size=_shape(res3), p=prob)].astype(F32)


def zero_sheet(res3, tilted=False):
    """d = clip(0.25 * (z - k), -1, 1): a whole plane of exact zeros; tilted: one voxel per 4 in x, so the zeros lie on
    lines along y, four voxels apart -- single corners of the cells in between."""
    nx, ny, nz = res3
    z, _, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = 0.25 * (z - nz // 2)
    if tilted:
        d = d + 0.0625 * (x - nx // 2)
    return np.clip(d, -1, 1).astype(F32)


def shell_sign(res3):
    """-1 inside a sphere of radius 0.3 grid edges around the grid's centre, +1 outside ([z][y][x], float32)."""
    nx, ny, nz = res3
    z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n - 0.5 for n in (nz, ny, nx)], indexing="ij")
    return np.where(x * x + y * y + z * z < 0.3 * 0.3, F32(-1), F32(1)).astype(F32)


def denormal_shell(res3, seed):
    """The sphere with -1e-40 or -1e-45 inside (drawn per voxel) and + the same outside."""
    rng = np.random.RandomState(3000 + seed)
    mag = np.where(rng.rand(*_shape(res3)) < 0.5, TINY, TINIEST).astype(F32)
    return (shell_sign(res3) * mag).astype(F32)


def normal_shell(res3):
    """The same shell with normal-range values: what a reader that lost the denormals' signs must NOT agree with."""
    return (shell_sign(res3) * F32(0.5)).astype(F32)


def build(family, res3, color=True, f32w=False, seed=SEED):
    """(d, w, rgb or None) of a named family."""
    if family.startswith("random"):
        d = random(res3, seed, family == "random_nonfinite")
    elif family.startswith("zero_sheet"):
        d = zero_sheet(res3, family.endswith("tilted"))
    elif family.startswith("denormal_shell"):
        d = denormal_shell(res3, seed)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(d), weights(res3, seed, f32w), (colours(res3, seed) if color else None)


def with_quiet_nans(d):
    """A copy with the two quiet NaNs of QUIET_NANS planted (payload and sign are what storage has to keep)."""
    d = d.copy()
    u = d.view(np.uint32)
    for bits, (x, y, z) in QUIET_NANS:
        u[z, y, x] = bits
    return d


def params(res3, size, family, color, width=80, height=60):
    """capi.TsdfParams of the volume tests/common.make_volume(32, 80, 60, ...) configures for this family."""
    from cpu_tsdf_amd import capi, synth
    p = capi.default_params()
    p.res[:] = res3
    p.size[:] = (size,) * 3
    p.fx, p.fy, p.cx, p.cy = synth.cli_intrinsics(width, height)
    p.image_width, p.image_height = width, height
    p.min_sensor_dist, p.max_sensor_dist = 0.0, 3 * size
    p.max_dist_pos, p.max_dist_neg = TRUNC[family]
    p.max_weight = MAX_WEIGHT
    p.integrate_color = int(color)
    return p


def model_of(p, family, f32w=False, seed=SEED):
    """A tests.sequence_model.Model that holds the family, and the arrays that went in."""
    from tests.sequence_model import Model
    m = Model(p)
    d, w, rgb = build(family, tuple(p.res), bool(p.integrate_color), f32w, seed)
    m.upload(d, w, rgb)
    return m, (d, w, rgb)


def assert_same_bits(a, b, what):
    """Equality of the uint32 views of two float32 arrays: the sign of zero and a NaN's payload count."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ne = a.view(np.uint32) != b.view(np.uint32)
    if ne.any():
        idx = np.argwhere(ne)[:5]
        raise AssertionError(f"{what}: {int(ne.sum())} of {a.size} words differ; first {idx.tolist()} got "
                             f"{[hex(v) for v in a.view(np.uint32)[ne][:5]]} want {[hex(v) for v in b.view(np.uint32)[ne][:5]]}")


# ---- poses and points -------------------------------------------------------------------------------------------------------
def poses(size):
    """Two cameras outside the grid, one inside looking across it, one inside looking along -z straight at the sheet."""
    from cpu_tsdf_amd import synth
    S = size
    return [synth.look_at_pose((0.9 * S, -0.5 * S, -1.9 * S)), synth.look_at_pose((-1.6 * S, 0.4 * S, 1.5 * S), target=(0.05 * S, 0.0, -0.05 * S)),
            synth.look_at_pose((0.1 * S, -0.05 * S, -0.45 * S)), synth.look_at_pose((0.0, 0.0, 0.45 * S))]


FRONT = 2   # the pose "from the front": inside the grid, so that a ray starts with a voxel's step also at max_dist_neg = 1


def sample_points(ov, n_random=2400, seed=SEED):
    """Random points over (and a little beyond) the grid, then points whose coordinates are voxel centres (all three, or one
    of them) and points on the faces between voxels, where getVoxelIndex's floor changes."""
    rng = np.random.RandomState(4000 + seed)
    res, size = tuple(ov.p.res), [float(s) for s in ov.p.size]
    half = np.array(size) / 2
    pts = [rng.uniform(-1.05, 1.05, (n_random, 3)) * half]
    ctr = [ov.centers(a).astype(np.float64) for a in range(3)]
    n = 400
    on_ctr = np.stack([ctr[a][rng.randint(res[a], size=n)] for a in range(3)], 1)
    pts.append(on_ctr)
    one = rng.uniform(-1.0, 1.0, (n, 3)) * half                      # one coordinate on a centre
    axis = rng.randint(3, size=n)
    one[np.arange(n), axis] = on_ctr[np.arange(n), axis]
    pts.append(one)
    face = rng.uniform(-1.0, 1.0, (n, 3)) * half                     # one coordinate on a face between two voxels
    for a in range(3):
        sel = axis == a
        face[sel, a] = rng.randint(res[a] + 1, size=int(sel.sum())) * (size[a] / res[a]) - half[a]
    pts.append(face)
    faces3 = np.stack([rng.randint(res[a] + 1, size=n) * (size[a] / res[a]) - half[a] for a in range(3)], 1)
    pts.append(faces3)
    return np.ascontiguousarray(np.concatenate(pts).astype(F32))


def align_points(family, size, n=1500, seed=SEED):
    """Points around the sheet or the shell (anywhere in the grid for the random families), in the volume frame."""
    rng = np.random.RandomState(5000 + seed)
    S = size
    if family.startswith("zero_sheet"):
        p = rng.uniform(-0.45, 0.45, (n, 3)) * S
        p[:, 2] = rng.normal(0.0, 0.03, n) * S
    elif family.startswith("denormal_shell"):
        v = rng.normal(size=(n, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.3 + rng.normal(0.0, 0.02, (n, 1))) * S
    else:
        p = rng.uniform(-0.48, 0.48, (n, 3)) * S
    return np.ascontiguousarray(p.astype(F32))


# ---- the conditions ---------------------------------------------------------------------------------------------------------
CLEANUP_VOXELS, CLEANUP_MIN_NEIGHBORS, POST_W_MIN = 1.1, 12, 2.5
FLOORS = {"triangles_w0": 10000, "triangles_w2": 10000, "triangles_w2.5": 2000, "share_two_equal_vertices": 0.05, "flatten_dropped": 0.05,
          "cleanup_dropped": 0.05, "cleanup_kept": 0.05, "occupied_listed": 0.30, "occupied_left_out": 0.05, "hits_per_pose": 300,
          "nan_t_rays": 100, "sample_ok": (0.30, 0.90), "sample_nan_ok": 50}


def cleanup_setting(model):
    return (CLEANUP_VOXELS * float(model.ov.p.size[0]) / int(model.ov.p.res[0]), CLEANUP_MIN_NEIGHBORS)


def two_equal_vertices(verts):
    t = np.ascontiguousarray(verts, F32).view(np.uint32).reshape(-1, 3, 3)
    return ((t[:, 0] == t[:, 1]).all(1) | (t[:, 1] == t[:, 2]).all(1) | (t[:, 2] == t[:, 0]).all(1))


def tally(model, post=True):
    """The quantities of FLOORS for the volume a Model holds, from the oracle alone."""
    from tests import flatten_cases
    ov = model.ov
    out = {}
    for w_min, key in ((0.0, "triangles_w0"), (2.0, "triangles_w2"), (2.5, "triangles_w2.5")):
        verts, _, cells = ov.march(w_min, 0)
        out[key] = len(cells)
        if w_min == 0.0:
            out["share_two_equal_vertices"] = float(two_equal_vertices(verts).mean()) if len(cells) else 0.0
    if post:
        soup = model.mesh(POST_W_MIN)
        n = max(len(soup["cells"]), 1)
        out["flatten_dropped"] = 1.0 - len(model.mesh(POST_W_MIN, None, flatten_cases.MD)["cells"]) / n
        kept = len(model.mesh(POST_W_MIN, cleanup_setting(model))["cells"]) / n
        out["cleanup_dropped"], out["cleanup_kept"] = 1.0 - kept, kept
    listed = len(model.occupied()[0]) / ov.d.size
    out["occupied_listed"], out["occupied_left_out"] = listed, 1.0 - listed
    hits, nan_t = [], 0
    for tr in poses(float(ov.p.size[0])):
        view = ov.raycast(tr, 1)
        hits.append(int(np.isfinite(view[..., 0]).sum()))
        nan_t += int(np.isnan(view[..., 6]).sum())
    out["hits_per_pose"], out["nan_t_rays"] = hits, nan_t
    ok, val, _, _ = ov.sample(sample_points(ov))
    out["sample_ok"], out["sample_nan_ok"] = float(ok.mean()), int(np.isnan(val[ok]).sum())
    return out


def check_floors(t):
    """The random family's floors (tests/test_oracle_lattice.py asserts them on the CPU; the GPU tests before any product call)."""
    for key, floor in FLOORS.items():
        if key not in t:
            continue
        v = t[key]
        if key == "hits_per_pose":
            assert min(v) >= floor, (key, v)
        elif isinstance(floor, tuple):
            assert floor[0] <= v <= floor[1], (key, v)
        else:
            assert v >= floor, (key, v)
