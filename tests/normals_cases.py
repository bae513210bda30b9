"""The cases of the meshNormals tests and a numpy model of the rule (include/tsdf_hip.h, tsdf_hip_mesh_normals), written
without looking at cpu_tsdf::mesh_post::normalArrays: the face vectors are float64 element operations (numpy rounds each
once and fuses nothing), the vertex sums are an explicit loop over the faces in index order and over their corners, one add
at a time, and the normalisation is float64 element operations again.  tests/test_normals_oracle.py pins the host pass to
this model on the CPU tier; tests/test_normals_gpu.py the GPU pass."""
import functools
from fractions import Fraction

import numpy as np

from tests import smooth_cases as sc

F32 = np.float32
U32 = np.uint32
NO_FACES = np.empty((0, 3), U32)


def _fma(a, b, c):
    """a * b + c rounded once (float(Fraction) rounds correctly)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


class Model:
    """The rule on (verts n x 3 float32, faces k x 3, or None for a soup: face f = vertices 3f, 3f + 1, 3f + 2).  The two
    switches are NOT the rule -- they exist only to show that a case can tell implementations apart: descending adds the
    faces of a vertex in DESCENDING face index; contracted computes a * b - c * d as fma(a, b, -(c * d)), what a compiler
    that contracts would emit."""

    def __init__(self, verts, faces, descending=False, contracted=False):
        verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        n = len(verts)
        if faces is None:
            assert n % 3 == 0
            f = np.arange(n, dtype=np.int64).reshape(-1, 3)
        else:
            f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
        assert not len(f) or (0 <= int(f.min()) and int(f.max()) < n)
        p = verts.astype(np.float64)
        pa, pb, pc = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        self.skipped_faces = ~(np.isfinite(pa).all(1) & np.isfinite(pb).all(1) & np.isfinite(pc).all(1))
        with np.errstate(all="ignore"):
            e1, e2 = pb - pa, pc - pa
            if contracted:
                g = np.zeros((len(f), 3))
                for i in range(len(f)):
                    for k, (u, v) in enumerate(((1, 2), (2, 0), (0, 1))):
                        g[i, k] = _fma(e1[i, u], e2[i, v], -(e1[i, v] * e2[i, u])) if not self.skipped_faces[i] else 0.0
            else:
                g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                              e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                              e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        g[self.skipped_faces] = 0.0
        self.face_vectors = g
        s = [[0.0, 0.0, 0.0] for _ in range(n)]  # +0.0
        named = np.zeros(n, bool)
        near_skipped = np.zeros(n, bool)
        self.valence = np.zeros(n, np.int64)  # entries of each vertex's run: corners that name it
        order = range(len(f) - 1, -1, -1) if descending else range(len(f))
        fl, gl, sk = f.tolist(), g.tolist(), self.skipped_faces.tolist()
        for i in order:
            for v in fl[i]:
                named[v] = True
                self.valence[v] += 1
                if sk[i]:
                    near_skipped[v] = True
                    continue
                acc, add = s[v], gl[i]
                acc[0] += add[0]
                acc[1] += add[1]
                acc[2] += add[2]
        s = np.asarray(s, np.float64).reshape(n, 3)
        self.sums = s
        l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        zero = l2 == 0.0
        with np.errstate(all="ignore"):
            unit = (s / np.sqrt(l2)[:, None]).astype(F32)
        self.normals = np.where(zero[:, None], F32(0.0), unit).astype(F32)
        self.flags = ((~named) * 1 + zero * 2 + near_skipped * 4).astype(np.uint8)
        self.n_skipped = int(self.skipped_faces.sum())
        self.n_zero = int(zero.sum())

    @property
    def stats(self):
        """the first three words of tsdf_hip_mesh_normals_stats"""
        return [len(self.normals), self.n_skipped, self.n_zero]


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def opposite():
    """the same triangle in both windings, twice over: every sum is g + (-g) = +0.0 exactly"""
    v = np.asarray([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.7, 0.6]], F32)
    return v, np.asarray([[0, 1, 2], [0, 2, 1]], U32)


def coincident(k=40, seed=21):
    """k faces (a, b, c) whose corners b and c are DIFFERENT vertices at ONE position; coordinates of mixed magnitude, 1e-6 ..
    1e6 per component, so that the products e1y * e2z are inexact"""
    rng = np.random.default_rng(seed)
    a = 10.0 ** rng.uniform(-6, 6, (k, 3)) * rng.choice([-1.0, 1.0], (k, 3))
    b = 10.0 ** rng.uniform(-6, 6, (k, 3)) * rng.choice([-1.0, 1.0], (k, 3))
    v = np.stack([a, b, b], 1).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * k, dtype=U32).reshape(-1, 3)


def add_order():
    """vertex 0 is named by four faces of one plane whose z-components are, in ascending face index, 1, 1, 2^60 and -2^60:
    ascending, ((1 + 1) + 2^60) - 2^60 = 0 (the 2 is below the double's last bit at 2^60); descending, ((-2^60 + 2^60) + 1) + 1
    = 2"""
    big = 2.0 ** 30
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [big, 0, 0], [0, big, 0]], F32)
    return v, np.asarray([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 4]], U32)


def non_finite():
    """smooth_cases.non_finite: a strip of 24 whose vertex 5 has a NaN, 15 an infinite component and 6 a -0.0 (which is
    finite).  The faces 3, 4, 5 (all of vertex 5's) and 13, 14, 15 are skipped."""
    return sc.non_finite()


def random_soup(k=257, seed=31):
    """a soup of k triangles; face 100 is degenerate (two corners at one position), face 200 has a NaN"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (3 * k, 3)).astype(F32)
    v[3 * 100 + 2] = v[3 * 100 + 1]
    v[3 * 200 + 1, 0] = np.nan
    return v, None


def icosphere5():
    v, f = sc.icosphere(5)
    return (v * 0.7 + 0.25).astype(F32), f


SPHERE_RES = 32


def sphere_field(params):
    """The orientation tests' volume, for the parameters of a SPHERE_RES^3 volume: w = 1 everywhere and
    d = clip((|x - c| - 10.3 voxels) / (3 voxels), -1, 1) at the voxel centres x (negative inside), c = the centre voxel's
    centre + (0.13, 0.27, -0.31) voxels.  -> (d, w as [z][y][x] float32, c in the volume's coordinates)"""
    from oracle.oracle import OracleVolume
    ov = OracleVolume(params)
    res = list(params.res)
    assert res == [SPHERE_RES] * 3
    voxel = float(params.size[0]) / res[0]
    x, y, z = (ov.centers(a).astype(np.float64) for a in range(3))
    c = np.asarray([x[res[0] // 2], y[res[1] // 2], z[res[2] // 2]]) + np.asarray([0.13, 0.27, -0.31]) * voxel
    r = np.sqrt((z[:, None, None] - c[2]) ** 2 + (y[None, :, None] - c[1]) ** 2 + (x[None, None, :] - c[0]) ** 2)
    d = np.clip((r - 10.3 * voxel) / (3 * voxel), -1.0, 1.0).astype(F32)
    return np.ascontiguousarray(d), np.ones_like(d), c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (verts, faces or None for a soup)"""
    out = {}
    out["tetrahedron"] = sc.tetrahedron()
    out["grid_5x5"] = sc.grid_patch()
    out["fan_300"] = sc.fan(300, 1)
    out["double_fan_300"] = sc.fan(300, 2)
    for n in (255, 256, 257, 258, 259):  # 255 / 256 / 257 vertices, and 255 / 256 / 257 faces (a strip of n has n - 2)
        out[f"strip_{n}"] = sc.strip(n)
    out["unreferenced"] = sc.unreferenced()
    out["odd_faces"] = sc.odd_faces()
    out["opposite"] = opposite()
    out["coincident"] = coincident()
    out["add_order"] = add_order()
    out["non_finite"] = non_finite()
    out["random"] = sc.random_mesh()
    out["random_soup_257"] = random_soup()
    out["no_faces"] = (sc.strip(7)[0], NO_FACES)
    out["soup_no_faces"] = (sc.strip(6)[0], None, 0)  # a soup handed over with n_faces == 0: no vertex is named
    out["icosphere_5"] = icosphere5()
    return out


def arrays(name):
    """(verts, faces or None, n_faces as the entry points take it)"""
    c = cases()[name]
    v, f = c[0], c[1]
    nf = c[2] if len(c) == 3 else (len(v) // 3 if f is None else len(f))
    return v, f, nf


@functools.lru_cache(maxsize=None)
def model(name):
    v, f, nf = arrays(name)
    if f is None and nf == 0:
        return Model(v, NO_FACES)
    return Model(v, f)
