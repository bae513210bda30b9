"""Helper of the API-sequence tests (tests/test_api_sequences_gpu.py, tests/test_evidence_gpu.py): a plain model of what a
volume must hold and answer after ANY sequence of calls.  The model is an OracleVolume plus numpy, never the product:

  integrate   OracleVolume.integrate;
  shift       tests/shift_cases.shifted_volume applied in place to the oracle's arrays; frames integrated later are posed
              through the translations shiftVolume returned (Translation(-moved) * trans);
  uploads     the same array writes;
  readers     OracleVolume.march / raycast / sample on the model's arrays, the occupied restatement of
              tests/test_occupied_gpu.py, the cleanup oracle of tests/test_meshpost_gpu.py, the flatten oracle of
              tests/flatten_cases.py and the fp64 alignment system of tests/align_cases.py.

Record restates the host's bookkeeping of the implied distances (tsdf_hip_volume::band_exact / rest_state)."""
import numpy as np

from cpu_tsdf_amd import synth
from oracle.oracle import OracleVolume
from tests import shift_cases
from tests.common import assert_same_f32


class Record:
    """The host's record of what the planes may hold (tsdf_hip_volume::band_exact / rest_state), restated."""

    def __init__(self, packed, fixed, kmax):
        self.can = bool(packed and fixed and kmax >= 1)
        self.reset()

    def reset(self):
        self.flags_describe_planes, self.rest = True, 0

    def foreign_write(self):  # upload, set_planes_device on owned planes, device_planes, load, a plain-kernel launch
        self.flags_describe_planes = False

    def shift(self):
        """tsdf_hip_shift moves the flags with the voxels: what the record says of the planes holds of the moved planes."""

    def fast_launch(self):
        """A flag-keeping launch (k_integrate / k_integrate2): returns whether it may rebuild distances from counts."""
        if not self.flags_describe_planes:
            return False
        if not self.can:
            self.rest = 2
        elif self.rest == 0:
            self.rest = 1
        return self.rest == 1


def hinge_is_fixed(trunc, wmax):
    """The hinge identity of DESIGN.md 3.1c: the running mean of the free-space value p stays p for every count."""
    p = np.float32(trunc[0]) / np.float32(trunc[1])
    kmax = int(np.ceil(wmax))
    return wmax == np.floor(wmax) and all(np.float32(np.float32(p * np.float32(min(k, wmax))) + p) / np.float32(min(k, wmax) + 1) == p
                                          for k in range(kmax + 1))


def record_for(packed, trunc, wmax):
    return Record(packed, hinge_is_fixed(trunc, wmax), int(np.ceil(wmax)))


def compare(vol, ov, what):
    d, w, rgb = vol.download()
    assert_same_f32(d, ov.d, f"d {what}")
    assert_same_f32(w, ov.w, f"w {what}")
    if ov.rgb is not None:
        assert np.array_equal(rgb, ov.rgb), f"rgb {what}"
    return d, w, rgb


def clamp_shift(s, res):
    """tsdf_hip_shift clamps every component to [-res, res] (the result is the same: everything is reset)."""
    return tuple(int(max(-r, min(r, v))) for v, r in zip(s, res))


def slab_starts(res, n=3):
    """First plane of every slab of tsdf_hip_create_multi's partition of `res` planes over n devices, and res."""
    base, extra = res // n, res % n
    return [k * base + min(k, extra) for k in range(n + 1)]


def draw_shift(rng, cum, thick):
    """A random shift of the sequence tests: pure and mixed, +-1 / +-3 / a whole flag cell / one more along x, past a row
    cell along y, past a whole slab along z; `cum` (the sum so far) keeps the window near the scene."""
    t = thick + 1
    s = [int(rng.choice([0, 0, 1, -1, 3, -3, 64, -64, 65, -65])), int(rng.choice([0, 0, 1, -1, 4, -4, 5, -5])),
         int(rng.choice([0, 0, 1, -1, 2, -2, t, -t]))]
    for a, limit in enumerate((65, 5, t)):   # the window stays near the scene: a shift that would leave turns back
        if abs(cum[a] + s[a]) > limit:
            s[a] = -s[a]
    return tuple(s)


class Model:
    """An OracleVolume that follows shifts, uploads and resets.  `moved` is the sum of what shiftVolume returned, `G` the
    global transform the product's class keeps (reset() keeps it, like the class)."""

    def __init__(self, params, mode=None, cull=False):
        """mode: None (TSDF_COLOR_RGB, no weighting: OracleVolume.integrate) or one of tests/evidence/
        fuzz_product_colour_modes.MODES -- the oracle form that integrates, and the per-voxel state that goes with it
        (ov.cn of the colour modes, ov.M / ov.nsample of the variance weighting).  cull: every frame is integrated with the
        reference's frustum cull for the pose the product is handed (the product applies it on every frame; it only
        decides voxels under narrow off-centre cameras)."""
        if mode is not None:
            from tests.evidence.fuzz_product_colour_modes import MODES
            assert mode in MODES, mode
        self.params, self.mode, self.cull = params, mode, bool(cull)
        self.reset()
        self.color = self.ov.rgb is not None
        self.moved = np.zeros(3)
        self.G = np.eye(4)

    # ---- writers -------------------------------------------------------------------------------------------------------
    def reset(self):
        """A fresh volume that keeps its mode (and with it the state planes, zero like tsdf_hip_reset leaves them)."""
        self.ov = ov = OracleVolume(self.params)
        planes = {"RGBNormalized": 4, "LAB": 3}.get(self.mode, 0)
        if planes:
            ov.cn = np.zeros((planes,) + ov.d.shape, np.float32)
        if self.mode and "by_variance" in self.mode:
            ov.M, ov.nsample = np.zeros_like(ov.d), np.zeros(ov.d.shape, np.int32)

    def state_arrays(self):
        """The per-voxel state beyond d, w, rgb as (name, [z][y][x] array) pairs."""
        ov = self.ov
        out = [(f"cn[{k}]", ov.cn[k]) for k in range(len(ov.cn))] if hasattr(ov, "cn") else []
        if getattr(ov, "M", None) is not None:
            out += [("M", ov.M), ("nsample", ov.nsample)]
        return out

    def pose(self, trans):
        """The pose to hand to the product for a camera that stands at `trans` in the frame the volume started in."""
        t = np.eye(4)
        t[:3, 3] = -self.moved
        return t @ np.asarray(trans, np.float64)

    def integrate(self, depth, bgra, trans):
        """`trans`: the pose as handed to the product (Model.pose applied by the caller)."""
        ov, col, T = self.ov, bgra if self.color else None, synth.cam_from_vol_f32(trans)
        planes = ov.reference_cull_planes(trans) if self.cull else None
        if self.mode is None:
            return ov.integrate(depth, col, T, planes=planes) if self.cull else ov.integrate(depth, col, T)
        if self.mode == "RGBNormalized":
            return ov.integrate_rgbn(depth, col, T, planes=planes)
        if self.mode == "LAB":
            return ov.integrate_lab(depth, col, T, planes=planes)
        if "by_variance" in self.mode:
            return ov.integrate_variance(depth, col, T, "by_depth" in self.mode, planes=planes)
        return ov.integrate(depth, col, T, weight_by_depth=True, planes=planes)

    def shift(self, s, moved):
        """s: the voxels asked for; moved: what shiftVolume returned for them."""
        ov = self.ov
        res = tuple(ov.p.res)
        d, w, rgb = shift_cases.shifted_volume(ov.d, ov.w, ov.rgb, clamp_shift(s, res))
        ov.d[...], ov.w[...] = d, w
        if rgb is not None:
            ov.rgb[...] = rgb
        for _, a in self.state_arrays():
            a[...] = shift_cases.shifted(a, clamp_shift(s, res), shift_cases.FILL_STATE)
        self.moved = self.moved + np.asarray(moved, np.float64)
        t = np.eye(4)
        t[:3, 3] = np.asarray(moved, np.float64)
        self.G = self.G @ t

    def box(self, x0, y0, z0, nx, ny, nz):
        sl = (slice(z0, z0 + nz), slice(y0, y0 + ny), slice(x0, x0 + nx))
        return self.ov.d[sl], self.ov.w[sl], (self.ov.rgb[sl] if self.color else None)

    def upload(self, d=None, w=None, rgb=None, x0=0, y0=0, z0=0):
        ref = d if d is not None else (w if w is not None else rgb)
        nz, ny, nx = ref.shape[:3]
        bd, bw, brgb = self.box(x0, y0, z0, nx, ny, nz)
        if d is not None:
            bd[...] = d
        if w is not None:
            bw[...] = w
        if rgb is not None:
            brgb[...] = rgb

    def variance_box(self, box):
        """(M, nsample) views of box = (x0, y0, z0, nx, ny, nz)."""
        x0, y0, z0, nx, ny, nz = box
        sl = (slice(z0, z0 + nz), slice(y0, y0 + ny), slice(x0, x0 + nx))
        return self.ov.M[sl], self.ov.nsample[sl]

    def upload_variance(self, M, ns, box):
        """tsdf_hip_upload_variance_state: either array may be None."""
        bM, bns = self.variance_box(box)
        if M is not None:
            bM[...] = M
        if ns is not None:
            bns[...] = ns

    # ---- readers -------------------------------------------------------------------------------------------------------
    def to_world(self, verts):
        """reconstruct() hands vertices out after the global transform (pcl::transformPointCloud, evaluated in double)."""
        if np.array_equal(self.G, np.eye(4)):
            return verts
        p, m = verts.astype(np.float64), self.G
        out = np.empty_like(p)
        for r in range(3):
            out[..., r] = p[..., 0] * m[r, 0] + (p[..., 1] * m[r, 1] + (p[..., 2] * m[r, 2] + m[r, 3]))
        return out.astype(np.float32)

    def mesh(self, w_min, cleanup=None, flatten=None):
        """What MarchingCubesTSDFOctree.reconstruct(want_cells=True) returns: the soup, or with `flatten` the indexed mesh;
        cleanup = (face_dist, min_neighbors) runs first, both in the volume frame."""
        mode = 1 if self.color else 0
        verts, rgb, cells = self.ov.march(w_min, mode)
        rgb = rgb if mode else None
        if cleanup is not None:
            verts, rgb, cells = cleaned_soup(verts, rgb, cells, *cleanup)
        if flatten is None:
            n = len(cells)
            return {"vertices": self.to_world(verts), "polygons": np.arange(3 * n, dtype=np.int32).reshape(n, 3), "rgb": rgb, "cells": cells}
        from tests.flatten_cases import Flat
        f = Flat(verts, None, flatten)
        seeds = f.seeds.astype(np.int64)
        return {"vertices": self.to_world(f.vertices), "polygons": f.polygons, "rgb": rgb[seeds] if rgb is not None else None,
                "cells": cells[f.keep]}

    def occupied(self, box=None):
        from tests.test_occupied_gpu import expected
        if box is None:
            return expected(self.ov.d, self.ov.w, self.ov.rgb)
        d, w, rgb = self.box(*box)
        return expected(d, w, rgb, origin=tuple(box[:3]))

    def raycast(self, trans, ds):
        return self.ov.raycast(trans, ds)

    def sample(self, pts):
        return self.ov.sample(pts)

    def alignment(self, vol, pts, T, min_weight, r_max):
        """tests/align_cases.restate on the model's voxels (vol: the product object, for its parameters and mirror only)."""
        from tests import align_cases
        return align_cases.restate(vol, self.ov, self.ov.w, pts, T, min_weight, r_max)


def cleaned_soup(verts, rgb, cells, face_dist, min_neighbors):
    """tsdf_hip_march_cleanup on a soup (3 vertices per cell key; rgb may be None): the cleanup oracle of
    tests/test_meshpost_gpu.py decides which faces stay."""
    if not len(cells):
        return verts, rgb, cells
    from tests.test_meshpost_gpu import centroids, oracle_groups
    label, sizes = oracle_groups(centroids(verts), face_dist)
    keep = sizes[label] > min_neighbors
    k3 = np.repeat(keep, 3)
    return verts[k3], (rgb[k3] if rgb is not None else None), cells[keep]


def assert_same_mesh(got, want, what):
    assert np.array_equal(got["cells"], want["cells"]), f"{what}: cells ({len(got['cells'])} against {len(want['cells'])})"
    assert_same_f32(got["vertices"], want["vertices"], f"{what}: vertices")
    assert np.array_equal(got["polygons"], want["polygons"]), f"{what}: polygons"
    if want["rgb"] is not None:
        assert np.array_equal(got["rgb"], want["rgb"]), f"{what}: rgb"
