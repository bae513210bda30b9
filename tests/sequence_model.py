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


class Model:
    """An OracleVolume that follows shifts, uploads and resets.  `moved` is the sum of what shiftVolume returned, `G` the
    global transform the product's class keeps (reset() keeps it, like the class)."""

    def __init__(self, params):
        self.params = params
        self.ov = OracleVolume(params)
        self.color = self.ov.rgb is not None
        self.moved = np.zeros(3)
        self.G = np.eye(4)

    # ---- writers -------------------------------------------------------------------------------------------------------
    def reset(self):
        self.ov = OracleVolume(self.params)

    def pose(self, trans):
        """The pose to hand to the product for a camera that stands at `trans` in the frame the volume started in."""
        t = np.eye(4)
        t[:3, 3] = -self.moved
        return t @ np.asarray(trans, np.float64)

    def integrate(self, depth, bgra, trans):
        """`trans`: the pose as handed to the product (Model.pose applied by the caller)."""
        return self.ov.integrate(depth, bgra if self.color else None, synth.cam_from_vol_f32(trans))

    def shift(self, s, moved):
        """s: the voxels asked for; moved: what shiftVolume returned for them."""
        ov = self.ov
        res = tuple(ov.p.res)
        d, w, rgb = shift_cases.shifted_volume(ov.d, ov.w, ov.rgb, clamp_shift(s, res))
        ov.d[...], ov.w[...] = d, w
        if rgb is not None:
            ov.rgb[...] = rgb
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
        if cleanup is not None and len(cells):
            from tests.test_meshpost_gpu import centroids, oracle_groups
            label, sizes = oracle_groups(centroids(verts), cleanup[0])
            keep = sizes[label] > cleanup[1]
            k3 = np.repeat(keep, 3)
            verts, cells = verts[k3], cells[keep]
            rgb = rgb[k3] if rgb is not None else None
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


def assert_same_mesh(got, want, what):
    assert np.array_equal(got["cells"], want["cells"]), f"{what}: cells ({len(got['cells'])} against {len(want['cells'])})"
    assert_same_f32(got["vertices"], want["vertices"], f"{what}: vertices")
    assert np.array_equal(got["polygons"], want["polygons"]), f"{what}: polygons"
    if want["rgb"] is not None:
        assert np.array_equal(got["rgb"], want["rgb"]), f"{what}: rgb"
