"""Helper of tests/test_feature_sequences_gpu.py and of its CPU replay in tests/test_sequence_model.py: what the feature
sequences expect, composed from the models the per-feature tests already pin bit for bit -- nothing here needs a GPU and
nothing is restated:

  remove    tests/deintegrate_cases.RemovalModel / remove_frame;
  merge     tests/merge_cases.merge_model on the two models' arrays;
  esdf      tests/esdf_cases.model, and merge_cases.containing (the oracle's getContainingVoxel) for the point queries;
  chain     Resident: what a handle holds after tsdf_hip_march and the calls that work on its result -- sequence_model.cleaned_soup
            (the cleanup oracle, as Model.mesh uses it), flatten_cases.Flat, decimate_cases.Dec, smooth_cases.Model, normals_cases.Model -- by the
            lifetime rules of include/tsdf_hip.h.

Stats collects what the floors of the issue are asserted on (assert_floors), from the CPU replay and from the GPU run alike."""
import collections

import numpy as np

from tests import decimate_cases, esdf_cases, flatten_cases, merge_cases, normals_cases, smooth_cases
from tests.deintegrate_cases import RemovalModel
from tests.sequence_model import cleaned_soup

CHAIN_CALLS = ("march", "march_cleanup", "march_flatten", "march_decimate", "march_smooth", "march_normals", "march_fetch",
               "march_fetch_indexed", "march_fetch_normals")
INVALID = "E_INVALID"


class FeatureModel(RemovalModel):
    """RemovalModel that remembers the frames it integrated (to take one back out later, posed through the shifts since),
    merges another model into itself and computes distance fields."""

    def __init__(self, params, mode=None, cull=False):
        self.frames = []
        super().__init__(params, mode, cull)

    def reset(self):
        super().reset()
        self.frames = []   # what was integrated before is a stranger to the new volume

    def integrate(self, depth, bgra, trans):
        n = super().integrate(depth, bgra, trans)
        self.frames.append((depth, bgra, np.asarray(trans, np.float64).copy(), self.moved.copy()))
        return n

    def take_frame(self, k):
        """Frame k of those integrated since the last reset, as (pose to hand to the product NOW, depth, bgra)."""
        depth, bgra, trans, moved_then = self.frames.pop(k)
        t = np.eye(4)
        t[:3, 3] = -(self.moved - moved_then)
        return t @ trans, depth, bgra

    def arrays(self):
        return self.ov.d, self.ov.w, self.ov.rgb

    def merge(self, src, dst_from_src, min_weight):
        """tests/merge_cases.merge_model with this model as dst; returns the number of merged voxels."""
        d, w, rgb, m = merge_cases.merge_model(self.params, self.arrays(), src.params, src.arrays(), dst_from_src, min_weight)
        self.ov.d[...], self.ov.w[...] = d, w
        if rgb is not None:
            self.ov.rgb[...] = rgb
        return int(m.sum())

    def field(self, box=None, r_max=0, min_weight=0.0):
        """tests/esdf_cases.model of the voxels as they are now: dict(box, d2, dist, sites)."""
        box = esdf_cases.whole(self.params.res) if box is None else tuple(int(v) for v in box)
        d2, dist, n = esdf_cases.model(self.params, self.ov.d, self.ov.w, box, r_max, min_weight)
        return dict(box=box, d2=d2, dist=dist, sites=n)

    def distance(self, field, pts):
        """tsdf_hip_esdf_sample: the field's value at the voxel that CONTAINS each point (the oracle's getContainingVoxel);
        found only where that voxel exists and lies in the field's box."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        found, idx = merge_cases.containing(self.ov, pts, np.isfinite(pts).all(1))
        x0, y0, z0, nx, ny, nz = field["box"]
        i, j, k = idx[:, 0] - x0, idx[:, 1] - y0, idx[:, 2] - z0
        found &= (i >= 0) & (i < nx) & (j >= 0) & (j < ny) & (k >= 0) & (k < nz)
        out = np.full(len(pts), np.nan, np.float32)
        out[found] = field["dist"][k[found], j[found], i[found]]
        return out, found


def box_face_points(rng, box, res, size, n):
    """n points within one voxel of a face of `box` (x0, y0, z0, nx, ny, nz), in volume coordinates."""
    voxel = size / res
    lo, ext = np.array(box[:3], np.float64), np.array(box[3:], np.float64)
    pts = (lo + rng.uniform(0.0, 1.0, (n, 3)) * ext) * voxel - 0.5 * size
    axis, side = rng.randint(3, size=n), rng.randint(2, size=n)
    face = (lo + side[:, None] * ext)[np.arange(n), axis]
    pts[np.arange(n), axis] = (face + rng.uniform(-1.0, 1.0, n)) * voxel - 0.5 * size
    return pts


class Resident:
    """What a handle holds after tsdf_hip_march and the calls that work on its result, by the header's rules: flatten and
    decimate write the indexed mesh and the soup stays; smooth moves the indexed vertices; normals describe the indexed mesh
    while one is valid, else the soup; march and cleanup end the indexed mesh; march, cleanup, flatten, decimate and smooth end
    the normals.  All vertices are in the VOLUME frame.  Every method returns what the call reports, or INVALID."""

    def __init__(self):
        self.clear()
        self.cap = collections.Counter()   # the largest result of each kind this handle ever held (fetch buffers are sized by it)

    def clear(self):
        """A new handle."""
        self.soup = self.indexed = self.normals = None

    def _seen(self):
        if self.soup is not None:
            self.cap["tri"] = max(self.cap["tri"], len(self.soup["cells"]))
        if self.indexed is not None:
            self.cap["verts"] = max(self.cap["verts"], len(self.indexed["verts"]))
            self.cap["faces"] = max(self.cap["faces"], len(self.indexed["faces"]))
        if self.normals is not None:
            self.cap["normals"] = max(self.cap["normals"], len(self.normals))

    def march(self, ov, w_min, mode):
        verts, rgb, cells = ov.march(w_min, mode)
        self.soup = dict(verts=verts, rgb=rgb if mode else None, cells=cells, w_min=w_min, mode=mode)
        self.indexed = self.normals = None
        self._seen()
        return len(cells)

    def march_cleanup(self, face_dist, min_neighbors):
        if self.soup is None:
            return INVALID
        s = self.soup
        self.indexed = self.normals = None
        s["verts"], s["rgb"], s["cells"] = cleaned_soup(s["verts"], s["rgb"], s["cells"], face_dist, min_neighbors)
        return len(s["cells"])

    def _index(self, verts, rgb, faces, cells):
        self.indexed = dict(verts=np.ascontiguousarray(verts, np.float32).reshape(-1, 3), rgb=rgb,
                            faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), cells=cells)
        self.normals = None
        self._seen()
        return len(self.indexed["verts"]), len(self.indexed["faces"])

    def march_flatten(self, min_dist):
        if self.soup is None:
            return INVALID
        s = self.soup
        if not len(s["cells"]):
            return self._index(s["verts"], s["rgb"], np.empty((0, 3), np.int32), s["cells"])
        f = flatten_cases.Flat(s["verts"], None, min_dist)
        seeds = f.seeds.astype(np.int64)
        return self._index(f.vertices, s["rgb"][seeds] if s["rgb"] is not None else None, f.polygons, s["cells"][f.keep])

    def march_decimate(self, cell_size):
        if self.soup is None:
            return INVALID
        s = self.soup
        if not len(s["cells"]):
            return self._index(s["verts"], s["rgb"], np.empty((0, 3), np.int32), s["cells"])
        dec = decimate_cases.Dec(s["verts"], None, s["rgb"], cell_size)
        return self._index(dec.vertices, dec.rgb, dec.polygons, s["cells"][dec.keep])

    def march_smooth(self, lam, mu, iterations, keep_boundary):
        if self.indexed is None:
            return INVALID
        ix = self.indexed
        self.normals = None
        if not len(ix["verts"]):
            return 0
        m = smooth_cases.Model(ix["verts"], ix["faces"], lam, mu, iterations, keep_boundary)
        ix["verts"] = m.vertices
        return m.n_fixed

    def march_normals(self):
        if self.soup is None:
            return INVALID
        if self.indexed is not None:
            verts, faces = self.indexed["verts"], self.indexed["faces"]
        else:
            verts, faces = self.soup["verts"], None
        if not len(verts):
            self.normals = np.empty((0, 3), np.float32)
            return 0, 0
        m = normals_cases.Model(verts, faces)
        self.normals = m.normals
        self._seen()
        return len(m.normals), m.n_zero

    def triangles(self, call):
        """How many triangles the mesh has that a fetch returns (or describes, for the normals)."""
        if call == "march_fetch" or (call == "march_fetch_normals" and self.indexed is None):
            return len(self.soup["cells"])
        return len(self.indexed["faces"])


class Stats:
    """What the floors are asserted on, per shape."""

    def __init__(self):
        self.tally = collections.Counter()
        self.remove_drawn = self.remove_fell_back = self.chain_invalid = self.refused_with_kept = 0
        self.rng_end = []   # one draw from the driver's generator after the last step of each case: the draws were the same
        self.prelude_merges, self.random_merges, self.removals, self.prelude_fields, self.fetch_triangles = [], [], [], [], []

    def add(self, other):
        self.tally.update(other.tally)
        for k in ("remove_drawn", "remove_fell_back", "chain_invalid", "refused_with_kept"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        for k in ("prelude_merges", "random_merges", "removals", "prelude_fields", "fetch_triangles", "rng_end"):
            getattr(self, k).extend(getattr(other, k))

    def summary(self):
        share = lambda v, floor: f"{sum(x > floor for x in v)}/{len(v)}"  # noqa: E731
        return (f"{dict(self.tally)} remove fell back {self.remove_fell_back}/{self.remove_drawn}, prelude merges {self.prelude_merges}, "
                f"random merges > 100: {share(self.random_merges, 100)}, removals > 100: {share(self.removals, 100)}, prelude fields "
                f"{self.prelude_fields}, fetches > 300 triangles: {share(self.fetch_triangles, 300)}, E_INVALID states {self.chain_invalid}, refusals with a kept result "
                f"{self.refused_with_kept}")


def assert_floors(stats, operations, single, what):
    """The conditions on the inputs of one shape, over all its seeds: no comparison may pass on nothing.  (A set refuses
    remove, merge and esdf: there the steps are counted, and nothing is merged, removed or computed.)"""
    t = stats.tally
    for op in operations:
        assert t[op] >= 5, (what, op, dict(t))
    for call in CHAIN_CALLS:
        assert t["chain:" + call] >= 5, (what, call, dict(t))
    assert stats.chain_invalid >= 5, (what, stats.chain_invalid)
    halves = [("fetch_triangles", 300)]
    if single:
        assert 4 * stats.remove_fell_back <= stats.remove_drawn, (what, stats.remove_fell_back, stats.remove_drawn)
        assert stats.prelude_merges and all(n > 1000 for n in stats.prelude_merges), (what, stats.prelude_merges)
        assert stats.prelude_fields and all(n > 0 for n in stats.prelude_fields), (what, stats.prelude_fields)
        halves += [("random_merges", 100), ("removals", 100)]
    else:
        assert stats.refused_with_kept >= 5, (what, stats.refused_with_kept)
    for name, floor in halves:
        v = getattr(stats, name)
        assert v and 2 * sum(x > floor for x in v) >= len(v), (what, name, v)
