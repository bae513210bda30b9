"""GPU tier: random sequences of API calls through the entry points that came after tests/test_api_sequences_gpu.py --
tsdf_hip_deintegrate (remove), tsdf_hip_merge (merge), tsdf_hip_esdf* (esdf) and the resident-mesh calls tsdf_hip_march_cleanup /
_flatten / _decimate / _smooth / _normals with their three fetches (chain) -- mixed with every operation of that file, on one
handle and on a two-slab set (setDevices([0, 0])), checked after EVERY step against plain models.

What is checked is what one call leaves behind for the next.  A handle keeps five results side by side -- the soup, the
indexed mesh, the normals, the occupied list and the distance field -- in buffers that grow on demand and that unrelated calls
borrow; include/tsdf_hip.h says which later call keeps, replaces or ends each.  The driver keeps a SNAPSHOT of each (taken from
the model's voxels when the result was made; it does not follow the volume afterwards), lets the other steps of the sequence
run in between, and the next step on a result must still see the earlier one bit for bit, or E_INVALID where the header ends
it.  The band flags and the implied-distance record have two new writers with opposite rules (merge ends them on dst and
leaves src alone; deintegrate keeps them), followed through shifts, held-back ring frames, uploads and save / load.

Every expectation is composed from models that the per-feature tests pin bit for bit (tests/feature_cases.py); none comes
from the product.  FeatureDriver runs with or without a product: tests/test_sequence_model.py replays every case through the
models alone, with the same seeds and draws, and asserts the floors on the inputs there (feature_cases.assert_floors); the
last test of this file asserts them again on what really ran, so the file is meant to be run as a whole."""
import ctypes as C
import time
import types

import numpy as np
import pytest
import torch  # noqa: F401

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, backproject
from tests import esdf_cases, flatten_cases, merge_cases
from tests.common import assert_same_f32, make_volume
from tests.feature_cases import CHAIN_CALLS, INVALID, FeatureModel, Resident, Stats, assert_floors, box_face_points
from tests.sequence_model import assert_same_mesh, compare, record_for, slab_starts
from tests.sequence_util import march_stats, read_detail
from tests.test_api_sequences_gpu import MUTATING as PARENT_MUTATING
from tests.test_api_sequences_gpu import N_FRAMES, READING as PARENT_READING, SINGLE_ONLY, Driver
from tests.test_implied_d_gpu import open_scene

pytestmark = pytest.mark.gpu

SHAPES = {"one_handle": None, "set_0_0": [0, 0]}
# (grid, colour, seeds, shapes): seed 0 of every (shape, grid) is the prelude.  50^3: pitch 52 != nx, no octree levels (the
# closed-form centre tables), a partial flag cell
GRIDS = [(64, True, 6, ("one_handle", "set_0_0")), (64, False, 6, ("one_handle", "set_0_0")), (50, True, 4, ("one_handle",))]
# the seed sets whose draws meet the floors of tests/feature_cases.assert_floors on the CPU replay (tests/test_sequence_model.py)
SALT = {"one_handle": 0, "set_0_0": 2}
CASES = [(shape, res, color, seed) for shape in SHAPES for res, color, n, shapes in GRIDS if shape in shapes for seed in range(n)]
IDS = [f"{shape}-{res}-{'colour' if color else 'plain'}-seed{seed}" for shape, res, color, seed in CASES]
STEPS = 20
MUTATING = PARENT_MUTATING + ["remove", "remove", "merge", "merge"]
READING = PARENT_READING + ["esdf", "esdf", "chain", "chain", "chain", "chain", "chain"]
OPERATIONS = sorted(set(MUTATING + READING))
PRELUDE_CONDITIONS = ("a: a removal keeps the flags through a shift", "b: a removal flushes the ring frame it removes",
                      "c: a merge ends dst's flags and leaves src's", "d: the resident mesh, the list and the field survive unrelated calls",
                      "e: small results after large ones on one handle")
SET_CONDITIONS = ("d", "e", "r: a set refuses remove, merge and esdf and keeps everything")
STATS = {shape: Stats() for shape in SHAPES}
RAN, SECONDS = set(), {}
SENTINEL = 0xA5
SRC_RES = 32
U32P, U64P, I32P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


def guarded(n, shape, dtype):
    """A buffer for n rows and one more, every byte SENTINEL: a fetch writes the rows it returns and nothing else."""
    a = np.empty((n + 1,) + shape, dtype)
    a.view(np.uint8)[...] = SENTINEL
    return a


def untouched(a, n):
    return bool((a[n:].view(np.uint8) == SENTINEL).all())


def same_words(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


class FeatureDriver(Driver):
    """The Driver of tests/test_api_sequences_gpu.py with the newer operations.  live=False: no product -- every operation
    makes the same draws and acts on the models alone (the CPU replay)."""
    mutating = MUTATING

    def __init__(self, shape, res, color, seed, tmp_path, live=True):
        self.rng = rng = np.random.RandomState(31000 + 100000 * SALT[shape] + 1000 * list(SHAPES).index(shape) + 100 * res + 20 * int(color) + seed)
        self.shape, self.res, self.color, self.tmp_path, self.live = shape, res, color, tmp_path, live
        wmax, trunc, layout = 100.0, (0.03, 0.03), capi.LAYOUT_AUTO
        if seed > 0:   # (the parent driver's draws)
            wmax = float(rng.choice([100.0, 4.0, 2.5, 255.0]))
            trunc = [(0.03, 0.03), (0.05, 0.02), (0.01, 0.03)][rng.randint(3)]
            layout = capi.LAYOUT_F32W if rng.rand() < 0.15 else capi.LAYOUT_AUTO
        self.wmax, self.trunc, self.layout = wmax, trunc, layout
        self.vol, sc = make_volume(res, color=color, max_weight=wmax, trunc=trunc)
        self.vol.setLayout(layout)
        self.single = SHAPES[shape] is None
        if not self.single:
            self.vol.setDevices(SHAPES[shape])
        self.sc = open_scene(sc)
        self.packed = layout == capi.LAYOUT_AUTO   # (every max_weight drawn is in [0, 255])
        if live:
            self.vol.reset()
            assert (self.vol.getLayout() == capi.LAYOUT_PACKED) == self.packed
            self.lib = capi.load()
        self.model = FeatureModel(self.vol._p)
        self.rec = record_for(self.packed, trunc, wmax) if self.single else None
        if self.single:   # the seams of the parent's three-slab partition: planes like any other here
            self.starts = slab_starts(res)
        else:             # one seam; (starts[1 + randint(2)] and starts[1:3] of the parent's draws both name it)
            mid = slab_starts(res, 2)[1]
            self.starts = [0, mid, mid, res]
            if live:
                assert [s[1] for s in self.vol.slabs()] == [0, mid]
        self.thick = max(b - a for a, b in zip(self.starts, self.starts[1:]))
        self.voxel = self.sc.size / res
        self.frame_no, self.keep, self.cum = 0, [], [0, 0, 0]
        self.pairing, self.held = False, False
        self.stale = None      # (idx of an occupied list, whether a later step ended it)
        self.field = None      # the distance field the handle holds: FeatureModel.field's dict and "ended"
        self.resident = Resident()
        self.src, self.merges = None, 0
        self.stats, self.quiet, self.ran_as = Stats(), False, None

    def compare(self, what):
        if self.live:
            compare(self.vol, self.model.ov, what)

    def close(self):
        if self.live:
            self.vol.close()
            if self.src is not None:
                self.src.vol.close()

    def check_detail(self, allowed, what, counted=False):
        if self.live:
            super().check_detail(allowed, what, counted)

    def moved_by(self, s):
        p = self.vol._p
        return np.array([int(s[a]) * float(p.size[a]) / int(p.res[a]) for a in range(3)], np.float64)

    def new_handle(self):
        """vol.reset() and vol.load() make a new handle: it holds none of the kept results."""
        self.resident.clear()
        if self.field:
            self.field["ended"] = True
        if self.stale:
            self.stale = (self.stale[0], True)

    # ---- the inherited operations without a product: the same draws, the model alone ---------------------------------------------
    def op_host(self, what, count=None, pipelined=None):
        if self.live:
            return super().op_host(what, count, pipelined)
        T, dep, col = self.next_frame()
        want = self.model.integrate(dep, col, T)
        if count is None:
            self.rng.randint(2)
        if pipelined is None:
            self.rng.randint(2)
        self.launched()
        return want

    def op_device(self, what):
        if self.live:
            return super().op_device(what)
        T, dep, col = self.next_frame()
        self.model.integrate(dep, col, T)
        self.rng.randint(2)
        self.launched()

    def op_pair(self, what):
        if self.live:
            return super().op_pair(what)
        for _ in range(2):
            T, dep, col = self.next_frame()
            self.model.integrate(dep, col, T)
        self.launched(2)

    def op_staged(self, what):
        if self.live:
            return super().op_staged(what)
        T, dep, col = self.next_frame()
        xyz = backproject(dep, self.sc.fx, self.sc.fy, self.sc.cx, self.sc.cy)
        d_ref, c_ref, _ = self.model.ov.organize(xyz, np.ascontiguousarray(col[~np.isnan(dep)]) if self.color else None)
        self.model.integrate(d_ref, c_ref if self.color else None, T)
        self.rng.randint(2)
        self.launched()

    def op_ring(self, what, n=None):
        if self.live:
            return super().op_ring(what, n)
        self.pairing = True
        for _ in range(int(self.rng.randint(1, 4)) if n is None else n):
            T, dep, col = self.next_frame()
            self.model.integrate(dep, col, T)
            self.launched()
            self.held = not self.held

    def op_shift(self, what, s=None):
        if self.live:
            s = super().op_shift(what, s)
        else:
            s = self.draw_shift() if s is None else s
            self.model.shift(s, self.moved_by(s))
            self.cum = [c + v for c, v in zip(self.cum, s)]
            if any(s) and self.stale:
                self.stale = (self.stale[0], True)
        if any(s) and self.field:
            self.field["ended"] = True   # the indices moved
        return s

    def op_upload(self, what, box=None, which=None):
        if self.live:
            return super().op_upload(what, box, which)
        x0, y0, z0, nx, ny, nz = self.seam_box() if box is None else box
        d, w, rgb = (a.copy() if a is not None else None for a in self.model.box(x0, y0, z0, nx, ny, nz))
        seen = w > 0
        which = ["d", "w", "all"][self.rng.randint(3)] if which is None else which
        if which in ("d", "all"):
            d[seen] = np.maximum(d[seen] - np.float32(0.125), np.float32(-1.0))
        if which in ("w", "all"):
            w = np.floor(w * np.float32(0.5))
        if which == "all" and rgb is not None:
            rgb = 255 - rgb
        self.model.upload(x0=x0, y0=y0, z0=z0, d=d if which != "w" else None, w=w if which != "d" else None, rgb=rgb if which == "all" else None)
        if self.single:
            self.rec.foreign_write()
        return int(seen.sum())

    def op_set_planes(self, what):
        if self.live:
            return super().op_set_planes(what)
        res, ov = self.res, self.model.ov
        z0, nz = int(self.rng.randint(res - 4)), int(self.rng.randint(1, 4))
        hit = np.argwhere((ov.w[z0:z0 + nz] > 0) & (ov.d[z0:z0 + nz] > 0))
        if len(hit):
            ov.d[z0 + hit[0][0], hit[0][1], hit[0][2]] = np.float32(-0.5)
        self.rec.foreign_write()

    def op_device_planes(self, what):
        if self.live:
            return super().op_device_planes(what)
        self.rec.foreign_write()

    def op_save_load(self, what):
        if self.live:
            super().op_save_load(what)
        elif self.single:
            self.rec.reset()
            self.rec.foreign_write()
        self.new_handle()

    def op_reset(self, what):
        if self.live:
            super().op_reset(what)
        else:
            self.model.reset()
            if self.single:
                self.rec.reset()
        self.new_handle()

    def op_occupied(self, what):
        if self.live:
            return super().op_occupied(what)
        self.seam_box()

    def op_render(self, what, trans=None, ds=None):
        if self.live:
            return super().op_render(what, trans, ds)
        if trans is None:
            self.look_at()
        if ds is None:
            self.rng.choice([1, 2, 3])

    def op_sample(self, what):
        if self.live:
            return super().op_sample(what)
        rng = self.rng
        rng.uniform(-0.5, 0.5, (400, 3))
        rng.randint(2, size=100)
        rng.uniform(-1.0, 1.0, 100)

    def op_align(self, what):
        if self.live:
            return super().op_align(what)
        rng = self.rng
        tr = synth.turntable_pose(rng.uniform(0, N_FRAMES), N_FRAMES, self.sc.size, tilt=0.1)
        n = int(np.isfinite(self.sc.depth(tr)).sum())   # (backproject keeps the pixels with a depth)
        if n > 1500:
            rng.choice(n, 1500, replace=False)
        rng.normal(size=3)
        rng.normal(size=3)
        rng.choice([0.0, 1.0])

    def make_list(self):
        if self.live:
            return super().make_list()
        self.stale = (None, False)

    def check_list(self, what):
        if self.live:
            return super().check_list(what)
        self.stale = None

    # ---- remove ---------------------------------------------------------------------------------------------------------------
    def refused(self, call, what):
        with pytest.raises(capi.TsdfHipError) as err:
            call()
        assert err.value.code == capi.E_UNSUPPORTED, (what, err.value.code)

    def op_remove(self, what, k=None, stranger=None):
        """deintegrateCloud of a frame integrated earlier in this sequence, posed through the shifts since; one time in four
        of a stranger.  Without a frame to remove the step integrates one (host)."""
        rng, model = self.rng, self.model
        stranger = bool(rng.rand() < 0.25) if stranger is None else stranger
        if not self.single:
            T, dep, col = self.next_frame()
            if self.live:
                self.refused(lambda: self.vol.deintegrateCloud(dep, col, T, count=True), what)
            return None
        self.stats.remove_drawn += 1
        if not stranger and not model.frames:
            self.stats.remove_fell_back += 1
            self.ran_as = "host"
            return self.op_host(what)
        if stranger:
            T, dep, col = self.next_frame()
        else:
            T, dep, col = model.take_frame(int(rng.randint(len(model.frames))) if k is None else k)
        want = model.deintegrate(dep, col, T)
        if self.live:
            n = self.vol.deintegrateCloud(dep, col, T, count=True)
            got = self.vol.deintegrateStats()[:3]
            assert n == want[1] and got == want, (what, n, got, want)
        if self.field:
            self.field["ended"] = True   # tsdf_hip_deintegrate invalidates the distance field
        self.stats.removals.append(want[1])
        return want

    # ---- merge ----------------------------------------------------------------------------------------------------------------
    def source(self):
        """The second volume: cubic, 32^3 over the same extent (voxels twice as large), the same truncation limits, layout,
        max_weight and colour setting, fused from 2 - 3 frames."""
        if self.src is None:
            vol, _ = make_volume(SRC_RES, color=self.color, max_weight=self.wmax, trunc=self.trunc, size=self.sc.size)
            vol.setLayout(self.layout)
            if self.live:
                vol.reset()
                assert vol.getLayout() == self.vol.getLayout()
            self.src = types.SimpleNamespace(vol=vol, model=FeatureModel(vol._p), rec=record_for(self.packed, self.trunc, self.wmax))
            for _ in range(2 + int(self.rng.randint(2))):
                self.src_frame("the first frames of src")
        return self.src

    def src_frame(self, what, count=False):
        src, k = self.src, int(self.rng.randint(N_FRAMES))
        tr = synth.turntable_pose(k, N_FRAMES, self.sc.size, tilt=0.2 * np.cos(k))
        dep, col = self.sc.depth(tr, noise_seed=700 + k), (self.sc.bgra(k) if self.color else None)
        want = src.model.integrate(dep, col, tr)
        allowed = src.rec.fast_launch()
        if self.live:
            n = src.vol.integrateCloud(dep, col, tr, count=count)
            if count:
                assert n == want, (what, n, want)
                assert read_detail(src.vol)[1] == int(allowed), (what, allowed, src.rec.__dict__)
        return want

    def draw_transform(self):
        v = self.voxel
        return [np.eye(4), merge_cases.rigid((1, 0, 0), 0.0, (0.3 * v, -0.45 * v, 0.2 * v)),
                merge_cases.rigid((1, 2, 3), 0.3, (2.5 * v, -1.25 * v, 3.0 * v))][self.rng.randint(3)]

    def op_merge(self, what, G=None, min_weight=None, prelude=False):
        """mergeVolume(src, G, min_weight, count=True); afterwards src is unchanged in every respect that can be read."""
        src = self.source()
        if self.merges % 3 == 2:
            self.src_frame(f"{what}: one more frame for src")
        self.merges += 1
        G = self.draw_transform() if G is None else G
        min_weight = float(self.rng.choice([0.0, 1.0])) if min_weight is None else min_weight
        if not self.single:
            if self.live:
                self.refused(lambda: self.vol.mergeVolume(src.vol, G, min_weight, count=True), f"{what}: the set as dst")
                self.refused(lambda: src.vol.mergeVolume(self.vol, G, min_weight, count=True), f"{what}: the set as src")
                compare(src.vol, src.model.ov, f"src {what}")
            return 0
        want = self.model.merge(src.model, G, min_weight)
        flags_live = self.rec.flags_describe_planes
        if self.live:
            n = self.vol.mergeVolume(src.vol, G, min_weight, count=True)
            st = self.vol.mergeStats()
            assert n == want and st[1:3] == (want, int(flags_live)), (what, n, want, st, flags_live)
        self.rec.foreign_write()   # dst's flags no longer describe its planes, exactly as after an upload
        if self.live:
            compare(src.vol, src.model.ov, f"src {what}")
            n = C.c_uint64(0)
            capi.check(self.lib.tsdf_hip_march(src.vol._need(), 1.0, 1 if self.color else 0, C.byref(n)), "march")
            tri = src.model.ov.march(1.0, 1 if self.color else 0)[2]
            assert n.value == len(tri) and march_stats(src.vol)[3] & 1 == 1, (what, n.value, len(tri), march_stats(src.vol))
        self.src_frame(f"{what}: the next frame of src", count=True)
        (self.stats.prelude_merges if prelude else self.stats.random_merges).append(want)
        return want

    # ---- esdf -----------------------------------------------------------------------------------------------------------------
    def seam_box(self, seam=None):
        x0, y0, z0, nx, ny, nz = super().seam_box(seam)
        return x0, y0, z0, nx, ny, min(nz, self.res - z0)

    def draw_field(self):
        rng = self.rng
        return int(rng.choice([0, 6])), float(rng.choice([0.0, 1.0])), (None if rng.rand() < 0.5 else self.seam_box())

    def compute_field(self, what, r_max, min_weight, box, model=True):
        f = self.model.field(box, r_max, min_weight) if (self.live or model) else dict(box=box or esdf_cases.whole(self.vol._p.res), sites=None)
        if self.live:
            n = self.vol.computeDistanceField(r_max, min_weight, box)
            assert n == f["sites"], (what, n, f["sites"])
        f["ended"] = False
        self.field = f
        return f

    def query_points(self, n_inside, n_faces):
        S, f = self.sc.size, self.field
        return np.concatenate([self.rng.uniform(-0.5 * S, 0.5 * S, (n_inside, 3)),
                               box_face_points(self.rng, f["box"], self.res, S, n_faces)]).astype(np.float32)

    def check_field(self, what, n_inside=30, n_faces=10):
        """include/tsdf_hip.h, LIFETIME: the field describes the volume at the time of the call and stays valid, STALE BY
        DESIGN, across every later writer except those that end it -- shift, deintegrate, reset, load: then the fetches and the
        sample return E_INVALID."""
        f = self.field
        pts = self.query_points(n_inside, n_faces)
        if not self.live:
            self.field = None if f["ended"] else f
            return
        x0, y0, z0, nx, ny, nz = f["box"]
        h, lib = self.vol._need(), self.lib
        d2, dist = guarded(nx * ny * nz, (), np.uint32), guarded(nx * ny * nz, (), np.float32)
        val, found = np.empty(len(pts), np.float32), np.empty(len(pts), np.uint8)
        rcs = (lib.tsdf_hip_esdf_fetch(h, d2.ctypes.data_as(U32P), capi.as_f32p(dist)), lib.tsdf_hip_esdf_fetch_device(h, None, None),
               lib.tsdf_hip_esdf_sample(h, capi.as_f32p(pts), len(pts), capi.as_f32p(val), capi.as_u8p(found)))
        if f["ended"]:
            assert rcs == (capi.E_INVALID,) * 3, (what, rcs)
            assert untouched(d2, 0) and untouched(dist, 0), what
            self.field = None
            return
        assert rcs == (capi.OK,) * 3, (what, rcs)
        n = nx * ny * nz
        assert same_words(d2[:n].reshape(nz, ny, nx), f["d2"]), f"{what}: d2 of the earlier field"
        assert same_words(dist[:n].reshape(nz, ny, nx), f["dist"]), f"{what}: dist of the earlier field"
        assert untouched(d2, n) and untouched(dist, n), what
        want, want_found = self.model.distance(f, pts)
        assert np.array_equal(found.astype(bool), want_found), f"{what}: found"
        assert same_words(val[want_found], want[want_found]) and np.isnan(val[~want_found]).all(), f"{what}: getDistance"

    def op_esdf(self, what, args=None, prelude=False):
        """computeDistanceField, both planes of the field and getDistance on 400 points, a quarter within a voxel of the
        box's faces."""
        r_max, min_weight, box = self.draw_field() if args is None else args
        if not self.single:
            if self.live:
                self.refused(lambda: self.vol.computeDistanceField(r_max, min_weight, box), what)
            return None
        f = self.compute_field(f"{what} r_max {r_max} min_weight {min_weight} box {box}", r_max, min_weight, box, model=prelude)
        self.check_field(what, 300, 100)
        if prelude:
            self.stats.prelude_fields.append(f["sites"])
        return f

    # ---- mesh: the inherited reader with the newer extras --------------------------------------------------------------------------
    def op_mesh(self, what, w_min=None, cleanup=None, flatten=None, extras=True):
        """reconstruct() with setCleanup / setFlatten as the parent draws them and setDecimate(2 voxels), setSmooth(3) and
        setNormals() with the same probability, against the composed models.  It marches on the handle: the snapshot follows."""
        rng, R, mode = self.rng, self.resident, 1 if self.color else 0
        w_min = float(rng.choice([0.0, 1.0, 2.5])) if w_min is None else w_min
        if extras and rng.rand() < 0.3:
            cleanup = (1.5 * self.voxel, int(rng.choice([3, 40])))
        if extras and rng.rand() < 0.3:
            flatten = flatten_cases.MD
        decimate = 2 * self.voxel if extras and rng.rand() < 0.3 else None
        smooth = 3 if extras and rng.rand() < 0.3 else None
        normals = bool(extras and rng.rand() < 0.3)
        R.march(self.model.ov, w_min, mode)
        if cleanup:
            R.march_cleanup(*cleanup)
        if decimate is not None:
            R.march_decimate(decimate)           # (with setFlatten as well, decimate runs and flatten is skipped)
        elif flatten is not None or smooth is not None:
            R.march_flatten(0.0001 if flatten is None else flatten)
        if smooth is not None:
            R.march_smooth(0.5, -0.53, smooth, 1)
        if normals:
            R.march_normals()
        if not self.live:
            return None, None
        mc = MarchingCubesTSDFOctree()
        mc.setInputTSDF(self.vol)
        mc.setMinWeight(w_min)
        mc.setColorByRGB(self.color)
        if cleanup:
            mc.setCleanup(*cleanup)
        if flatten:
            mc.setFlatten(flatten)
        if decimate is not None:
            mc.setDecimate(decimate)
        if smooth is not None:
            mc.setSmooth(smooth)
        mc.setNormals(normals)
        got = mc.reconstruct(want_cells=True)
        st = march_stats(self.vol)
        what = f"{what} w_min {w_min} cleanup {cleanup} flatten {flatten} decimate {decimate} smooth {smooth} normals {normals}"
        if R.indexed is not None:
            ix = R.indexed
            want = {"vertices": self.model.to_world(ix["verts"]), "polygons": ix["faces"], "rgb": ix["rgb"], "cells": ix["cells"]}
        else:
            s, n = R.soup, len(R.soup["cells"])
            want = {"vertices": self.model.to_world(s["verts"]), "polygons": np.arange(3 * n, dtype=np.int32).reshape(n, 3), "rgb": s["rgb"],
                    "cells": s["cells"]}
        assert_same_mesh(got, want, what)
        if normals:   # (the global transform is a translation: the normals are the volume frame's)
            assert same_words(got["normals"], R.normals), f"{what}: normals"
        if self.single and not self.rec.flags_describe_planes:
            assert st[3] & 1 == 0, (what, st)
        return got, st

    # ---- chain: one step of the resident-mesh state machine, through the C entry points ------------------------------------------------
    def op_chain(self, what, call=None, **kw):
        rng, R, mode = self.rng, self.resident, 1 if self.color else 0
        call = CHAIN_CALLS[rng.randint(len(CHAIN_CALLS))] if call is None else call
        if call == "march_fetch" and R.soup is None:
            call = "march"   # (tsdf_hip_march_fetch before any march: the header promises nothing)
        self.stats.tally["chain:" + call] += 1
        what = f"{what} {call}"
        lib, h = (self.lib, self.vol._need()) if self.live else (None, None)
        a, b = C.c_uint64(7), C.c_uint64(7)

        def reported(rc, want, got):
            if want is INVALID:
                assert rc == capi.E_INVALID, (what, rc)
            else:
                assert rc == capi.OK and got == want, (what, rc, got, want)

        if call == "march":
            w_min = kw.get("w_min", None)
            w_min = float(rng.choice([0.0, 1.0, 2.5])) if w_min is None else w_min
            want = R.march(self.model.ov, w_min, mode)
            if self.live:
                reported(lib.tsdf_hip_march(h, w_min, mode, C.byref(a)), want, a.value)
                if self.single and not self.rec.flags_describe_planes:
                    assert march_stats(self.vol)[3] & 1 == 0, what
        elif call == "march_cleanup":
            args = (1.5 * self.voxel, int(rng.choice([3, 40])))
            want = R.march_cleanup(*args)
            if self.live:
                reported(lib.tsdf_hip_march_cleanup(h, args[0], args[1], C.byref(a)), want, a.value)
        elif call in ("march_flatten", "march_decimate"):
            arg = flatten_cases.MD if call == "march_flatten" else 2 * self.voxel
            want = getattr(R, call)(arg)
            if self.live:
                reported(getattr(lib, "tsdf_hip_" + call)(h, arg, C.byref(a), C.byref(b)), want, (a.value, b.value))
        elif call == "march_smooth":
            iterations, keep = int(rng.randint(1, 4)), int(rng.randint(2))
            want = R.march_smooth(0.5, -0.53, iterations, keep)
            if self.live:
                reported(lib.tsdf_hip_march_smooth(h, 0.5, -0.53, iterations, keep, C.byref(a)), want, a.value)
        elif call == "march_normals":
            want = R.march_normals()
            if self.live:
                reported(lib.tsdf_hip_march_normals(h, C.byref(a), C.byref(b)), want, (a.value, b.value))
        else:
            want = self.fetch(call, what)
        if want is INVALID:
            self.stats.chain_invalid += 1
        return want

    def fetch(self, call, what):
        """One of the three fetches into buffers as long as the longest result the handle ever held (and one row): the rows
        of the snapshot bit for bit, nothing behind them."""
        R, cap, live = self.resident, self.resident.cap, self.live
        lib, h = (self.lib, self.vol._need()) if live else (None, None)
        if call == "march_fetch":
            s, n = R.soup, len(R.soup["cells"])
            self.stats.fetch_triangles.append(n)
            if live:
                verts, rgb, cells = guarded(cap["tri"], (3, 3), np.float32), guarded(cap["tri"], (3, 3), np.uint8), guarded(cap["tri"], (), np.uint64)
                capi.check(lib.tsdf_hip_march_fetch(h, capi.as_f32p(verts), capi.as_u8p(rgb) if s["mode"] else None, cells.ctypes.data_as(U64P)), what)
                assert same_words(verts[:n].reshape(-1, 3), s["verts"]) and same_words(cells[:n], s["cells"]), f"{what}: the soup of the earlier march"
                assert not s["mode"] or same_words(rgb[:n].reshape(-1, 3), s["rgb"]), f"{what}: rgb"
                assert untouched(verts, n) and untouched(rgb, n if s["mode"] else 0) and untouched(cells, n), f"{what}: rows behind the soup"
            return n
        if call == "march_fetch_indexed":
            ix = R.indexed
            if live:
                verts, rgb = guarded(cap["verts"], (3,), np.float32), guarded(cap["verts"], (3,), np.uint8)
                faces, cells = guarded(cap["faces"], (3,), np.uint32), guarded(cap["faces"], (), np.uint64)
                with_rgb = ix is not None and ix["rgb"] is not None
                rc = lib.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(verts), capi.as_u8p(rgb) if with_rgb else None, faces.ctypes.data_as(U32P),
                                                      cells.ctypes.data_as(U64P))
            if ix is None:
                if live:
                    assert rc == capi.E_INVALID and untouched(verts, 0) and untouched(faces, 0), (what, rc)
                return INVALID
            m, k = len(ix["verts"]), len(ix["faces"])
            self.stats.fetch_triangles.append(k)
            if live:
                assert rc == capi.OK, (what, rc)
                assert same_words(verts[:m], ix["verts"]), f"{what}: vertices of the indexed mesh"
                assert same_words(faces[:k].view(np.int32), ix["faces"]) and same_words(cells[:k], ix["cells"]), f"{what}: faces, cells"
                assert not with_rgb or same_words(rgb[:m], ix["rgb"]), f"{what}: rgb"
                assert untouched(verts, m) and untouched(rgb, m if with_rgb else 0) and untouched(faces, k) and untouched(cells, k), what
            return m, k
        assert call == "march_fetch_normals", call
        if live:
            out = guarded(cap["normals"], (3,), np.float32)
            rc = lib.tsdf_hip_march_fetch_normals(h, capi.as_f32p(out))
        if R.normals is None:
            if live:
                assert rc == capi.E_INVALID and untouched(out, 0), (what, rc)
            return INVALID
        n = len(R.normals)
        self.stats.fetch_triangles.append(R.triangles(call))
        if live:
            assert rc == capi.OK and same_words(out[:n], R.normals) and untouched(out, n), (what, rc)
        return n

    # ---- the occupied list, as a kept result --------------------------------------------------------------------------------------
    def keep_list(self, what, box=None):
        """tsdf_hip_occupied and a fetch into buffers one row longer than the list: the model's list, nothing behind it."""
        want = self.model.occupied(box)
        if self.live:
            n = C.c_uint64(0)
            capi.check(self.lib.tsdf_hip_occupied(self.vol._need(), (C.c_int32 * 6)(*box) if box else None, C.byref(n)), "occupied")
            assert n.value == len(want[0]), (what, n.value, len(want[0]))
        self.stale = (want[0].copy(), False)
        self.cap_list = max(getattr(self, "cap_list", 0), len(want[0]))
        self.look_at_list(what)
        return len(want[0])

    def look_at_list(self, what):
        """check_list without forgetting the list."""
        want_idx, ended = self.stale
        if not self.live:
            return
        idx, d = guarded(self.cap_list, (3,), np.int32), guarded(self.cap_list, (), np.float32)
        rc = self.lib.tsdf_hip_occupied_fetch(self.vol._need(), idx.ctypes.data_as(I32P), capi.as_f32p(d), None, None)
        if ended:
            assert rc == capi.E_INVALID and untouched(idx, 0), (what, rc)
            return
        n = len(want_idx)
        assert rc == capi.OK and same_words(idx[:n], want_idx) and untouched(idx, n) and untouched(d, n), (what, rc)
        assert_same_f32(d[:n], self.model.ov.d[want_idx[:, 2], want_idx[:, 1], want_idx[:, 0]], f"values of the earlier list {what}")

    def c_reset(self, what):
        """tsdf_hip_reset on the SAME handle (vol.reset() makes a new one): the planes, the flags and the record start over;
        the distance field and the normals are dropped; the soup, the indexed mesh and the occupied list are plain data and
        stay (the list's fetch gathers the reset values)."""
        if self.live:
            capi.check(self.lib.tsdf_hip_reset(self.vol._need()), "reset")
        self.model.reset()
        if self.single:
            self.rec.reset()
        self.resident.normals = None
        if self.field:
            self.field["ended"] = True
        self.compare(what)

    # ---- one step -------------------------------------------------------------------------------------------------------------
    def step(self, op, what, **kw):
        mutating = op in self.mutating
        if mutating and op != "ring" and not self.pairing and not self.quiet:
            if self.rng.rand() < 0.5:
                self.make_list()
            if self.single and self.rng.rand() < 0.5:
                self.compute_field(f"{what}: a field before the step", *self.draw_field(), model=False)
        if op != "ring":
            self.before(op)
        self.ran_as = op
        if not self.single and op in ("remove", "merge", "esdf") and (self.resident.soup is not None or self.stale):
            self.stats.refused_with_kept += 1   # a refusal that a kept result has to outlive
        out = getattr(self, "op_" + op)(what, **kw)
        self.after(op)
        self.stats.tally[self.ran_as] += 1
        if mutating and not self.quiet:
            if self.stale:
                self.check_list(what)
            if self.field:
                self.check_field(f"{what}: the field made before")
        if not self.held:
            self.compare(what)
        return out

    def after(self, op):
        if self.pairing and op != "ring":
            if self.live:
                self.vol.setFramePairing(False)
            self.pairing = False

    def random_steps(self, n, tag):
        ops = [o for o in MUTATING + READING if (self.single or o not in SINGLE_ONLY) and (o != "save_load" or self.res == 64)]
        for k in range(n):   # (the .vol format needs a cubic power-of-two grid: no save_load at 50^3)
            op = ops[self.rng.randint(len(ops))]
            self.step(op, f"{tag} step {k} {op}")


def prelude(dr, tag):
    """The scripted start of every (shape, grid): returns the conditions that really happened."""
    happened, single, R = set(), dr.single, dr.resident
    assert dr.packed and dr.wmax == 100.0
    flags_in_use = lambda: march_stats(dr.vol)[3] & 1   # noqa: E731
    detail_on = lambda: read_detail(dr.vol)[1]           # noqa: E731
    if single:
        # (a) three frames, a z shift that carries the flags, the middle frame removed (posed through the shift): the next march
        # goes through the flags and the next counted integrate rebuilds distances from counts
        for k in range(3):
            dr.step("host", f"{tag} (a) frame {k}", count=(k == 2), pipelined=False)
        dr.step("shift", f"{tag} (a) z shift", s=(0, 0, 5))
        assert dr.rec.flags_describe_planes and (not dr.live or dr.vol.shiftStats()[2] == 1)
        dr.compute_field(f"{tag} (a) a field for the removal to end", 0, 0.0, None)
        st = dr.step("remove", f"{tag} (a) the middle frame", k=1, stranger=False)   # (step() finds the field ended)
        assert st[1] > 1000 and dr.field is None, st
        assert dr.step("chain", f"{tag} (a)", call="march", w_min=1.0) > 300
        assert not dr.live or flags_in_use() == 1
        assert dr.step("host", f"{tag} (a) a frame after the removal", count=True, pipelined=False) > 0
        assert not dr.live or detail_on() == 1
        happened.add("a")
        # (b) a ring frame is held back; the removal of that very frame launches it first
        dr.step("ring", f"{tag} (b) ring", n=1)
        assert dr.held
        st = dr.step("remove", f"{tag} (b) the frame that waits", k=len(dr.model.frames) - 1, stranger=False)
        assert st[1] > 1000 and not dr.held, st
        happened.add("b")
        # (c) a merge into a dst whose flags are live ends them; src keeps its own (op_merge); a removal afterwards keeps none
        assert dr.rec.flags_describe_planes
        dr.compute_field(f"{tag} (c) a field for the merge to leave stale", 6, 0.0, None)
        assert dr.step("merge", f"{tag} (c) merge", G=merge_cases.rigid((1, 2, 3), 0.3, (2.5 * dr.voxel, -1.25 * dr.voxel, 3.0 * dr.voxel)),
                       min_weight=0.0, prelude=True) > 1000
        assert not dr.rec.flags_describe_planes and (not dr.live or dr.vol.mergeStats()[2] == 1)
        assert dr.field is not None and not dr.field["ended"]   # (step() fetched it: valid, and the volume's before the merge)
        assert dr.step("chain", f"{tag} (c)", call="march", w_min=1.0) > 300
        assert not dr.live or flags_in_use() == 0
        dr.step("host", f"{tag} (c) a frame after the merge", count=True, pipelined=False)
        assert not dr.live or detail_on() == 0
        st = dr.step("remove", f"{tag} (c) a removal after the merge", k=0, stranger=False)
        assert st[1] > 1000, st
        assert dr.step("chain", f"{tag} (c) after the removal", call="march", w_min=1.0) > 300
        assert not dr.live or flags_in_use() == 0
        assert dr.src.rec.flags_describe_planes
        happened.add("c")
    else:
        for k in range(4):
            dr.step("host", f"{tag} frame {k}", count=(k == 3), pipelined=False)
        # (r) the refusals, with every result a set can keep alive across them: the soup, the indexed mesh, the normals and the
        # occupied list still fetch as made (step() finds the planes as before), and the flags' readers read as before
        dr.quiet = True
        assert dr.step("chain", f"{tag} (r)", call="march", w_min=1.0) > 300
        mk = dr.step("chain", f"{tag} (r)", call="march_decimate")
        assert mk[1] > 300 and dr.step("chain", f"{tag} (r)", call="march_normals")[0] == mk[0]
        assert dr.keep_list(f"{tag} (r) occupied") > 1000
        before = (march_stats(dr.vol), read_detail(dr.vol)) if dr.live else None
        assert not dr.live or (before[0][3] & 1 == 1 and before[1][1] == 1), before   # the flags and the implied distances are in use
        refusals = dr.stats.tally["remove"] + dr.stats.tally["merge"] + dr.stats.tally["esdf"]
        for op in ("remove", "merge", "esdf"):
            assert not dr.step(op, f"{tag} (r) refused {op}")   # (None or 0: nothing was removed, merged or computed)
        assert dr.stats.tally["remove"] + dr.stats.tally["merge"] + dr.stats.tally["esdf"] == refusals + 3
        assert not dr.live or (march_stats(dr.vol), read_detail(dr.vol)) == before
        assert dr.step("chain", f"{tag} (r) after the refusals", call="march_fetch") > 300
        assert dr.step("chain", f"{tag} (r) after the refusals", call="march_fetch_indexed") == mk
        assert dr.step("chain", f"{tag} (r) after the refusals", call="march_fetch_normals") == mk[0]
        assert not dr.stale[1]
        dr.look_at_list(f"{tag} (r) after the refusals")
        assert dr.step("chain", f"{tag} (r) the next march", call="march", w_min=1.0) > 300   # ... and what they decide is as before
        assert not dr.live or flags_in_use() == 1
        assert dr.step("host", f"{tag} (r) the next counted frame", count=True, pipelined=False) > 0
        assert not dr.live or detail_on() == 1
        dr.stale, dr.quiet = None, False
        happened.add("r")
    # (d) the resident mesh survives unrelated calls, the list and the field until the shift ends both
    dr.quiet = True
    n_first = dr.step("chain", f"{tag} (d)", call="march", w_min=1.0)
    first = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in R.soup.items()}
    assert n_first > 300
    assert dr.keep_list(f"{tag} (d) occupied") > 1000
    if single:
        dr.step("esdf", f"{tag} (d) esdf", args=(0, 0.0, None), prelude=True)
    dr.step("render", f"{tag} (d) render", trans=dr.look_at(target=-np.array(dr.cum) * dr.voxel, direction=(0.5, 0.3, 1.0)), ds=1)
    assert 0 < dr.step("chain", f"{tag} (d)", call="march_cleanup") <= n_first
    dr.look_at_list(f"{tag} (d) after the cleanup")
    dr.step("sample", f"{tag} (d) sample")
    m, k = dr.step("chain", f"{tag} (d)", call="march_decimate")
    assert 0 < m < 3 * n_first and k > 300
    dr.step("host", f"{tag} (d) an integrate", count=False, pipelined=False)
    dr.look_at_list(f"{tag} (d) after the integrate")
    if single:
        assert not dr.field["ended"]
        dr.check_field(f"{tag} (d) after the integrate")
        assert dr.field is not None
    dr.step("chain", f"{tag} (d)", call="march_smooth")
    dr.step("shift", f"{tag} (d) shift", s=(1, 0, -2))
    dr.look_at_list(f"{tag} (d) after the shift")
    assert dr.stale[1]
    if single:
        assert dr.field["ended"]
        dr.check_field(f"{tag} (d) after the shift")
    assert dr.step("chain", f"{tag} (d)", call="march_normals")[0] == m
    assert dr.step("chain", f"{tag} (d)", call="march_fetch") == len(R.soup["cells"]) <= n_first
    assert dr.step("chain", f"{tag} (d)", call="march_fetch_indexed") == (m, k)
    assert dr.step("chain", f"{tag} (d)", call="march_fetch_normals") == m
    assert R.soup["w_min"] == first["w_min"] and np.isin(R.soup["cells"], first["cells"]).all()   # the mesh of the first march
    dr.stale = None
    happened.add("d")
    # (e) small after large, on ONE handle (tsdf_hip_reset: vol.reset() would make a new one)
    large = dr.step("chain", f"{tag} (e) large", call="march", w_min=0.0)
    dr.step("chain", f"{tag} (e) large", call="march_fetch")
    dr.step("chain", f"{tag} (e) large", call="march_normals")
    n_list = dr.keep_list(f"{tag} (e) the whole grid")
    if single:
        dr.step("esdf", f"{tag} (e) the whole grid", args=(0, 0.0, None), prelude=True)
    dr.c_reset(f"{tag} (e) tsdf_hip_reset")
    dr.step("chain", f"{tag} (e) the soup outlives tsdf_hip_reset", call="march_fetch")
    dr.step("chain", f"{tag} (e) the normals do not", call="march_fetch_normals")
    dr.look_at_list(f"{tag} (e) the list outlives tsdf_hip_reset")
    if single:
        dr.check_field(f"{tag} (e) the field does not")
    dr.step("host", f"{tag} (e) one frame", count=True, pipelined=False)
    small = dr.step("chain", f"{tag} (e) small", call="march", w_min=0.0)
    assert 300 < small < large, (small, large)
    dr.step("chain", f"{tag} (e) small", call="march_fetch")
    mk = dr.step("chain", f"{tag} (e) small", call="march_flatten")
    dr.step("chain", f"{tag} (e) small", call="march_normals")
    assert dr.step("chain", f"{tag} (e) small", call="march_fetch_indexed") == mk
    dr.step("chain", f"{tag} (e) small", call="march_fetch_normals")
    box = (dr.res // 4, dr.res // 4, dr.res // 2 - 3, dr.res // 3, dr.res // 2, 6)
    assert 0 < dr.keep_list(f"{tag} (e) a small box", box) < n_list
    if single:
        f = dr.step("esdf", f"{tag} (e) a small box", args=(6, 0.0, box), prelude=True)
        assert f["d2"].size < dr.res ** 3
    for k in range(2):
        dr.step("host", f"{tag} (e) frame {k} more", count=False, pipelined=False)
    again = dr.step("chain", f"{tag} (e) large again", call="march", w_min=0.0)
    assert again > small
    dr.step("chain", f"{tag} (e) large again", call="march_fetch")
    assert dr.step("chain", f"{tag} (e) large again", call="march_decimate")[1] > 300
    dr.step("chain", f"{tag} (e) large again", call="march_normals")
    dr.step("chain", f"{tag} (e) large again", call="march_fetch_indexed")
    dr.step("chain", f"{tag} (e) large again", call="march_fetch_normals")
    assert dr.step("chain", f"{tag} (e) a cleanup ends the indexed mesh and the normals", call="march_cleanup") > 300
    for call in ("march_fetch_indexed", "march_smooth", "march_fetch_normals"):
        assert dr.step("chain", f"{tag} (e) after the cleanup", call=call) is INVALID
    assert dr.keep_list(f"{tag} (e) the whole grid again") > 1000
    if single:
        dr.step("esdf", f"{tag} (e) the whole grid again", args=(0, 1.0, None), prelude=True)
    dr.stale = None
    dr.quiet = False
    happened.add("e")
    return happened


def run_case(shape, res, color, seed, tmp_path, live=True):
    """One case, with or without the product: its Stats."""
    tag = f"{shape} {res} {'colour' if color else 'plain'} seed {seed}"
    dr = FeatureDriver(shape, res, color, seed, tmp_path, live=live)
    try:
        if seed == 0:
            happened = prelude(dr, tag)
            want = {c[0] for c in PRELUDE_CONDITIONS} if dr.single else {c[0] for c in SET_CONDITIONS}
            assert happened == want, happened
        dr.random_steps(STEPS, tag)
        dr.stats.rng_end.append(int(dr.rng.randint(1 << 30)))   # (the generator stands where the replay's stands)
    finally:
        dr.close()
    return dr.stats


def assert_all_floors(stats):
    for shape in SHAPES:
        single = SHAPES[shape] is None
        assert_floors(stats[shape], [o for o in OPERATIONS if single or o not in SINGLE_ONLY], single, shape)


@pytest.mark.parametrize("shape,res,color,seed", CASES, ids=IDS)
def test_feature_sequences_equal_the_models_after_every_step(gpu, tmp_path, shape, res, color, seed):
    t0 = time.perf_counter()
    stats = run_case(shape, res, color, seed, tmp_path)
    replayed = run_case(shape, res, color, seed, tmp_path, live=False)   # what the CPU tier asserts its floors on is this very sequence
    assert replayed.__dict__ == stats.__dict__, (replayed.summary(), stats.summary())
    STATS[shape].add(stats)
    RAN.add((shape, res, color, seed))
    tag = IDS[CASES.index((shape, res, color, seed))]
    SECONDS[tag] = time.perf_counter() - t0
    print(f"{tag}: {SECONDS[tag]:.1f} s; {stats.summary()}")


def test_every_operation_and_chain_call_occurred_on_inputs_that_count(gpu):
    """The floors of tests/feature_cases.assert_floors on what really ran (this test needs the sequence tests above to have
    run in this process: run the file as a whole)."""
    assert RAN == set(CASES), f"{len(set(CASES) - RAN)} sequence cases did not finish in this run"
    assert_all_floors(STATS)
    for shape in SHAPES:
        print(shape, STATS[shape].summary())
    print({k: round(v, 1) for k, v in SECONDS.items()}, "slowest", max(SECONDS.values()))
