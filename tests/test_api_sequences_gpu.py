"""GPU tier: random sequences of API calls on one handle and on a three-slab set (setDevices([0, 0, 0])), checked after
EVERY step against the plain model of tests/sequence_model.py -- what one call leaves behind for the next: the band flags
and the implied-distance record, a frame held back by frame pairing, the occupied list, the halo planes of a set and the
slabs' own copies of all of that.

Every (shape, grid) starts with a scripted prelude that makes the coincidences happen which random draws alone do not
guarantee (PRELUDE_CONDITIONS), with parameters under which the band flags and the implied distances are in use; the other
seeds draw their parameters and run random steps only.  A module-level tally of the operations is checked by the last test
of the file, so the file is meant to be run as a whole.

The set's bookkeeping (per-slab launch timing on the paired paths, tsdf_hip_last_read_detail after a counting pair) has
its tests at the end."""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, backproject
from tests import align_cases, flatten_cases
from tests.common import assert_same_f32, make_volume
from tests.sequence_model import Model, assert_same_mesh, compare, draw_shift, record_for, slab_starts  # noqa: F401
from tests.test_fused2_gpu import device_frame
from tests.test_implied_d_gpu import holes, open_scene, read_detail
from tests.test_occupied_gpu import check as check_occupied

pytestmark = pytest.mark.gpu

SET = [0, 0, 0]
SHAPES = {"one_handle": None, "set_0_0_0": SET}
# (grid, colour, seeds): seed 0 of every grid is the prelude
GRIDS = [(64, True, 8), (64, False, 8), (128, True, 2)]
CASES = [(shape, res, color, seed) for shape in SHAPES for res, color, n in GRIDS for seed in range(n)]
IDS = [f"{shape}-{res}-{'colour' if color else 'plain'}-seed{seed}" for shape, res, color, seed in CASES]
STEPS = 20
N_FRAMES = 40
PRELUDE_CONDITIONS = ("a: z shift past a slab with the flags carried, then a march through the flags and an integrate with implied distances",
                      "b: a pair fused on every slab", "c: a held-back ring frame flushed by a shift and by a reader",
                      "d: renderView straight after an upload that changed a halo plane's owner")
MUTATING = ["host", "host", "device", "pair", "staged", "ring", "shift", "shift", "upload", "upload", "set_planes", "device_planes",
            "save_load", "reset"]
READING = ["mesh", "mesh", "occupied", "render", "render", "sample", "align"]
SINGLE_ONLY = ("set_planes", "device_planes")
TALLY = {shape: collections.Counter() for shape in SHAPES}
RAN, SECONDS = set(), {}


def march_stats(vol):
    st = (C.c_uint64 * 4)()
    capi.check(capi.load().tsdf_hip_march_stats(vol._need(), st), "march_stats")
    return [int(v) for v in st]


def kernel_launches(vol):
    """(launches, milliseconds) per slab since the last read (tsdf_hip_multi_kernel_ms)."""
    out = []
    for k in range(len(vol.slabs())):
        ms, cnt = C.c_float(0), C.c_int32(0)
        capi.check(capi.load().tsdf_hip_multi_kernel_ms(vol._need(), k, C.byref(ms), C.byref(cnt)), "multi_kernel_ms")
        out.append((cnt.value, ms.value))
    return out


class Driver:
    """One volume and its model; every operation acts on both and checks what the call itself returns."""

    def __init__(self, shape, res, color, seed, tmp_path, draw_parameters):
        self.rng = rng = np.random.RandomState(9000 + 100 * res + 10 * int(color) + seed)
        self.shape, self.res, self.color, self.tmp_path = shape, res, color, tmp_path
        wmax, trunc, layout = 100.0, (0.03, 0.03), capi.LAYOUT_AUTO
        if draw_parameters:
            wmax = float(rng.choice([100.0, 4.0, 2.5, 255.0]))           # 2.5: a non-integer limit -- no implied distances, no PACKED
            trunc = [(0.03, 0.03), (0.05, 0.02), (0.01, 0.03)][rng.randint(3)]   # 0.01 / 0.03: the hinge identity fails
            layout = capi.LAYOUT_F32W if rng.rand() < 0.15 else capi.LAYOUT_AUTO
        self.vol, sc = make_volume(res, color=color, max_weight=wmax, trunc=trunc)
        self.vol.setLayout(layout)
        self.single = SHAPES[shape] is None
        if not self.single:
            self.vol.setDevices(SHAPES[shape])
        self.sc = open_scene(sc)
        self.vol.reset()
        self.model = Model(self.vol._p)
        self.packed = self.vol.getLayout() == capi.LAYOUT_PACKED
        self.rec = record_for(self.packed, trunc, wmax) if self.single else None
        self.starts = slab_starts(res)
        self.thick = max(b - a for a, b in zip(self.starts, self.starts[1:]))
        if not self.single:
            assert [s[1] for s in self.vol.slabs()] == self.starts[:3]
        self.voxel = self.sc.size / res
        self.frame_no, self.keep, self.cum = 0, [], [0, 0, 0]
        self.pairing, self.held = False, False
        self.stale = None   # single handle: (idx of an occupied list, whether a later step invalidated it)
        self.lib = capi.load()

    mutating, tally = MUTATING, TALLY   # (what a subclass with other operations replaces)

    def compare(self, what):
        compare(self.vol, self.model.ov, what)

    def close(self):
        self.vol.close()

    # ---- helpers -------------------------------------------------------------------------------------------------------
    def next_frame(self):
        i = self.frame_no
        self.frame_no += 1
        tr = synth.turntable_pose(i % N_FRAMES, N_FRAMES, self.sc.size, tilt=0.2 * np.sin(i))
        dep, col = holes(self.sc.depth(tr, noise_seed=900 + i), i), self.sc.bgra(i)
        return self.model.pose(tr), dep, (col if self.color else None)

    def launched(self, n_launches=1, fused=False):
        """The record after flag-keeping launches; returns whether the last one may rebuild distances from counts."""
        if not self.single:
            return None
        allowed = False
        for _ in range(n_launches):
            allowed = self.rec.fast_launch()
        return False if fused else allowed   # (k_integrate2 keeps the record but reads every distance itself)

    def check_detail(self, allowed, what, counted=False):
        if not self.single:
            return
        self.vol.synchronize()
        skipped, on = read_detail(self.vol)
        assert on == int(allowed), (what, on, allowed, self.rec.__dict__)
        if counted and not allowed:
            assert skipped == 0, (what, skipped)

    def before(self, op):
        """What any call but a ring frame does first: it launches a frame held back for pairing."""
        self.held = False

    def after(self, op):
        if self.pairing and op != "ring":   # pairing ends with the operation that followed the ring frames
            self.vol.setFramePairing(False)
            self.pairing = False

    # ---- mutating operations ----------------------------------------------------------------------------------------------
    def op_host(self, what, count=None, pipelined=None):
        T, dep, col = self.next_frame()
        want = self.model.integrate(dep, col, T)
        count = bool(self.rng.randint(2)) if count is None else count
        # (with pairing still on, a pipelined frame would be one more ring frame: the frame after the ring is synchronous)
        pipelined = (bool(self.rng.randint(2)) if pipelined is None else pipelined) and not count and not self.pairing
        n = self.vol.integrateCloud(dep, col, T, count=count, pipelined=pipelined)
        if count:
            assert n == want, (what, n, want)
        self.check_detail(self.launched(), what, count)
        return want

    def op_device(self, what):
        T, dep, col = self.next_frame()
        want = self.model.integrate(dep, col, T)
        t = device_frame(dep, col)
        torch.cuda.synchronize()
        self.keep.append(t)
        count = bool(self.rng.randint(2))
        n = self.vol.integrateCloudDevice(t[0].data_ptr(), t[1].data_ptr() if self.color else 0, T, count=count)
        if count:
            assert n == want, (what, n, want)
        self.check_detail(self.launched(), what, count)

    def op_pair(self, what):
        pair, want = [], []
        for _ in range(2):
            T, dep, col = self.next_frame()
            t = device_frame(dep, col)
            self.keep.append(t)
            pair.append((t[0].data_ptr(), t[1].data_ptr() if self.color else 0, T))
            want.append(self.model.integrate(dep, col, T))
        torch.cuda.synchronize()
        fused, counts = self.vol.integrateCloudDevice2(pair[0], pair[1], count=True)
        assert counts == want, (what, counts, want)
        if self.single:
            self.check_detail(self.launched(1 if fused else 2, fused), what)
        elif fused:
            assert read_detail(self.vol) == (0, 0), what   # every slab swept once and read every distance word
        return fused

    def op_staged(self, what):
        T, dep, col = self.next_frame()
        keep = ~np.isnan(dep)
        xyz = backproject(dep, self.sc.fx, self.sc.fy, self.sc.cx, self.sc.cy)
        pts_col = np.ascontiguousarray(col[keep]) if self.color else None
        d_ref, c_ref, n_ref = self.model.ov.organize(xyz, pts_col)
        d_gpu, c_gpu, n_gpu = self.vol.organize(xyz, pts_col)
        assert n_gpu == n_ref, (what, n_gpu, n_ref)
        assert_same_f32(d_gpu, d_ref, f"organised depth {what}")
        if self.color:
            filled = np.isfinite(d_ref)
            assert np.array_equal(c_gpu[filled], c_ref[filled]), what
        want = self.model.integrate(d_ref, c_ref if self.color else None, T)
        count = bool(self.rng.randint(2))
        n = self.vol.integrateStaged(T, count=count)
        if count:
            assert n == want, (what, n, want)
        self.check_detail(self.launched(), what, count)

    def op_ring(self, what, n=None):
        """setFramePairing(True) and one to three frames through the ring; an odd frame waits for whatever comes next."""
        self.vol.setFramePairing(True)
        self.pairing = True
        for _ in range(int(self.rng.randint(1, 4)) if n is None else n):
            T, dep, col = self.next_frame()
            self.model.integrate(dep, col, T)
            self.vol.integrateCloud(dep, col, T, pipelined=True)
            self.launched()   # (when it is launched, no foreign write can have come in between: every call launches it first)
            self.held = not self.held

    def draw_shift(self):
        return draw_shift(self.rng, self.cum, self.thick)

    def op_shift(self, what, s=None):
        s = self.draw_shift() if s is None else s
        moved = self.vol.shiftVolume(*s)
        self.model.shift(s, moved)
        self.cum = [c + v for c, v in zip(self.cum, s)]
        if any(s):
            carried = self.vol.shiftStats()[2]
            if self.single:
                self.rec.shift()
                assert carried == int(self.rec.flags_describe_planes), (what, s, carried)
            if self.stale:
                self.stale = (self.stale[0], True)
        return s

    def seam_box(self, seam=None):
        """A box with non-zero x0 / y0 / z0 whose z range crosses a slab seam of the three-slab partition."""
        rng, res = self.rng, self.res
        seam = self.starts[1 + rng.randint(2)] if seam is None else seam
        z0 = seam - int(rng.randint(1, 4))
        nz = seam - z0 + int(rng.randint(1, 4))
        x0, y0 = int(rng.randint(1, res // 4)), int(rng.randint(1, res // 4))
        nx, ny = int(rng.randint(res // 2, res - x0 + 1)), int(rng.randint(res // 2, res - y0 + 1))
        return x0, y0, z0, nx, ny, nz

    def op_upload(self, what, box=None, which=None):
        x0, y0, z0, nx, ny, nz = self.seam_box() if box is None else box
        d, w, rgb = (a.copy() if a is not None else None for a in self.model.box(x0, y0, z0, nx, ny, nz))
        seen = w > 0
        which = ["d", "w", "all"][self.rng.randint(3)] if which is None else which
        if which in ("d", "all"):   # the surface moves, and free space leaves the hinge value: only reading it can tell
            d[seen] = np.maximum(d[seen] - np.float32(0.125), np.float32(-1.0))
        if which in ("w", "all"):
            w = np.floor(w * np.float32(0.5))
        if which == "all" and rgb is not None:
            rgb = 255 - rgb
        args = dict(d=d if which != "w" else None, w=w if which != "d" else None, rgb=rgb if which == "all" else None)
        self.vol.upload(x0=x0, y0=y0, z0=z0, **args)
        self.model.upload(x0=x0, y0=y0, z0=z0, **args)
        if self.single:
            self.rec.foreign_write()
        return int(seen.sum())

    def op_set_planes(self, what):
        vol, res, ov = self.vol, self.res, self.model.ov
        z0, nz = int(self.rng.randint(res - 4)), int(self.rng.randint(1, 4))
        dev = torch.device("cuda", 0)
        dt = torch.empty((nz, res, res), dtype=torch.float32, device=dev)
        wt = torch.empty_like(dt)
        ct = torch.empty((nz, res, res), dtype=torch.int32, device=dev) if self.color else None
        args = (C.c_void_p(dt.data_ptr()), C.c_void_p(wt.data_ptr()), C.c_void_p(ct.data_ptr()) if self.color else None)
        capi.check(self.lib.tsdf_hip_get_planes_device(vol._need(), z0, nz, *args), "get_planes_device")
        vol.synchronize()
        sel = (wt > 0) & (dt > 0)
        if bool(sel.any()):
            idx = torch.nonzero(sel)[0]
            dt[idx[0], idx[1], idx[2]] = -0.5
            ov.d[z0 + int(idx[0]), int(idx[1]), int(idx[2])] = np.float32(-0.5)
        torch.cuda.synchronize()
        capi.check(self.lib.tsdf_hip_set_planes_device(vol._need(), z0, nz, *args), "set_planes_device")
        self.rec.foreign_write()

    def op_device_planes(self, what):
        self.vol.device_planes()   # raw pointers handed out: the caller may write through them
        self.rec.foreign_write()

    def op_save_load(self, what):
        path = str(self.tmp_path / f"{what.replace(' ', '_')}.vol")
        self.vol.save(path)
        self.vol.load(path)
        assert np.array_equal(self.vol.getGlobalTransform(), self.model.G), what
        if self.single:
            self.rec.reset()
            self.rec.foreign_write()   # a loaded volume holds whatever the file held
        if self.stale:
            self.stale = (self.stale[0], True)   # a new handle: no list yet

    def op_reset(self, what):
        self.vol.reset()
        self.model.reset()
        if self.single:
            self.rec.reset()
        if self.stale:
            self.stale = (self.stale[0], True)

    # ---- reading operations -----------------------------------------------------------------------------------------------
    def op_mesh(self, what, w_min=None, cleanup=None, flatten=None, extras=True):
        rng = self.rng
        w_min = float(rng.choice([0.0, 1.0, 2.5])) if w_min is None else w_min
        if extras and rng.rand() < (0.3 if self.res <= 64 else 0.15):
            cleanup = (1.5 * self.voxel, int(rng.choice([3, 40])))
        if extras and rng.rand() < (0.3 if self.res <= 64 else 0.15):
            flatten = flatten_cases.MD
        mc = MarchingCubesTSDFOctree()
        mc.setInputTSDF(self.vol)
        mc.setMinWeight(w_min)
        mc.setColorByRGB(self.color)
        if cleanup:
            mc.setCleanup(*cleanup)
        if flatten:
            mc.setFlatten(flatten)
        got = mc.reconstruct(want_cells=True)
        st = march_stats(self.vol)
        assert_same_mesh(got, self.model.mesh(w_min, cleanup, flatten), f"{what} w_min {w_min} cleanup {cleanup} flatten {flatten}")
        if self.single and not self.rec.flags_describe_planes:
            assert st[3] & 1 == 0, (what, st)   # after a foreign write the flags decide nothing
        return got, st

    def op_occupied(self, what):
        check_occupied(self.vol, self.model.occupied(), what=what)
        box = self.seam_box()
        check_occupied(self.vol, self.model.occupied(box), box=box, what=f"{what} box {box}")

    def look_at(self, target=None, direction=None):
        rng, S = self.rng, self.sc.size
        v = rng.normal(size=3) if direction is None else np.asarray(direction, np.float64)
        v[1] *= 0.3   # (the camera's down axis is y: stay away from looking along it)
        eye = 2.2 * S * v / np.linalg.norm(v)
        target = rng.uniform(-0.1, 0.1, 3) * S if target is None else np.asarray(target)
        return synth.look_at_pose(eye + target, target=target)

    def op_render(self, what, trans=None, ds=None):
        trans = self.look_at() if trans is None else trans
        ds = int(self.rng.choice([1, 2, 3])) if ds is None else ds
        got, want = self.vol.renderView(trans, ds, camera_frame=False), self.model.raycast(trans, ds)
        assert got.shape == want.shape == (120 // ds, 160 // ds, 8), what
        hit = np.isfinite(want[..., 0])
        assert np.array_equal(np.isfinite(got[..., 0]), hit), f"{what} ds {ds}: hit mask"
        self.assert_same_hits(got[hit], want[hit], f"{what} ds {ds}: hits")
        return got, int(hit.sum())

    def assert_same_hits(self, got, want, what):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what

    def op_sample(self, what):
        rng, S = self.rng, self.sc.size
        pts = rng.uniform(-0.5 * S, 0.5 * S, (400, 3))
        seam = np.array(self.starts[1:3])[rng.randint(2, size=100)]   # a quarter within one voxel of a seam plane's centre
        pts[:100, 2] = (seam + 0.5 + rng.uniform(-1.0, 1.0, 100)) * self.voxel - 0.5 * S
        pts = pts.astype(np.float32)
        got, want = self.vol.sample(pts), self.model.sample(pts)
        ok = want[0]
        assert np.array_equal(got[0], ok), what
        for g, w_, name in zip(got[1:], want[1:], ("getFxn", "getGradient", "getHessian")):
            assert_same_f32(g[ok], w_[ok], f"{name} {what}")
        return int(ok.sum())

    def op_align(self, what):
        rng = self.rng
        tr = synth.turntable_pose(rng.uniform(0, N_FRAMES), N_FRAMES, self.sc.size, tilt=0.1)
        cloud = backproject(self.sc.depth(tr), self.sc.fx, self.sc.fy, self.sc.cx, self.sc.cy)
        pts = cloud[rng.choice(len(cloud), 1500, replace=False)] if len(cloud) > 1500 else cloud
        xi = np.concatenate([0.01 * rng.normal(size=3), self.voxel * rng.normal(size=3)])
        T = align_cases.se3_exp(xi) @ self.model.pose(tr)
        min_weight = float(rng.choice([0.0, 1.0]))
        want = self.model.alignment(self.vol, pts, T, min_weight, 0.9)
        out, used = self.vol.alignmentSystem(pts, T, min_weight, 0.9, want_used=True)
        assert np.array_equal(used, want["used"]), what
        align_cases.assert_system(out, want, what)   # out[28] exact, the sums within the bound of re-ordered fp64 summation

    # ---- the occupied list across mutating steps (single handle) ---------------------------------------------------------------
    def make_list(self):
        n = C.c_uint64(0)
        capi.check(self.lib.tsdf_hip_occupied(self.vol._need(), None, C.byref(n)), "occupied")
        self.stale = (self.model.occupied()[0].copy(), False)
        assert n.value == len(self.stale[0])

    def check_list(self, what):
        """include/tsdf_hip.h: a list names voxels by index, so a shift ends it (E_INVALID), and a new handle (reset, load) has
        none; after any other write it still names the same voxels and the fetch gathers what they hold NOW."""
        want_idx, ended = self.stale
        self.stale = None
        idx = np.empty((len(want_idx), 3), np.int32)
        d = np.empty(len(want_idx), np.float32)
        rc = self.lib.tsdf_hip_occupied_fetch(self.vol._need(), idx.ctypes.data_as(C.POINTER(C.c_int32)), capi.as_f32p(d), None, None)
        if ended:
            assert rc == capi.E_INVALID, (what, rc)
            return
        assert rc == capi.OK, (what, rc)
        assert np.array_equal(idx, want_idx), what
        assert_same_f32(d, self.model.ov.d[want_idx[:, 2], want_idx[:, 1], want_idx[:, 0]], f"values of the earlier list {what}")

    # ---- one step ---------------------------------------------------------------------------------------------------------
    def step(self, op, what, **kw):
        mutating = op in self.mutating
        if self.single and mutating and op != "ring" and not self.pairing and self.rng.rand() < 0.5:
            self.make_list()
        if op != "ring":
            self.before(op)
        out = getattr(self, "op_" + op)(what, **kw)
        self.after(op)
        self.tally[self.shape][op] += 1
        if self.stale and mutating:
            self.check_list(what)
        if not self.held:   # (download() is a call like any other: it would launch the frame that waits for the NEXT operation)
            self.compare(what)
        return out

    def random_steps(self, n, tag):
        ops = [o for o in MUTATING + READING if self.single or o not in SINGLE_ONLY]
        for k in range(n):
            op = ops[self.rng.randint(len(ops))]
            self.step(op, f"{tag} step {k} {op}")


def prelude(dr, tag):
    """The scripted start of every (shape, grid): returns the conditions that really happened."""
    vol, happened = dr.vol, set()
    assert dr.packed
    if not dr.single:
        capi.check(dr.lib.tsdf_hip_multi_timing(vol._need(), 1), "multi_timing")
    for k in range(3):
        dr.step("host", f"{tag} prelude frame {k}", count=(k == 2), pipelined=False)
    # (b) a pair that every slab sweeps once (without colour only with the knob that shares the sweep wherever it can)
    try:
        capi.set_tuning("fuse2", 2)
        assert dr.step("pair", f"{tag} prelude pair") is True
    finally:
        capi.set_tuning("fuse2", 1)
    happened.add("b")
    if not dr.single:
        assert [n for n, _ in kernel_launches(vol)] == [4, 4, 4]   # three frames and ONE sweep for the pair, on every slab
    # (c), (a): a ring frame waits; the z shift past a slab launches it first and carries the flags
    _, st = dr.step("mesh", f"{tag} prelude mesh", w_min=1.0, extras=False)   # (and the one-plane halo is fresh now)
    assert st[3] & 1 == 1, st
    dr.step("ring", f"{tag} prelude ring", n=1)
    assert dr.held
    if not dr.single:
        assert [n for n, _ in kernel_launches(vol)] == [0, 0, 0]
    s = (0, 0, dr.thick + 1)
    dr.step("shift", f"{tag} prelude shift", s=s)
    assert vol.shiftStats()[2] == 1
    if not dr.single:
        assert [n for n, _ in kernel_launches(vol)] == [1, 1, 1]
    got, st = dr.step("mesh", f"{tag} prelude mesh after the shift", w_min=1.0, extras=False)
    assert st[3] & 1 == 1 and len(got["cells"]) > 100, (st, len(got["cells"]))
    T, dep, col = dr.next_frame()
    want = dr.model.integrate(dep, col, T)
    assert vol.integrateCloud(dep, col, T, count=True) == want and want > 0
    dr.launched()
    assert read_detail(vol)[1] == 1   # implied distances on, on one handle and folded over the slabs of a set
    compare(vol, dr.model.ov, f"{tag} prelude frame after the shift")
    happened.add("a")
    dr.step("ring", f"{tag} prelude ring before a reader", n=1)
    assert dr.held
    if not dr.single:
        assert [n for n, _ in kernel_launches(vol)] == [1, 1, 1]   # (the counted frame above; the ring frame waits)
    assert dr.step("sample", f"{tag} prelude sample") > 100
    if not dr.single:
        assert [n for n, _ in kernel_launches(vol)] == [1, 1, 1]   # the reader launched it
        capi.check(dr.lib.tsdf_hip_multi_timing(vol._need(), 0), "multi_timing")
    happened.add("c")
    # the reader left plane z_end of every slab fresh, and no frame is waiting: a shift has to mark the halo stale itself
    dr.step("shift", f"{tag} prelude shift with a fresh halo", s=(1, 0, -2))
    assert dr.step("sample", f"{tag} prelude sample after the second shift") > 100
    got, _ = dr.step("mesh", f"{tag} prelude mesh after the second shift", w_min=0.0, extras=False)
    assert len(got["cells"]) > 100
    # (d) the whole halo fresh (renderView), an upload across the seam that the surface now crosses, renderView at once
    seam = dr.starts[1]
    trans = dr.look_at(target=-np.array(dr.cum) * dr.voxel, direction=(0.5, 0.3, 1.0))   # at the sphere's centre, from the seam's side
    before, hits = dr.step("render", f"{tag} prelude render", trans=trans, ds=1)
    box = (1, 2, seam - 2, dr.res - 2, dr.res - 4, 4)
    assert dr.step("upload", f"{tag} prelude upload", box=box, which="d") > 100
    after, _ = dr.step("render", f"{tag} prelude render after the upload", trans=trans, ds=1)
    assert hits > 100 and not np.array_equal(before.view(np.uint32), after.view(np.uint32))   # the rays do see the changed planes
    happened.add("d")
    return happened


@pytest.mark.parametrize("shape,res,color,seed", CASES, ids=IDS)
def test_api_sequences_equal_the_model_after_every_step(gpu, tmp_path, shape, res, color, seed):
    t0 = time.perf_counter()
    tag = f"{shape} {res} {'colour' if color else 'plain'} seed {seed}"
    dr = Driver(shape, res, color, seed, tmp_path, draw_parameters=seed > 0)
    try:
        if seed == 0:
            happened = prelude(dr, tag)
            assert happened == {c[0] for c in PRELUDE_CONDITIONS}, happened
        dr.random_steps(STEPS if res <= 64 else STEPS * 3 // 4, tag)
    finally:
        dr.close()
    RAN.add((shape, res, color, seed))
    SECONDS[tag] = time.perf_counter() - t0
    print(f"{tag}: {SECONDS[tag]:.1f} s")


def test_every_operation_occurred_in_the_sequences(gpu):
    """Over all seeds every operation ran at least five times on either shape (this test needs the sequence tests above to
    have run in this process: run the file as a whole)."""
    assert RAN == set(CASES), f"{len(set(CASES) - RAN)} sequence cases did not finish in this run"
    for shape in SHAPES:
        for op in set(MUTATING + READING):
            if SHAPES[shape] is not None and op in SINGLE_ONLY:
                continue   # a set refuses set_planes_device / device_planes
            assert TALLY[shape][op] >= 5, (shape, op, dict(TALLY[shape]))
    print({k: round(v, 1) for k, v in SECONDS.items()})


# ---- scripted reproductions and the set's bookkeeping ---------------------------------------------------------------------------
def paired_frames(sc, color, n):
    poses = [synth.turntable_pose(i, 12, sc.size, tilt=0.05 * i) for i in range(n)]
    frames = [device_frame(sc.depth(tr, noise_seed=500 + i), sc.bgra(i) if color else None) for i, tr in enumerate(poses)]
    torch.cuda.synchronize()
    return poses, frames


@pytest.mark.parametrize("color", [True, False], ids=["colour_pairs_fuse", "plain_pairs_do_not"])
def test_paired_paths_report_the_sweeps_every_slab_ran(gpu, color):
    """tsdf_hip_multi_timing / tsdf_hip_multi_kernel_ms on the paired paths: one launch per sweep a slab really ran -- 1 for
    a pair it fused (with colour, from the turntable, every slab does), 2 for one it did not (without colour the default
    leaves a pair to two launches), 1 for a frame launched on its own, none while a frame waits; milliseconds > 0."""
    vol, sc = make_volume(64, color=color)
    vol.setDevices(SET)
    vol.reset()
    lib, h = capi.load(), vol._need()
    poses, fr = paired_frames(sc, color, 8)
    ptr = lambda i: (fr[i][0].data_ptr(), fr[i][1].data_ptr() if color else 0, poses[i])  # noqa: E731
    per_pair = 1 if color else 2
    try:
        capi.check(lib.tsdf_hip_multi_timing(h, 1), "multi_timing")
        for k in range(3):   # n pairs
            fused, _ = vol.integrateCloudDevice2(ptr(2 * k), ptr(2 * k + 1), count=(k == 1))
            assert fused == color
        got = kernel_launches(vol)
        assert [n for n, _ in got] == [3 * per_pair] * 3 and all(ms > 0 for _, ms in got), got
        for i in (6, 7):     # the frame-by-frame path is unchanged
            vol.integrateCloudDevice(ptr(i)[0], ptr(i)[1], poses[i])
        got = kernel_launches(vol)
        assert [n for n, _ in got] == [2, 2, 2] and all(ms > 0 for _, ms in got), got
        vol.setFramePairing(True)   # host frames through every slab's ring: a pair, then a frame that waits
        for i in range(3):
            vol.integrateCloud(sc.depth(poses[i]), sc.bgra(i) if color else None, poses[i], pipelined=True)
        got = kernel_launches(vol)
        assert [n for n, _ in got] == [per_pair] * 3 and all(ms > 0 for _, ms in got), got
        vol.download(nz=1)          # any other call launches the frame that waited
        got = kernel_launches(vol)
        assert [n for n, _ in got] == [1, 1, 1] and all(ms > 0 for _, ms in got), got
        assert [n for n, _ in kernel_launches(vol)] == [0, 0, 0]   # read and forgotten
    finally:
        vol.close()


def test_last_read_detail_after_a_counting_pair_on_a_set(gpu):
    """A frame-by-frame counting launch with implied distances on, then a pair that every slab fuses: k_integrate2 reads every
    distance word, so tsdf_hip_last_read_detail reads (0, 0) as on one handle -- not the verdict of the earlier launch."""
    got = {}
    for name, devices in SHAPES.items():
        vol, sc = make_volume(64, color=True)
        vol.setDevices(devices)
        vol.reset()
        assert vol.getLayout() == capi.LAYOUT_PACKED
        sc = open_scene(sc)
        poses, fr = paired_frames(sc, True, 2)
        try:
            tr = synth.turntable_pose(5, 12, sc.size)
            for _ in range(2):
                assert vol.integrateCloud(sc.depth(tr), sc.bgra(0), tr, count=True) > 0
            first = read_detail(vol)
            assert first[1] == 1 and first[0] > 0, (name, first)
            fused, counts = vol.integrateCloudDevice2((fr[0][0].data_ptr(), fr[0][1].data_ptr(), poses[0]),
                                                      (fr[1][0].data_ptr(), fr[1][1].data_ptr(), poses[1]), count=True)
            assert fused and min(counts) > 0, (name, fused, counts)
            got[name] = read_detail(vol)
        finally:
            vol.close()
    assert got["one_handle"] == (0, 0) and got["set_0_0_0"] == (0, 0), got
