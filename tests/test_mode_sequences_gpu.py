"""GPU tier: random sequences of API calls on volumes of the SECOND integrate family -- setColorMode("RGBNormalized"),
setColorMode("LAB"), setWeighting(by_depth, by_variance) -- on one handle and on a three-slab set, checked after EVERY step
against the plain model of tests/sequence_model.py: d, w, rgb, and the state these modes keep besides (the float colour
planes cn[], M and nsample), which a shift, a pull between slabs, an upload, a reset or a save/load can lose without the
volume looking wrong until a later frame is integrated.

The Driver is the one of tests/test_api_sequences_gpu.py; ModeDriver replaces what differs (the frames, the compare, the
operations that are other calls here).  The cases, their frames and their plans come from tests/mode_cases.py, which the
CPU tier replays through the model alone (tests/test_sequence_model.py): conditions and tally are known before this file
runs, and are checked again here from what really ran.  Grids: 64^3 (save/load; slabs of 22, 21, 21 planes) and
70 x 36 x 45 (pitch 72 != nx, a partial second flag cell in x, ny no multiple of the 4-row cell, 15-plane slabs).

The module-level tally is checked by test_every_legal_operation_ran_in_every_mode: run the file as a whole."""
import collections
import ctypes as C
import time
import warnings

import numpy as np
import pytest
import torch  # noqa: F401

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, NonCubicQueryWarning
from tests import mode_cases
from tests.common import assert_same_f32, make_volume
from tests.evidence.fuzz_product_colour_modes import oracle_colours
from tests.mode_cases import CASES, COLOUR_MODES, SHAPES, case_id
from tests.sequence_model import Model, Record, compare
from tests.test_api_sequences_gpu import Driver, march_stats
from tests.test_lab_gpu import assert_bytes_equal
from tests.test_occupied_gpu import check as check_occupied

pytestmark = pytest.mark.gpu

TALLY = {(c.mode, c.shape): collections.Counter() for c in CASES}
RAN, SECONDS, COUNTS = set(), {}, {}
I32P = C.POINTER(C.c_int32)


def variance_state(vol, box=None):
    """(M, nsample) of a box (default: the whole grid) through the C entry point; works on a set too."""
    rx, ry, rz = vol._p.res
    x0, y0, z0, nx, ny, nz = box or (0, 0, 0, rx, ry, rz)
    M, ns = np.empty((nz, ny, nx), np.float32), np.empty((nz, ny, nx), np.int32)
    capi.check(capi.load().tsdf_hip_download_variance_state(vol._need(), x0, y0, z0, nx, ny, nz, capi.as_f32p(M), ns.ctypes.data_as(I32P)),
               "download_variance_state")
    return M, ns


def compare_all(vol, model, what, single):
    """d, w, rgb bit for bit (LAB bytes as tests/test_lab_gpu.py compares them: equal); M / nsample on both shapes; the float
    colour state where it can be read (tsdf_hip_download_color_state is single-handle only)."""
    ov = model.ov
    d, w, rgb = vol.download()
    assert_same_f32(d, ov.d, f"d {what}")
    assert_same_f32(w, ov.w, f"w {what}")
    if ov.rgb is not None:
        assert_bytes_equal(rgb, ov.rgb, f"rgb {what}")
    if getattr(ov, "M", None) is not None:
        M, ns = variance_state(vol)
        assert_same_f32(M, ov.M, f"M {what}")
        assert np.array_equal(ns, ov.nsample), f"nsample {what}: {int((ns != ov.nsample).sum())} voxels differ"
    if hasattr(ov, "cn") and single:
        state = vol.downloadColorState()
        assert state.shape == ov.cn.shape, what
        for k in range(len(state)):
            assert_same_f32(state[k], ov.cn[k], f"cn[{k}] {what}")


class ModeDriver(Driver):
    mutating = mode_cases.MUTATING

    def __init__(self, case, tmp_path):
        self.case, self.setup = case, mode_cases.Setup(case)
        su = self.setup
        self.rng = np.random.RandomState(mode_cases.case_seed(case) + 2)   # what the plan leaves open: entry-point variants, readers
        self.shape, self.tmp_path, self.color = case.shape, tmp_path, case.color
        self.tally = {case.shape: TALLY[case.mode, case.shape]}
        self.res3, self.res = su.res3, su.res3[0]
        self.vol = su.product()
        self.vol.reset()
        assert self.vol.getLayout() == capi.LAYOUT_F32W
        self.single = SHAPES[case.shape] is None
        self.sc = su.sc
        self.model = mode_cases.TwinModel(su, self.vol._p)
        self.packed = False
        self.rec = Record(False, False, 0) if self.single else None   # (the plain kernels keep no flags: every launch is a foreign write)
        self.flags_gone = False
        self.starts, self.thick = su.starts, su.thick
        if not self.single:
            assert [s[1] for s in self.vol.slabs()] == self.starts[:3]
        self.voxel = float(self.vol._p.size[0]) / self.res
        self.frame_no, self.keep, self.cum = 0, [], [0, 0, 0]
        self.pairing, self.held, self.stale = False, False, None
        self.lib = capi.load()

    def compare(self, what):
        compare_all(self.vol, self.model, what, self.single)

    def plain_volume(self):
        """An empty 32^3 volume of the first family (TSDF_COLOR_RGB, no weighting), F32W with the case's truncation limits and
        max_weight: only the mode stands between it and a merge with the case's volume."""
        if getattr(self, "other", None) is None:
            self.other, _ = make_volume(32, mode_cases.W, mode_cases.H, color=self.color, trunc=self.setup.trunc, max_weight=self.setup.wmax)
            self.other.setLayout(capi.LAYOUT_F32W)
            self.other.reset()
        return self.other

    def close(self):
        super().close()
        if getattr(self, "other", None) is not None:
            self.other.close()

    def next_frame(self):
        tr, dep, col = self.setup.frame(self.frame_no)
        self.frame_no += 1
        return self.model.pose(tr), dep, (col if self.color else None)

    def launched(self, n_launches=1, fused=False):
        self.flags_gone = True
        if not self.single:
            return None
        self.rec.foreign_write()
        return False

    def assert_no_flags(self, what):
        """After a plain-kernel launch (an upload, a load) no reader may trust the band flags."""
        if self.flags_gone:
            assert self.vol.occupiedStats()[2] == 0, (what, self.vol.occupiedStats())

    # ---- mutating operations that are other calls here ---------------------------------------------------------------------------
    def op_upload(self, what, box, which):
        e = dict(box=box, which=which)
        d, w = mode_cases.upload_arrays(self.model, e)
        self.vol.upload(d=d, w=w, x0=box[0], y0=box[1], z0=box[2])
        self.model.upload(d=d, w=w, x0=box[0], y0=box[1], z0=box[2])
        self.flags_gone = True
        if self.single:
            self.rec.foreign_write()

    def op_upload_variance(self, what, box, which, seed):
        M, ns = mode_cases.variance_arrays(dict(box=box, which=which, seed=seed))
        capi.check(self.lib.tsdf_hip_upload_variance_state(self.vol._need(), *box, capi.as_f32p(M) if M is not None else None,
                                                           ns.ctypes.data_as(I32P) if ns is not None else None), "upload_variance_state")
        self.model.upload_variance(M, ns, box)
        gM, gns = variance_state(self.vol, box)   # the box read back through the same seam
        wM, wns = self.model.variance_box(box)
        assert_same_f32(gM, wM, f"M of the box {what}")
        assert np.array_equal(gns, wns), f"nsample of the box {what}"

    def op_save_load(self, what):
        super().op_save_load(what)
        mode = self.case.mode
        assert self.vol._weighting == ("by_depth" in mode, "by_variance" in mode), (what, self.vol._weighting)
        self.flags_gone = True

    def op_reset(self, what):
        """reset() keeps the weighting: the class's reset (a new handle) or, on even seeds, tsdf_hip_reset on the handle that
        holds the state planes."""
        if self.case.seed % 2 == 0:
            capi.check(self.lib.tsdf_hip_reset(self.vol._need()), "reset")
            self.model.reset()
            if self.single:
                self.rec.reset()   # (the handle, and a list made on it, live on: the list names the same voxels)
        else:
            super().op_reset(what)
        self.flags_gone = False

    def op_refused(self, what):
        """Calls the mode refuses, with the documented code; step() then finds nothing changed (compare: d, w, rgb and the
        state planes)."""
        lib, h, UNSUPPORTED = self.lib, self.vol._need(), capi.E_UNSUPPORTED
        # every mode, weighted or RGB_NORMALIZED / LAB, on either shape: no frame is taken back out, nothing is merged in or out
        tr, dep, col = self.setup.frame(self.frame_no)   # (looked at, not consumed: the plan's frames stay the replay's)
        T, col = self.model.pose(tr), (col if self.color else None)
        other = self.plain_volume()
        for name, call in (("deintegrateCloud", lambda: self.vol.deintegrateCloud(dep, col, T, count=True)),
                           ("mergeVolume as dst", lambda: self.vol.mergeVolume(other, np.eye(4), 0.0, count=True)),
                           ("mergeVolume as src", lambda: other.mergeVolume(self.vol, np.eye(4), 0.0, count=True))):
            with pytest.raises(capi.TsdfHipError) as err:
                call()
            assert err.value.code == UNSUPPORTED, (what, name, err.value.code)
        assert not any(a.any() for a in other.download()[1:] if a is not None), f"{what}: the other volume of the refused merges"
        if self.case.mode in COLOUR_MODES:
            rgb = np.full((2, 3, 4, 3), 200, np.uint8)
            assert lib.tsdf_hip_upload(h, 1, 1, self.starts[1] - 1, 4, 3, 2, None, None, capi.as_u8p(rgb)) == UNSUPPORTED, what
            with pytest.raises(capi.TsdfHipError) as err:
                self.vol.save(str(self.tmp_path / "refused.vol"))
            assert err.value.code == UNSUPPORTED, what
            n = C.c_uint64(0)
            capi.check(lib.tsdf_hip_occupied(h, None, C.byref(n)), "occupied")
            idx, col = np.empty((max(1, n.value), 3), np.int32), np.empty((max(1, n.value), 3), np.uint8)
            assert lib.tsdf_hip_occupied_fetch(h, idx.ctypes.data_as(I32P), None, None, capi.as_u8p(col)) == UNSUPPORTED, what
            for flags in ((1, 0), (0, 1), (1, 1)):
                assert lib.tsdf_hip_set_weighting(h, *flags) == UNSUPPORTED, (what, flags)
        if not self.single:
            out = np.empty(self.res3[0] * self.res3[1], np.float32)
            assert lib.tsdf_hip_download_color_state(h, 0, 0, 1, capi.as_f32p(out)) == UNSUPPORTED, what

    # ---- reading operations -----------------------------------------------------------------------------------------------
    def op_occupied(self, what):
        rgb = self.case.mode not in COLOUR_MODES   # (their exact bytes need the host's pow: the fetch refuses rgb)
        check_occupied(self.vol, self.model.occupied(), rgb=rgb, what=what)
        self.assert_no_flags(what)
        box = self.setup.seam_box(self.rng)
        check_occupied(self.vol, self.model.occupied(box), box=box, rgb=rgb, what=f"{what} box {box}")
        self.assert_no_flags(what)

    def op_render(self, what, trans=None, ds=None):
        trans = self.look_at() if trans is None else trans
        ds = int(self.rng.choice([1, 2, 3])) if ds is None else ds
        out = super().op_render(what, trans, ds)
        if self.color:
            cloud, crgb = self.vol.renderColoredView(trans, ds)
            assert np.array_equal(crgb, oracle_colours(self.model.ov, cloud, trans)), f"{what} ds {ds}: renderColoredView"
        return out

    def assert_same_hits(self, got, want, what):
        """The variance weighting can give an observation the weight 0, and a voxel first seen that way d = 0 / 0: the normals
        next to it are NaN, whose sign and payload no one specifies.  Bit for bit everywhere else, as for d itself."""
        assert_same_f32(got, want, what)

    def op_sample(self, what):
        rng, size3 = self.rng, np.array([float(v) for v in self.vol._p.size])
        pts = rng.uniform(-0.5, 0.5, (400, 3)) * size3
        seam = np.array(self.starts[1:3])[rng.randint(2, size=100)]   # a quarter within one voxel of a seam plane's centre
        pts[:100, 2] = (seam + 0.5 + rng.uniform(-1.0, 1.0, 100)) * self.voxel - 0.5 * size3[2]
        pts = pts.astype(np.float32)
        got, want = self.vol.sample(pts), self.model.sample(pts)
        ok = want[0]
        assert np.array_equal(got[0], ok), what
        for g, w_, name in zip(got[1:], want[1:], ("getFxn", "getGradient", "getHessian")):
            assert_same_f32(g[ok], w_[ok], f"{name} {what}")
        return int(ok.sum())

    def run_plan(self, tag):
        for k, e in enumerate(self.setup.plan):
            kw = {k_: v for k_, v in e.items() if k_ != "op"}
            self.step(e["op"], f"{tag} step {k} {e['op']} {kw if e['op'] != 'upload_variance' else ''}", **kw)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_mode_sequences_equal_the_model_after_every_step(gpu, tmp_path, case):
    t0 = time.perf_counter()
    tag = case_id(case)
    dr = ModeDriver(case, tmp_path)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", NonCubicQueryWarning)   # (the flat grid: the queries answer for its own geometry)
            dr.run_plan(tag)
        assert not dr.held
        planned = sum(mode_cases.FRAME_OPS.get(e["op"], e.get("n", 0)) for e in dr.setup.plan)
        assert dr.frame_no == planned, (dr.frame_no, planned)   # the frames mode_cases.replay integrates, no more and no fewer
        COUNTS[tag] = dr.model.assert_conditions(tag)   # tests/mode_cases.CONDITIONS, from the model the product just equalled
    finally:
        dr.close()
    RAN.add(case)
    SECONDS[tag] = time.perf_counter() - t0
    print(f"{tag}: {SECONDS[tag]:.1f} s, {dr.frame_no} frames, wmax {dr.setup.wmax}, {COUNTS[tag]}")


def test_every_legal_operation_ran_in_every_mode(gpu):
    """All cases ran, the operations that ran are the plans' (which tests/test_sequence_model.py replays on the CPU), and
    every operation legal in a mode ran at least three times in that mode on each shape, the two ending frames not counted
    (this test needs the sequence tests above to have run in this process: run the file as a whole)."""
    assert RAN == set(CASES), f"{len(set(CASES) - RAN)} sequence cases did not finish in this run"
    planned = {key: collections.Counter() for key in TALLY}
    for c in CASES:
        for e in mode_cases.Setup(c).plan:
            planned[c.mode, c.shape][e["op"]] += 1
    assert {k: dict(v) for k, v in TALLY.items()} == {k: dict(v) for k, v in planned.items()}
    for (mode, shape), t in TALLY.items():
        mine = [c for c in CASES if (c.mode, c.shape) == (mode, shape)]
        for op in set().union(*[mode_cases.legal_ops(c) for c in mine]):
            assert t[op] - (2 * len(mine) if op == "host" else 0) >= 3, (mode, shape, op, dict(t))
        print(mode, shape, dict(t))
    print({k: round(v, 1) for k, v in SECONDS.items()})


# ---- scripted steps ---------------------------------------------------------------------------------------------------------------
def test_by_depth_toggle_on_an_f32w_rgb_handle(gpu):
    """tsdf_hip_set_weighting(h, 1, 0), a frame, tsdf_hip_set_weighting(h, 0, 0), a frame: the model after both; the plain
    launch of the first frame ends the band flags for every reader (tsdf_hip_march_stats out[3] bit 0, occupiedStats()[2])."""
    vol, sc = make_volume(64, color=True)
    vol.setLayout(capi.LAYOUT_F32W)
    vol.reset()
    lib, h = capi.load(), vol._need()
    model = Model(vol._p)
    try:
        for k, (flag, mode) in enumerate(((1, "by_depth"), (0, None))):
            capi.check(lib.tsdf_hip_set_weighting(h, flag, 0), "set_weighting")
            model.mode = mode
            tr = synth.turntable_pose(k, 8, sc.size)
            dep, col = sc.depth(tr, noise_seed=70 + k), sc.bgra(k)
            assert vol.integrateCloud(dep, col, tr, count=True) == model.integrate(dep, col, tr) > 0
            compare(vol, model.ov, f"frame {k}, weight_by_depth {flag}")
            mc = MarchingCubesTSDFOctree()
            mc.setInputTSDF(vol)
            mc.setMinWeight(0.5)
            mc.setColorByRGB(True)
            mesh = mc.reconstruct(want_cells=True)
            want = model.mesh(0.5)
            assert len(want["cells"]) > 100 and np.array_equal(mesh["cells"], want["cells"])
            assert march_stats(vol)[3] & 1 == 0
            check_occupied(vol, model.occupied(), what=f"frame {k}")
            assert vol.occupiedStats()[2] == 0
        assert ((model.ov.w % 1) != 0).sum() > 1000 and (model.ov.w > 1).sum() > 1000   # one weighted and one plain observation
    finally:
        vol.close()


# ---- scripted reproductions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["RGBNormalized", "PACKED"])
def test_a_refused_upload_leaves_the_band_flags_alone(gpu, mode):
    """Found by one_handle-RGBNormalized-64-colour-seed2 (reset, refused calls, shift): tsdf_hip_upload ended the band flags
    before it looked at its arguments, so a call it REFUSED -- r,g,b bytes into an RGB_NORMALIZED volume (E_UNSUPPORTED), a
    box outside the grid (E_INVALID) -- cost every later reader its skips: the shift after it reported shiftStats()[2] == 0
    where the handle's flags were still exact, and on a fused PACKED volume the march read every cell."""
    vol, sc = make_volume(64, color=True)
    if mode == "RGBNormalized":
        vol.setColorMode(mode)
    vol.reset()
    lib, h = capi.load(), vol._need()
    rgb = np.full((2, 3, 4, 3), 200, np.uint8)
    try:
        if mode == "RGBNormalized":   # a fresh handle: the flags describe the planes until the first plain launch
            assert lib.tsdf_hip_upload(h, 1, 1, 1, 4, 3, 2, None, None, capi.as_u8p(rgb)) == capi.E_UNSUPPORTED
        else:
            assert vol.getLayout() == capi.LAYOUT_PACKED
            for k in range(2):
                tr = synth.turntable_pose(k, 8, sc.size)
                vol.integrateCloud(sc.depth(tr), sc.bgra(k), tr)
            assert lib.tsdf_hip_upload(h, 62, 1, 1, 4, 3, 2, None, None, capi.as_u8p(rgb)) == capi.E_INVALID
            mc = MarchingCubesTSDFOctree()
            mc.setInputTSDF(vol)
            mc.setMinWeight(1.0)
            mc.setColorByRGB(True)
            assert len(mc.reconstruct(want_cells=True)["cells"]) > 100 and march_stats(vol)[3] & 1 == 1
        vol.shiftVolume(1, 0, 0)
        assert vol.shiftStats()[2] == 1
        d = np.zeros((2, 3, 4), np.float32)   # ... and an upload that does write ends them, as before
        vol.upload(d=d, x0=1, y0=1, z0=1)
        vol.shiftVolume(-1, 0, 0)
        assert vol.shiftStats()[2] == 0
    finally:
        vol.close()
