"""Helper of tests/test_mode_sequences_gpu.py and of its CPU replay in tests/test_sequence_model.py: the cases, their
parameters, their frames and their PLANS for the second integrate family (setColorMode("RGBNormalized" / "LAB"),
setWeighting(by_depth, by_variance)).  Nothing here touches a GPU.

A plan is the whole list of operations of a case with every parameter that changes the volume, drawn up front from the
case's seed: a shuffled deck that holds every operation legal in the case once (upload and save_load twice, shift three
times) plus a few random extras, behind one host frame, with its one reset in the first third and with a ring step that
holds a frame back right before the last shift.  So the model's side of a sequence can be replayed without the product (replay()), the tally of
operations is known before any GPU runs, and the conditions the inputs must meet (CONDITIONS) are checked twice: by the
replay on the CPU and from the GPU driver's own model after the sequence.

The counts of CONDITIONS are the PEAK over the steps of a sequence (a reset, or an x shift by the whole 64^3 grid, late in a
plan empties the state again; what matters is that the state existed at steps that were compared and had frames after
them).  TwinModel keeps, next to the model, a plain-RGB model (colour modes) and an unculled one (cull seeds) that see the
same operations, for the two conditions that compare against them."""
import collections

import numpy as np

from cpu_tsdf_amd import synth
from cpu_tsdf_amd.volume import TSDFVolumeOctree
from tests.evidence.fuzz_product_colour_modes import MODES
from tests.sequence_model import Model, draw_shift, slab_starts

SET = [0, 0, 0]
SHAPES = {"one_handle": None, "set_0_0_0": SET}
GRIDS = {"64": (64, 64, 64), "flat": (70, 36, 45)}   # flat: pitch 72 != nx, a partial second x cell, ny % 4 != 0, 15-plane slabs
COLOUR_MODES = ("RGBNormalized", "LAB")
W, H = 160, 120
N_POSES = 3
EXTRA_STEPS = 4
PURE_X = [1, -1, 3, -3, 64, -64, 65, -65]   # the register path, whole flag cells, a cell and one more
FRAME_OPS = {"host": 1, "device": 1, "pair": 2}   # (ring: 1 - 3, drawn)
MUTATING = ["host", "device", "pair", "ring", "shift", "upload", "upload_variance", "save_load", "reset", "refused"]
READING = ["mesh", "occupied", "render", "sample", "align"]
# seeds whose first draw missed a condition of CONDITIONS on the CPU replay: (shape, mode, grid, seed) -> the salt that replaces it
SALT = {("one_handle", "RGBNormalized", "64", 1): 1, ("one_handle", "LAB", "64", 1): 1, ("one_handle", "by_variance", "64", 1): 4,
        ("one_handle", "by_variance", "64", 2): 3, ("one_handle", "by_variance", "flat", 0): 1, ("one_handle", "by_depth+by_variance", "64", 0): 1,
        ("one_handle", "by_depth+by_variance", "64", 1): 1, ("set_0_0_0", "by_variance", "64", 2): 1, ("set_0_0_0", "by_depth+by_variance", "64", 0): 2}

Case = collections.namedtuple("Case", "shape mode grid seed color cull order")


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        for mi, mode in enumerate(MODES):
            for grid, seeds in (("64", 3), ("flat", 1)):
                for seed in range(seeds):
                    # the weightings run with and without colour; seed 1 of every mode on 64^3 has the cull decide voxels
                    color = mode in COLOUR_MODES or (seed != 1 if grid == "64" else (mi + si) % 2 == 0)
                    out.append(Case(shape, mode, grid, seed, color, grid == "64" and seed == 1, (seed + mi + si) % 2))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.shape}-{c.mode}-{c.grid}-{'colour' if c.color else 'plain'}-seed{c.seed}{'-cull' if c.cull else ''}"


def case_seed(c):
    key = (c.shape, c.mode, c.grid, c.seed)
    return 77000 + 1000 * MODES.index(c.mode) + 100 * list(GRIDS).index(c.grid) + 10 * c.seed + 5 * list(SHAPES).index(c.shape) + 100000 * SALT.get(key, 0)


def legal_ops(c):
    ops = ["host", "device", "pair", "ring", "shift", "upload", "reset"] + READING
    if "by_variance" in c.mode:
        ops.append("upload_variance")
    if c.mode not in COLOUR_MODES and c.grid == "64":
        ops.append("save_load")   # (.vol needs a cubic power-of-two grid; RGB_NORMALIZED / LAB have no .vol form)
    ops.append("refused")         # (every mode refuses deintegrateCloud and mergeVolume; the colour modes and the sets refuse more)
    return ops


def refused_is_drawn(c):
    """The cases whose plans DRAW `refused` steps from their deck; the others (a weighted single handle, which had no call to
    refuse before deintegrateCloud and mergeVolume came) get one refused step at a fixed place, so that their draws stay as
    they were."""
    return c.mode in COLOUR_MODES or SHAPES[c.shape] is not None


class Setup:
    """Everything of a case that is not the volume: parameters, camera, scene, poses, frames, plan."""

    def __init__(self, c):
        self.case = c
        rng = np.random.RandomState(case_seed(c))
        self.res3 = GRIDS[c.grid]
        nx = self.res3[0]
        self.size3 = tuple(1.0 * r / nx for r in self.res3)   # cubic voxels
        self.size = min(self.size3)
        self.wmax = float(rng.choice([2.0, 3.5, 100.0, 255.0]))
        self.trunc = (float(rng.choice([0.04, 0.06])), float(rng.choice([0.04, 0.06])))
        if c.cull:   # the narrow off-centre camera of the colour-mode fuzz script: the reference's cull drops voxels that project into the image
            f = float(rng.uniform(1.0, 1.6)) * W
            cx = W / 2 - 0.5 + rng.choice([-1, 1]) * float(rng.uniform(0.15, 0.4)) * W / 2
            cy = H / 2 - 0.5 + rng.choice([-1, 1]) * float(rng.uniform(0.0, 0.4)) * H / 2
        else:
            f, cx, cy = 0.9 * W, W / 2 - 0.5, H / 2 - 0.5
        self.cam = (f, f * float(rng.uniform(0.95, 1.05)), cx, cy)
        sc = synth.Scene(self.size, W, H, sphere=float(rng.uniform(0.2, 0.3)), box=0.47)
        sc.fx, sc.fy, sc.cx, sc.cy = self.cam
        sc.h = np.array([0.47 * s for s in self.size3])
        self.sc = sc
        self.poses = []
        for _ in range(N_POSES):
            eye = rng.normal(size=3)
            eye[1] *= 0.4
            eye *= float(rng.uniform(1.3, 2.0)) * self.size / np.linalg.norm(eye)
            self.poses.append(synth.look_at_pose(eye, target=rng.uniform(-0.1, 0.1, 3) * self.size))
        self.starts = slab_starts(self.res3[2])
        self.thick = max(b - a for a, b in zip(self.starts, self.starts[1:]))
        self.plan = self._plan(np.random.RandomState(case_seed(c) + 1))

    def product(self):
        """The configured product volume (reset() not yet called)."""
        c, v = self.case, TSDFVolumeOctree()
        v.setResolution(*self.res3)
        v.setGridSize(*self.size3)
        v.setImageSize(W, H)
        v.setCameraIntrinsics(*self.cam)
        v.setSensorDistanceBounds(0.0, 3.0)
        v.setDepthTruncationLimits(*self.trunc)
        v.setWeightTruncationLimit(self.wmax)
        v.setIntegrateColor(c.color)
        v.setTransformOrder(c.order)
        if c.mode in COLOUR_MODES:
            v.setColorMode(c.mode)
        else:
            v.setWeighting("by_depth" in c.mode, "by_variance" in c.mode)
        v.setDevices(SHAPES[c.shape])
        return v

    def frame(self, i):
        """Frame i in the frame the volume started in: (pose, depth, bgra).  Poses repeat every N_POSES frames, so nsample
        passes 5; NaN, 0 and inf depths in every frame; random colours with black pixels in every third frame."""
        rng = np.random.RandomState(case_seed(self.case) * 64 + 7 + i)
        tr = self.poses[i % N_POSES]
        dep = self.sc.depth(tr, noise_seed=int(rng.randint(1 << 30)), noise_sigma=float(rng.choice([0.002, 0.01])) * self.size)
        junk = rng.rand(H, W)
        dep[junk < 0.03] = np.nan
        dep[(junk >= 0.03) & (junk < 0.04)] = 0.0
        dep[(junk >= 0.04) & (junk < 0.05)] = np.inf
        if i % 3 == 1:
            col = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
            col[rng.rand(H, W) < 0.04, :3] = 0
        else:
            col = self.sc.bgra(i)
        return tr, dep, col

    def seam_box(self, rng):
        """(x0, y0, z0, nx, ny, nz) with non-zero origin whose z range crosses a slab seam of the three-slab partition."""
        rx, ry, _ = self.res3
        seam = self.starts[1 + rng.randint(2)]
        z0 = seam - int(rng.randint(1, 4))
        nz = seam - z0 + int(rng.randint(1, 4))
        x0, y0 = int(rng.randint(1, rx // 4)), int(rng.randint(1, ry // 4))
        return x0, y0, z0, int(rng.randint(rx // 2, rx - x0 + 1)), int(rng.randint(ry // 2, ry - y0 + 1)), nz

    def _plan(self, rng):
        legal = [o for o in legal_ops(self.case) if o != "refused" or refused_is_drawn(self.case)]
        deck = list(legal) + [o for o in ("shift", "shift", "upload", "save_load") if o in legal]
        extras = [o for o in legal if o != "reset"]
        deck += [extras[rng.randint(len(extras))] for _ in range(EXTRA_STEPS)]
        rng.shuffle(deck)
        at = deck.index("reset")   # the one reset comes in the first third: the frames after it let nsample pass 5 again
        deck.insert(int(rng.randint(len(deck) // 3)), deck.pop(at))
        deck.insert(0, "host")     # (and no plan starts by shifting an empty grid)
        deck.pop(deck.index("ring"))   # one ring step leaves a frame held back for pairing right before the last shift
        held = max(i for i, o in enumerate(deck) if o == "shift")
        deck.insert(held, "ring")
        plan, cum = [], [0, 0, 0]
        for i, op in enumerate(deck):
            e = dict(op=op)
            if op == "ring":
                e["n"] = int(rng.choice([1, 3])) if i == held else int(rng.randint(1, 4))
            elif op == "shift":
                e["s"] = draw_shift(rng, cum, self.thick)
                if not any("s" in q for q in plan):   # the first shift of a plan is a pure x shift: all eight occur on both grids
                    mine = [q for q in CASES if q.grid == self.case.grid]
                    e["s"] = (PURE_X[mine.index(self.case) % len(PURE_X)], 0, 0)
                cum = [a + b for a, b in zip(cum, e["s"])]
            elif op == "upload":
                e["box"], e["which"] = self.seam_box(rng), ["d", "w", "dw"][rng.randint(3)]
            elif op == "upload_variance":
                e["box"], e["which"], e["seed"] = self.seam_box(rng), ["M", "ns", "both"][rng.randint(3)], int(rng.randint(1 << 30))
            plan.append(e)
        if not refused_is_drawn(self.case):
            plan.insert(1, dict(op="refused"))   # right after the first frame
        return plan + [dict(op="host"), dict(op="host")]   # the ending: a damaged state plane shows in rgb or w


def upload_arrays(model, e):
    """What an upload step writes: d lowered by 1/8 (clamped), weights halved (F32W layouts: no floor)."""
    d, w, _ = (a.copy() if a is not None else None for a in model.box(*e["box"]))
    seen = w > 0
    d[seen] = np.maximum(d[seen] - np.float32(0.125), np.float32(-1.0))
    w = w * np.float32(0.5)
    return (d if "d" in e["which"] else None), (w if "w" in e["which"] else None)


def variance_arrays(e):
    rng = np.random.RandomState(e["seed"])
    shape = e["box"][5], e["box"][4], e["box"][3]
    M, ns = rng.uniform(0, 2, shape).astype(np.float32), rng.randint(0, 12, shape).astype(np.int32)
    return (M if e["which"] != "ns" else None), (ns if e["which"] != "M" else None)


CONDITIONS = ("by_variance: voxels with nsample > 5 and a fractional weight", "by_depth: voxels with a fractional weight",
              "colour modes: voxels with non-zero cn", "colour modes: observed voxels whose rgb differs from plain RGB integration",
              "cull seeds: voxels whose d or w differ from the unculled model", "a shift that left > 1000 observed voxels and had a frame after it")


class TwinModel(Model):
    """The model of a case, the twins that two of the conditions compare against, and the peak of every condition's count."""

    def __init__(self, setup, params):
        c = setup.case
        super().__init__(params, c.mode, cull=True)   # (the product applies the reference's cull on every frame)
        self.case = c
        self.twins = {}
        if c.mode in COLOUR_MODES:
            self.twins["plain"] = Model(params, None, cull=True)
        if c.cull:
            self.twins["uncull"] = Model(params, c.mode, cull=False)
        self.peak = collections.Counter()
        self.after_shift = False

    def reset(self):
        super().reset()
        for t in getattr(self, "twins", {}).values():
            t.reset()
        self.after_shift = False

    def integrate(self, depth, bgra, trans):
        n = super().integrate(depth, bgra, trans)
        for t in self.twins.values():
            t.integrate(depth, bgra, trans)
        if self.after_shift:
            self.peak["shift"] = 1
        self.measure()
        return n

    def shift(self, s, moved):
        super().shift(s, moved)
        for t in self.twins.values():
            t.shift(s, moved)
        self.after_shift = any(s) and int((self.ov.w > 0).sum()) > 1000

    def upload(self, d=None, w=None, rgb=None, x0=0, y0=0, z0=0):
        super().upload(d, w, rgb, x0, y0, z0)
        for t in self.twins.values():
            t.upload(d, w, rgb, x0, y0, z0)

    def upload_variance(self, M, ns, box):
        super().upload_variance(M, ns, box)
        if "uncull" in self.twins:
            self.twins["uncull"].upload_variance(M, ns, box)

    def measure(self):
        ov, mode, peak = self.ov, self.mode, self.peak
        frac = (ov.w % 1) != 0
        if "by_variance" in mode:
            peak["variance"] = max(peak["variance"], int(((ov.nsample > 5) & frac).sum()))
        if "by_depth" in mode:
            peak["depth"] = max(peak["depth"], int(frac.sum()))
        if mode in COLOUR_MODES:
            peak["cn"] = max(peak["cn"], int((ov.cn != 0).any(0).sum()))
            peak["rgb"] = max(peak["rgb"], int(((ov.w > 0) & (ov.rgb != self.twins["plain"].ov.rgb).any(-1)).sum()))
        if "uncull" in self.twins:
            u = self.twins["uncull"].ov
            peak["cull"] = max(peak["cull"], int(((ov.w.view(np.uint32) != u.w.view(np.uint32)) | (ov.d.view(np.uint32) != u.d.view(np.uint32))).sum()))

    def assert_conditions(self, what):
        """CONDITIONS, from the model's own arrays; returns the counts."""
        mode, peak = self.mode, dict(self.peak)
        if "by_variance" in mode:
            assert peak.get("variance", 0) >= 1000, (what, CONDITIONS[0], peak)
        if "by_depth" in mode:
            assert peak.get("depth", 0) >= 1000, (what, CONDITIONS[1], peak)
        if mode in COLOUR_MODES:
            assert peak.get("cn", 0) >= 1000, (what, CONDITIONS[2], peak)
            assert peak.get("rgb", 0) >= 1000, (what, CONDITIONS[3], peak)
        if self.case.cull:
            assert peak.get("cull", 0) >= 1, (what, CONDITIONS[4], peak)
        assert peak.get("shift", 0) == 1, (what, CONDITIONS[5], peak)
        return peak


def params_of(setup):
    """The tsdf_params of the case (the product object's, layout as reset() will resolve it: the oracle does not read it)."""
    return setup.product()._p


def replay(c):
    """The model's side of the whole plan of a case, without the product: (TwinModel, Counter of the operations)."""
    setup = Setup(c)
    p = params_of(setup)
    model = TwinModel(setup, p)
    tally, frame_no = collections.Counter(), 0
    voxel = [float(p.size[a]) / int(p.res[a]) for a in range(3)]   # (shiftVolume returns s * size / res of the float32 size)
    for e in setup.plan:
        op = e["op"]
        tally[op] += 1
        for _ in range(FRAME_OPS.get(op, e.get("n", 0))):
            tr, dep, col = setup.frame(frame_no)
            frame_no += 1
            model.integrate(dep, col, model.pose(tr))
        if op == "shift":
            model.shift(e["s"], np.array([e["s"][a] * voxel[a] for a in range(3)], np.float64))
        elif op == "upload":
            d, w = upload_arrays(model, e)
            model.upload(d=d, w=w, x0=e["box"][0], y0=e["box"][1], z0=e["box"][2])
        elif op == "upload_variance":
            model.upload_variance(*variance_arrays(e), e["box"])
        elif op == "reset":
            model.reset()
    tally["host"] -= 2   # (the ending is not part of the tally)
    return model, tally

