"""GPU tier: tsdf_hip_merge (cpu_tsdf_amd/csrc/tsdf_merge.hip) -- a second volume resampled at this one's voxel centres
under a rigid transform and added as weighted observations.  Every expectation is tests/merge_cases.merge_model (numpy,
float32 step by step, on the ORACLE's centre tables, getFxn and getContainingVoxel) applied to the two downloads taken
BEFORE the call, compared bit for bit with download() after it; the band flags are checked through what their readers do
against a twin volume that received the merged arrays through upload()."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection time, before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi, synth
from tests import merge_cases as mc
from tests.common import assert_same_f32, frames, make_volume
from tests.sequence_util import march, read_detail

pytestmark = pytest.mark.gpu
PACKED, F32W = capi.LAYOUT_PACKED, capi.LAYOUT_F32W
LAYOUT_PAIRS = [(F32W, F32W), (F32W, PACKED), (PACKED, PACKED)]  # dst, src
COLOURS = [(True, True), (False, False), (True, False), (False, True)]  # dst, src
RES3 = (130, 10, 7)  # a non-cubic dst whose pitch (132) differs from nx, as in tests/test_shift_gpu.py


def same_volume(got, want, what):
    assert_same_f32(got[0], want[0], what + ": d")
    assert_same_f32(got[1], want[1], what + ": w")
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]), what + ": rgb"


def volume(res, size, color, layout, max_weight=3.0, res3=None, content=None, size3=None):
    vol, _ = make_volume(res, 80, 60, color=color, size=size, max_weight=max_weight, res3=res3, size3=size3)
    vol.setLayout(layout)
    vol.reset()
    assert vol.getLayout() == layout
    if content is not None:
        vol.upload(content[0], content[1], content[2] if color else None)
    return vol


def merge_raw(lib, dst, src, m12, min_weight=0.0, n=None):
    m = None if m12 is None else (C.c_double * 12)(*[float(v) for v in np.asarray(m12).reshape(12)])
    return lib.tsdf_hip_merge(dst._need(), src._need() if src is not None else None, m, C.c_float(min_weight), n)


# ---- 1. random volumes, every supported layout pair and colour setting ------------------------------------------------------
CASES = [(g[0], g[1], g[2], (g[3],) * 3, g[4], g[5], g[6]) for g in mc.GEOMETRIES] + \
        [("non_cubic_dst", 16, 1.0, RES3, None, mc.rigid((1, 2, 3), 0.4, (0.07, -0.05, 0.03)), 0)]


@pytest.mark.parametrize("dst_color,src_color", COLOURS, ids=["both", "none", "dst_only", "src_only"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_random_volumes_equal_the_model(gpu, case, dst_color, src_color):
    name, rs, ss, res3_d, sd, T, quoted = case
    rng = np.random.RandomState(5)
    if sd is None:
        sd = float(synth.scene_a(res3_d[0], 80, 60).size)  # (make_volume's default: a cube of 130 / 256 m)
    src_c = mc.random_volume(rng, (rs,) * 3, ss, True)
    dst_c = mc.random_volume(rng, res3_d, sd, True)
    want = None
    for dst_layout, src_layout in LAYOUT_PAIRS:
        src = volume(rs, ss, src_color, src_layout, content=src_c)
        dst = volume(res3_d[0], sd, dst_color, dst_layout, res3=res3_d, content=dst_c)
        before_d, before_s = dst.download(), src.download()
        if want is None:  # (the model does not depend on the layouts: weights 0..3 under max_weight 3 are counts)
            want = mc.merge_model(dst._p, before_d, src._p, before_s, T)
            print(f"{name}: {int(want[3].sum())} merged (the feature's specification quoted {quoted})")
            assert int(want[3].sum()) >= max(quoted // 2, 100), "an (almost) empty merge tests nothing"
            assert (want[1][want[3]] == 3).any() and (want[1][want[3]] < 3).any()  # the clamp is reached, and not everywhere
        n = dst.mergeVolume(src, T, count=True)
        what = f"{name}, dst layout {dst_layout}, src layout {src_layout}"
        same_volume(dst.download(), want, what)
        st = dst.mergeStats()
        assert n == int(want[3].sum()) and st[1] == n and st[2] == 0, (what, n, st)
        nd = res3_d[0] * res3_d[1] * res3_d[2]
        assert n <= st[0] <= nd, (what, st)
        same_volume(src.download(), before_s, what + ": src is unchanged")
        dst.close()
        src.close()


@pytest.mark.parametrize("size3,lost_rows", [((0.5, 1.0, 1.0), 1), ((0.5, 2.0, 2.0), 3)], ids=["size_0.5_1_1", "size_0.5_2_2"])
def test_octree_dst_with_a_non_cubic_grid_size(gpu, size3, lost_rows):
    """A 16^3 dst is an octree grid: its centre tables descend from size_x on EVERY axis (tsdf_node_size), whatever
    setGridSize said for y and z, and those tables are what the merge transforms.  A small src observed up to its faces and
    pushed towards dst's upper y and z faces reaches dst's last rows and planes; a launch box laid out on size_y / size_z
    instead of the tables' spacing ends `lost_rows` rows early (worked by hand: hi = ceil((0.255 + size_y / 2) * 16 / size_y
    - 0.5) + 2 = 14 and 12), and the whole-grid comparison shows it."""
    rng = np.random.RandomState(5)
    T = mc.rigid((1, 0, 0), 0.0, (0.0, 0.13, 0.135))  # row / plane 15 (centre 0.2344) samples src at 0.1044 / 0.0994: below its last half voxel
    src_c = mc.random_volume(rng, (8,) * 3, 0.25, True, ball=False)
    dst_c = mc.random_volume(rng, (16,) * 3, 0.5, True)
    for dst_layout, src_layout in [(PACKED, PACKED), (F32W, F32W)]:
        src = volume(8, 0.25, True, src_layout, content=src_c)
        dst = volume(16, 0.5, True, dst_layout, size3=size3, content=dst_c)
        assert np.array_equal(dst.centers(1), dst.centers(0)) and np.array_equal(dst.centers(2), dst.centers(0))
        before_d, before_s = dst.download(), src.download()
        want = mc.merge_model(dst._p, before_d, src._p, before_s, T)
        m = want[3]
        assert m[:, 16 - lost_rows:, :].sum() > 20 and m[16 - lost_rows:, :, :].sum() > 20 and m[:, 15, :].any() and m[15].any()
        n = dst.mergeVolume(src, T, count=True)
        same_volume(dst.download(), want, f"dst size {size3}, layouts {dst_layout} {src_layout}")
        assert n == int(m.sum()) == dst.mergeStats()[1]
        dst.close()
        src.close()


def test_a_src_out_of_reach_touches_nothing(gpu):
    src = volume(16, 1.0, True, PACKED, content=mc.random_volume(np.random.RandomState(5), (16,) * 3, 1.0, True))
    dst, sc = make_volume(16, 80, 60, color=True, size=1.0, max_weight=3.0)
    dst.reset()
    for i, tr, dep, col in frames(sc, 2, 8):  # only integrateCloud has written dst: its band flags are live
        dst.integrateCloud(dep, col, tr)
    before = dst.download()
    assert (before[1] > 0).sum() > 500
    assert dst.mergeVolume(src, mc.FAR, count=True) == 0
    assert dst.mergeStats() == (0, 0, 0, 0)
    assert dst.mergeVolume(src, mc.FAR) is True and dst.mergeStats() == (0, 0, 0, 0)
    same_volume(dst.download(), before, "a translation by 2 m")
    dst.getOccupiedVoxelIndices()
    assert dst.occupiedStats()[2] == 1  # the flags still decide what the scan reads
    dst.close()
    src.close()


# ---- 2. saturation and min_weight ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_weight", [0.0, 1.0, 2.5])
def test_saturation_and_min_weight(gpu, min_weight):
    """max_weight = 3 with weights up to 3 on both sides: sums of 4, 5 and 6 are clamped (PACKED: the count kmax), sums of 2
    and 3 are not; min_weight 1 and 2.5 close the gate for neighbourhoods with a weight of 1, or of 1 or 2."""
    _, rs, ss, rd, sd, T, _ = mc.GEOMETRIES[1]
    rng = np.random.RandomState(5)
    # (80 % of src's weights are 3: about 0.8^8 of the neighbourhoods inside the ball still pass min_weight 2.5)
    src_c, dst_c = mc.random_volume(rng, (rs,) * 3, ss, True, p_max=0.8), mc.random_volume(rng, (rd,) * 3, sd, True)
    counts = []
    for dst_layout, src_layout in [(PACKED, PACKED), (F32W, F32W)]:
        src, dst = volume(rs, ss, True, src_layout, content=src_c), volume(rd, sd, True, dst_layout, content=dst_c)
        before_d, before_s = dst.download(), src.download()
        want = mc.merge_model(dst._p, before_d, src._p, before_s, T, min_weight)
        m = want[3]
        assert (want[1][m] == 3).any() and (before_d[1][m] == 3).any()  # the clamp works on sums of 4 .. 6
        if min_weight == 0.0:
            assert (want[1][m] < 3).any()  # ... and leaves a sum of 2 alone
        n = dst.mergeVolume(src, T, min_weight=min_weight, count=True)
        same_volume(dst.download(), want, f"min_weight {min_weight}, layouts {dst_layout} {src_layout}")
        assert n == int(m.sum()) == dst.mergeStats()[1]
        counts.append(n)
        dst.close()
        src.close()
    print(f"min_weight {min_weight}: {counts[0]} merged")
    # floors from the share of src neighbourhoods that pass: ~0.97^8 * 700, ~(0.97 * 0.93)^8 * 700, ~(0.97 * 0.87)^8 * 700, halved
    assert counts[0] == counts[1] and counts[0] >= {0.0: 270, 1.0: 150, 2.5: 90}[min_weight]


def test_min_weight_closes_the_gate_step_by_step(gpu):
    """The same pair under the three thresholds: every higher threshold merges a subset (model and product alike)."""
    _, rs, ss, rd, sd, T, _ = mc.GEOMETRIES[1]
    rng = np.random.RandomState(5)
    src_c, dst_c = mc.random_volume(rng, (rs,) * 3, ss, False, p_max=0.8), mc.random_volume(rng, (rd,) * 3, sd, False)
    got = []
    for mw in (0.0, 1.0, 2.5):
        src, dst = volume(rs, ss, False, PACKED, content=src_c), volume(rd, sd, False, PACKED, content=dst_c)
        got.append(dst.mergeVolume(src, T, min_weight=mw, count=True))
        dst.close()
        src.close()
    assert got[0] > got[1] > got[2] > 0, got


# ---- 3. fused data -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_scene(gpu):
    """scene_a(32, 160, 120), eight turntable frames: what every case of test 3 fuses."""
    vol, sc = make_volume(32, 160, 120, color=True)
    fr = [(tr, dep, col) for i, tr, dep, col in frames(sc, 8, 8)]
    return sc, fr


def fuse(fr, idx, G=np.eye(4)):
    vol, _ = make_volume(32, 160, 120, color=True)
    vol.reset()
    Gi = np.linalg.inv(G)
    for i in idx:
        vol.integrateCloud(fr[i][1], fr[i][2], Gi @ fr[i][0])
    return vol


@pytest.mark.parametrize("which", ["identity", "turned"])
def test_merging_two_fused_halves_against_fusing_all_frames(fused_scene, which):
    """Frames 0-3 into A, frames 4-7 into B whose volume frame sits at G in A's (B's poses are G^-1 * pose), all eight
    into C; A.mergeVolume(B, G) equals the model bit for bit and is compared with C on the merged voxels with C.w > 0 and
    |C.d| < 0.9.
    G = identity: the weights equal C's exactly, and a weighted mean of two running means is the running mean of all
    frames up to rounding: |d - C.d| <= 1e-6 is asserted.  Measured (CPU model = GPU, bit for bit): 29620 merged, 22585
    compared, max |d - C.d| 1.2e-7.
    G = 0.3 rad about (1, 2, 3) plus (1.7, -0.6, 0.9) voxels: B's voxels sit elsewhere and are resampled; the median of
    |d - C.d| is asserted <= 0.02.  Measured: 26229 merged, 19283 compared, median 0.0076, 99th percentile 0.18, maximum
    0.53 -- the last two from the edges of the truncation band (printed, not asserted); 96 % of the weights equal C's."""
    sc, fr = fused_scene
    voxel = sc.size / 32
    G = np.eye(4) if which == "identity" else mc.rigid((1, 2, 3), 0.3, np.array([1.7, -0.6, 0.9]) * voxel)
    A, B, Cv = fuse(fr, range(4)), fuse(fr, range(4, 8), G), fuse(fr, range(8))
    assert A.getLayout() == PACKED and B.getLayout() == PACKED
    before_a, before_b, c = A.download(), B.download(), Cv.download()
    want = mc.merge_model(A._p, before_a, B._p, before_b, G)
    n = A.mergeVolume(B, G, count=True)
    got = A.download()
    same_volume(got, want, which)
    same_volume(B.download(), before_b, "src is unchanged")
    m = want[3]
    assert n == int(m.sum()) and A.mergeStats()[1:3] == (n, 1)
    sel = m & (c[1] > 0) & (np.abs(c[0]) < 0.9)
    err = np.abs(got[0][sel] - c[0][sel])
    print(f"{which}: {n} merged, {int(sel.sum())} compared with C, weights equal {float((got[1][sel] == c[1][sel]).mean()):.4f}, "
          f"|d - C.d| median {np.median(err):.3g} p99 {np.percentile(err, 99):.3g} max {err.max():.3g}")
    assert n >= 20000 and sel.sum() >= 15000
    if which == "identity":
        assert np.array_equal(got[1][sel], c[1][sel])
        assert err.max() <= 1e-6
    else:
        assert np.median(err) <= 0.02
    for v in (A, B, Cv):
        v.close()


# ---- 4. the readers after a merge ---------------------------------------------------------------------------------------------
def test_readers_after_a_merge_equal_a_twin_that_was_uploaded(gpu):
    """dst holds two frames from one side and nothing but integrateCloud has written it: its band flags are live and say
    where NOT to look.  src holds two frames from the other side, so the merged surface lies where dst never observed
    inside the band.  Every reader that trusts live flags must then read everything, as on the twin."""
    def build(idx):
        vol, sc = make_volume(64, 160, 120, color=True)
        vol.reset()
        fr = list(frames(sc, 8, 8))
        for i in idx:
            vol.integrateCloud(fr[i][2], fr[i][3], fr[i][1])
        return vol, fr
    dst, fr = build((0, 1))
    src, _ = build((4, 5))
    assert dst.getLayout() == PACKED and read_detail(dst)[1] == 1  # (implied distances on: the flags are in use)
    mesh0, st0 = march(dst)
    assert st0[3] & 1 == 1
    before = dst.download()
    n = dst.mergeVolume(src, count=True)  # (both global transforms are the identity)
    assert n > 100000 and dst.mergeStats()[1:3] == (n, 1)
    merged = dst.download()
    new = (np.abs(merged[0]) < 1) & (merged[1] > 0) & ((before[1] == 0) | (np.abs(before[0]) >= 1))
    assert new.sum() > 10000, "the merged surface should lie where dst had none"
    twin, _ = make_volume(64, 160, 120, color=True)
    twin.reset()
    twin.upload(*merged)
    mesh, mst = march(dst)
    tmesh, tst = march(twin)
    assert mst[3] & 1 == 0 and tst[3] & 1 == 0, (mst, tst)
    assert np.array_equal(mesh["cells"], tmesh["cells"])
    assert np.setdiff1d(mesh["cells"], mesh0["cells"]).size > 1000  # triangles in cells that had none before the merge
    assert_same_f32(mesh["vertices"], tmesh["vertices"], "mesh vertices")
    assert np.array_equal(mesh["rgb"], tmesh["rgb"])
    a, b = dst.getOccupiedVoxelIndices(want=("d", "w", "rgb")), twin.getOccupiedVoxelIndices(want=("d", "w", "rgb"))
    assert len(a[0]) > 0 and dst.occupiedStats()[2] == 0 and twin.occupiedStats()[2] == 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    i, tr, dep, col = fr[2]
    na, nb = dst.integrateCloud(dep, col, tr, count=True), twin.integrateCloud(dep, col, tr, count=True)
    assert na == nb and na > 0 and read_detail(dst)[1] == 0 and read_detail(twin)[1] == 0
    same_volume(dst.download(), twin.download(), "one more frame after the merge")
    for v in (dst, src, twin):
        v.close()


# ---- 5. ordering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parked_in", ["dst", "src"])
def test_a_frame_held_back_by_frame_pairing_is_part_of_what_the_merge_sees(gpu, parked_in):
    got = []
    for pairing in (False, True):
        vols = {}
        for role in ("dst", "src"):
            vol, sc = make_volume(32, 160, 120, color=True)
            vol.setFramePairing(pairing and role == parked_in)
            vol.reset()
            fr = list(frames(sc, 8, 8))
            for i, tr, dep, col in (fr[:3] if role == "dst" else fr[4:7]):  # three frames: with pairing the third waits
                vol.integrateCloud(dep, col, tr, pipelined=True)
            vols[role] = vol
        vols["dst"].mergeVolume(vols["src"])
        got.append((vols["dst"].download(), vols["src"].download()))
        for v in vols.values():
            v.close()
    assert (got[0][0][1] > 0).sum() > 1000
    same_volume(got[1][0], got[0][0], f"dst, a frame parked in {parked_in}: pairing on against pairing off")
    same_volume(got[1][1], got[0][1], f"src, a frame parked in {parked_in}: pairing on against pairing off")


def test_src_on_a_stream_of_its_own_with_work_queued_before_and_after(gpu):
    """src integrates asynchronously on its own stream right before the merge and again right after it: the merge reads
    src after the first, and the second does not overtake the read.  Against the same sequence with a wait after each step."""
    got = []
    for wait in (True, False):
        stream = None if wait else torch.cuda.Stream()
        vols = {}
        for role in ("dst", "src"):
            vol, sc = make_volume(32, 160, 120, color=True)
            if role == "src" and stream is not None:
                vol.setStream(stream.cuda_stream)
            vol.reset()
            vols[role] = vol
        fr = list(frames(sc, 8, 8))
        dst, src = vols["dst"], vols["src"]
        dst.integrateCloud(fr[0][2], fr[0][3], fr[0][1])
        src.integrateCloud(fr[4][2], fr[4][3], fr[4][1])
        src.integrateCloud(fr[5][2], fr[5][3], fr[5][1], pipelined=not wait)
        if wait:
            src.synchronize()
        dst.mergeVolume(src)
        if wait:
            dst.synchronize()
        src.integrateCloud(fr[6][2], fr[6][3], fr[6][1], pipelined=not wait)
        got.append((dst.download(), src.download()))
        for v in vols.values():
            v.close()
    assert (got[0][0][1] > 1).sum() > 1000
    same_volume(got[1][0], got[0][0], "dst: asynchronous against synchronous")
    same_volume(got[1][1], got[0][1], "src: asynchronous against synchronous")


# ---- 6. every refusal -------------------------------------------------------------------------------------------------------------
IDENTITY12 = np.eye(4)[:3, :4]


def test_every_refusal(gpu):
    lib = gpu
    rng = np.random.RandomState(5)
    content = mc.random_volume(rng, (16,) * 3, 1.0, True)
    dst, src = volume(16, 1.0, True, PACKED, content=content), volume(16, 1.0, True, PACKED, content=content)
    before = dst.download()

    def refused(d, s, m12, min_weight, code, word, what):
        d_before = d.download()
        n = C.c_uint64(7)
        rc = merge_raw(lib, d, s, m12, min_weight, C.byref(n))
        assert rc == code, (what, rc)
        if code == capi.E_UNSUPPORTED:
            msg = lib.tsdf_hip_last_error().decode()
            assert "tsdf_hip_merge" in msg and word in msg, (what, msg)
        same_volume(d.download(), d_before, what + ": dst is unchanged")
        assert n.value == 7, what

    # E_INVALID
    refused(dst, src, None, 0.0, capi.E_INVALID, "", "a NULL matrix")
    refused(dst, None, IDENTITY12, 0.0, capi.E_INVALID, "", "a NULL src")
    refused(dst, dst, IDENTITY12, 0.0, capi.E_INVALID, "", "dst == src")
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            m = IDENTITY12.copy().reshape(12)
            m[k] = bad
            refused(dst, src, m, 0.0, capi.E_INVALID, "", f"matrix entry {k} = {bad}")
    refused(dst, src, IDENTITY12, -0.5, capi.E_INVALID, "", "a negative min_weight")
    refused(dst, src, IDENTITY12, float("nan"), capi.E_INVALID, "", "a NaN min_weight")

    # E_UNSUPPORTED: the odd volume once as src, once (where it can be a dst at all) as dst
    def odd(**kw):
        vol, _ = make_volume(kw.pop("res", 16), 80, 60, color=kw.pop("color", True), size=1.0, max_weight=kw.pop("max_weight", 3.0),
                             res3=kw.pop("res3", None), size3=kw.pop("size3", None), trunc=kw.pop("trunc", (0.03, 0.03)))
        vol.setLayout(kw.pop("layout", capi.LAYOUT_AUTO))
        for name, args in kw.items():
            getattr(vol, name)(*args)
        vol.reset()
        return vol
    both_ways = [
        ("multi-GPU", odd(setDevices=([0, 0],)), "a multi-GPU set"),
        ("part of its grid", odd(setZSlab=(4, 12, 2)), "a Z-slab handle"),
        ("truncation limits", odd(trunc=(0.03, 0.02)), "another max_dist_neg"),
        ("truncation limits", odd(trunc=(0.05, 0.03)), "another max_dist_pos"),
        ("RGB_NORMALIZED / LAB", odd(setColorMode=("RGBNormalized",)), "RGB_NORMALIZED"),
        ("RGB_NORMALIZED / LAB", odd(setColorMode=("LAB",)), "LAB"),
        ("by depth or by variance", odd(layout=F32W, setWeighting=(True, False)), "weight_by_depth"),
        ("by depth or by variance", odd(layout=F32W, setWeighting=(False, True)), "weight_by_variance"),
    ]
    f32w_dst = volume(16, 1.0, True, F32W, content=content)  # (a float-weighted odd volume must not trip the PACKED rule first)
    for word, vol, what in both_ways:
        refused(f32w_dst, vol, IDENTITY12, 0.0, capi.E_UNSUPPORTED, word, what + " as src")
        refused(vol, src, IDENTITY12, 0.0, capi.E_UNSUPPORTED, word, what + " as dst")
        vol.close()
    src_only = [
        ("cubic", odd(res=16, res3=(16, 16, 8)), "src res not equal on all axes"),
        ("cubic", odd(size3=(1.0, 1.0, 0.5)), "src size not equal on all axes"),
    ]
    for word, vol, what in src_only:
        refused(f32w_dst, vol, IDENTITY12, 0.0, capi.E_UNSUPPORTED, word, what)
        vol.close()
    for word, vol, what in [("PACKED", odd(layout=F32W), "a PACKED dst with an F32W src"),
                            ("PACKED", odd(layout=PACKED, max_weight=5.0), "a PACKED dst with another max_weight in src")]:
        refused(dst, vol, IDENTITY12, 0.0, capi.E_UNSUPPORTED, word, what)
        vol.close()
    if lib.tsdf_hip_device_count() > 1:  # (needs a second GPU; with one, no handle can be on another device)
        vol, _ = make_volume(16, 80, 60, color=True, size=1.0, max_weight=3.0)
        vol.setZSlab(0, 0, 0, device=1)
        vol.reset()
        refused(dst, vol, IDENTITY12, 0.0, capi.E_UNSUPPORTED, "different devices", "src on another device")
        vol.close()
    # and nothing of all that left a trace: the pair still merges
    same_volume(dst.download(), before, "dst after every refusal")
    assert dst.mergeVolume(src, count=True) == 675
    for v in (dst, src, f32w_dst):
        v.close()
