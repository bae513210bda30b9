"""GPU tier: the frame as 8-byte pixel records (k_frame_pairs + the colour instances of k_integrate and k_integrate2,
cpu_tsdf_amd/csrc/tsdf_integrate.hip).

The colour fast kernels gather {depth, bgra} of a pixel with one 8-byte load from records the handle builds from the caller's
two images right before the launch.  The bar is bit equality everywhere: the record pass against numpy, and the CPU oracle
(the reference's integrateCloud, include/cpu_tsdf/impl/tsdf_volume_octree.hpp:48-218) for every instance that reads records,
on the smallest grid that still has several wave-rows per block (64 x 16 x 8 voxels, a 33 x 17 image: odd width, odd pixel
count)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests.common import assert_same_f32, make_volume

pytestmark = pytest.mark.gpu

W, H = 33, 17
RES3, SIZE3 = (64, 16, 8), (0.25, 0.0625, 0.03125)  # voxels of 2^-8 m
_U32P = C.POINTER(C.c_uint32)


@pytest.fixture(autouse=True)
def _knobs_back(gpu):
    yield
    for name, value in (("pipe", 1), ("fuse2", 1), ("cull", 1), ("allin", 1), ("plain_kernel", 0)):
        capi.set_tuning(name, value)


def small_volume(color=True, layout=None):
    vol, sc = make_volume(64, W, H, color=color, res3=RES3, size3=SIZE3, zmax=3.0, trunc=(0.01, 0.01))
    if layout is not None:
        vol.setLayout(layout)
    vol.reset()
    return vol, sc


def launch_info(vol):
    out = (C.c_int32 * 4)()
    capi.check(capi.load().tsdf_hip_last_launch_info(vol._need(), out), "last_launch_info")
    return [int(out[0]) & 0xff, int(out[1]), int(out[2]), int(out[3]), bool(int(out[0]) & 0x100)]


def pose_outside(i):
    """The whole grid in view with pixels to spare (ALLIN): 0.3 m in front of it, columns 3 .. 29 of the image."""
    return synth.look_at_pose((0.02 * i - 0.02, 0.005 * i, -0.3))


def pose_close(i):
    """A decimetre from the grid: it overflows the image on every side (pixel -1 occurs, and the reference's cull bites)."""
    return synth.look_at_pose((0.01 * i - 0.01, 0.002 * i, -0.1))


def frame_for(tr, seed):
    """A noisy surface through the middle of the grid (voxels in front, inside the band and behind), NaN holes, random colour
    words with the alpha byte included."""
    rng = np.random.RandomState(seed)
    dist = float(np.linalg.norm(tr[:3, 3]))
    dep = (dist + rng.uniform(-0.03, 0.03, (H, W))).astype(np.float32)
    dep[rng.randint(0, H, 12), rng.randint(0, W, 12)] = np.nan
    col = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
    return dep, col


def device_frame(dep, col):
    """[depth | bgra] in one allocation (561 pixels: the colour image is only 4-byte aligned)."""
    t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    t[0].copy_(torch.from_numpy(dep))
    t[1].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
    return t


def planes_equal(vol, ov, what):
    d, w, rgb = vol.download()
    assert_same_f32(d, ov.d, what + ": d")
    assert_same_f32(w, ov.w, what + ": w")
    assert np.array_equal(rgb, ov.rgb), what + ": colour"
    return d.view(np.uint32).copy(), w.view(np.uint32).copy(), rgb.copy()


# ---- the record pass alone ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (33, 17)])
def test_k_frame_pairs_interleaves_bits_and_leaves_the_images_alone(gpu, w, h):
    n = w * h
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff, 0xffbfffff,
                        0x00000001, 0x807fffff, 0x00400000, 0x3f800000], np.uint32)  # +-0, +-Inf, quiet / signalling NaNs, subnormals
    depth = np.resize(special, n).astype(np.uint32)
    rng = np.random.RandomState(n)
    bgra = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    # the record form of tsdf_hip_selftest_struct_oob: the pass, then the kernels' 8-byte gather at every pixel and at a ring of
    # positions outside the image (pixel -1); the hook itself fails if the pass wrote behind the last record or changed its inputs
    img = np.concatenate([depth, bgra]).view(np.float32)
    uv = np.array([(u, v) for v in range(-1, h + 1) for u in range(-1, w + 1)], np.int32)
    out = np.full(2 * len(uv), 0xdeadbeef, np.uint32)
    capi.check(capi.load().tsdf_hip_selftest_struct_oob(capi.as_f32p(img), w, h, 2, -1, uv.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        out.ctypes.data_as(_U32P), len(uv)), "record gather")
    inside = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
    assert inside.sum() == n
    pix = (uv[:, 1] * w + uv[:, 0])[inside]
    assert np.array_equal(out[0::2][inside], depth[pix]) and np.array_equal(out[1::2][inside], bgra[pix])
    assert not out[0::2][~inside].any() and not out[1::2][~inside].any()


# ---- records == oracle, per instance ---------------------------------------------------------------------------------

def run_single(kind):
    """Four frames through the single-frame entry point: three through the instance `kind` names, the fourth through its
    counting twin (the observed-voxel count)."""
    capi.set_tuning("pipe", 0)
    capi.set_tuning("cull", 0 if kind == "general" else 1)
    vol, sc = small_volume()
    if kind == "general":
        vol.setReferenceCull(False)
    ov = OracleVolume(vol._p)
    counts = []
    for i in range(4):
        tr = pose_close(i) if kind in ("general", "live") else pose_outside(i)
        dep, col = frame_for(tr, 100 + i)
        count = kind == "count" or i == 3
        T = synth.cam_from_vol_f32(tr)
        want = ov.integrate(dep, col, T) if kind == "general" else ov.integrate_culled(dep, col, tr, T)
        got = vol.integrateCloud(dep, col, tr, count=count)
        if count:
            assert got == want, (kind, i, got, want)
        info = launch_info(vol)
        expect = {"allin": (1, 0, False), "count": (1, 0, False), "general": (0, 0, False), "live": (0, 2, False)}[kind]
        assert (info[0], info[2], info[4]) == expect and info[1] == 1, (kind, i, info)
    planes_equal(vol, ov, kind)
    assert ov.w.max() == 4 and (ov.w > 0).mean() > 0.2 and (np.abs(ov.d) < 1).sum() > 100  # counts reach 4, a band exists
    vol.close()


@pytest.mark.parametrize("kind", ["allin", "count", "general", "live"])
def test_records_and_planar_frame_give_the_oracles_voxels(gpu, kind):
    """(The planar gather the name recalls is gone: the oracle is the bar.)"""
    run_single(kind)


def run_pairs(poses, expect_fused):
    capi.set_tuning("fuse2", 2)
    vol, sc = small_volume()
    ov = OracleVolume(vol._p)
    keep = []
    for k in range(2):
        pair, want = [], []
        for i in (2 * k, 2 * k + 1):
            tr = poses(i)
            dep, col = frame_for(tr, 200 + i)
            t = device_frame(dep, col)
            keep.append(t)
            pair.append((t[0].data_ptr(), t[1].data_ptr(), tr))
            want.append(ov.integrate_culled(dep, col, tr, synth.cam_from_vol_f32(tr)))
        fused, got = vol.integrateCloudDevice2(pair[0], pair[1], count=(k == 1))
        assert fused == expect_fused[k], (k, fused, launch_info(vol))
        if fused:
            assert launch_info(vol)[0] == 2
        if got is not None:
            assert got == want, (k, got, want)
    vol.synchronize()
    planes_equal(vol, ov, "pairs")
    vol.close()


@pytest.mark.parametrize("fallback", [False, True])
def test_two_frames_per_sweep_from_records(gpu, fallback):
    """k_integrate2 with both frames as records; and a pair one of whose poses does not see the whole grid: two launches."""
    poses = (lambda i: pose_close(i) if i == 1 else pose_outside(i)) if fallback else pose_outside
    expect = [False, True] if fallback else [True, True]
    run_pairs(poses, expect)


# ---- the first and the last pixel ------------------------------------------------------------------------------------

def test_first_and_last_pixel_with_nan_depth_there(gpu):
    """A pose from which voxels project to pixel 0 and to pixel W*H - 1 (checked below on the centres), a frame whose depth is
    NaN at exactly those two pixels, then frames with a depth there."""
    vol, sc = small_volume()
    ov = OracleVolume(vol._p)
    tr = pose_close(1)
    T = synth.cam_from_vol_f32(tr).reshape(3, 4).astype(np.float64)
    cx_, cy_, cz_ = (ov.centers(a).astype(np.float64) for a in range(3))
    g = np.stack(np.meshgrid(cx_, cy_, cz_, indexing="ij"), -1).reshape(-1, 3) @ T[:, :3].T + T[:, 3]
    u = np.trunc(g[:, 0] * sc.fx / g[:, 2] + sc.cx).astype(np.int64)
    v = np.trunc(g[:, 1] * sc.fy / g[:, 2] + sc.cy).astype(np.int64)
    ok = (g[:, 0] * sc.fx / g[:, 2] + sc.cx > 0.01) & (g[:, 1] * sc.fy / g[:, 2] + sc.cy > 0.01)  # (not the cell (-1, 0) that truncates to 0)
    assert ((u == 0) & (v == 0) & ok).any() and ((u == W - 1) & (v == H - 1)).any()
    assert ((u < 0) | (u >= W)).any()  # ... and some fall outside: pixel -1
    for i in range(3):
        dep, col = frame_for(tr, 300 + i)
        dep[0, 0] = dep[H - 1, W - 1] = np.nan if i == 0 else dep[1, 1]
        assert vol.integrateCloud(dep, col, tr, count=True) == ov.integrate_culled(dep, col, tr, synth.cam_from_vol_f32(tr))
        assert launch_info(vol)[0] == 0
    planes_equal(vol, ov, "pixel extremes")
    vol.close()


# ---- where the caller's two images lie --------------------------------------------------------------------------------

def test_caller_layouts_give_identical_planes(gpu):
    """bgra right behind depth, two allocations, bgra in FRONT of depth: the record pass reads them wherever they lie."""
    frames_ = [(pose_outside(i),) + frame_for(pose_outside(i), 400 + i) for i in range(3)]
    vol, sc = small_volume()
    ov = OracleVolume(vol._p)
    for tr, dep, col in frames_:
        ov.integrate_culled(dep, col, tr, synth.cam_from_vol_f32(tr))
    vol.close()
    for layout in ("behind", "separate", "in front"):
        vol, sc = small_volume()
        keep, sent = [], []
        for tr, dep, col in frames_:
            if layout == "separate":
                td = torch.from_numpy(dep).cuda()
                tc = torch.from_numpy(col).cuda()
                keep += [td, tc]
                dp, cp = td.data_ptr(), tc.data_ptr()
                sent.append((td, tc.view(-1).view(torch.float32).view(H, W)))
            else:
                t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
                zi, ci = (0, 1) if layout == "behind" else (1, 0)
                t[zi].copy_(torch.from_numpy(dep))
                t[ci].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
                keep.append(t)
                dp, cp = t[zi].data_ptr(), t[ci].data_ptr()
                sent.append((t[zi], t[ci]))
            torch.cuda.synchronize()
            vol.integrateCloudDevice(dp, cp, tr)
            assert launch_info(vol)[0] == 1
        vol.synchronize()
        planes_equal(vol, ov, layout)
        # the caller's images are as they were handed over
        for (td, tc), (tr, dep, col) in zip(sent, frames_):
            assert np.array_equal(td.cpu().numpy().view(np.uint32), dep.view(np.uint32))
            assert np.array_equal(tc.cpu().numpy().view(np.uint32).reshape(-1), col.view(np.uint32).reshape(-1))
        vol.close()


def test_the_handles_own_staged_frame(gpu):
    """integrateStaged after organize: depth / bgra are the handle's own [depth | bgra] staging."""
    vol, sc = small_volume()
    ov = OracleVolume(vol._p)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for i in range(3):
        tr = pose_outside(i)
        dep, col = frame_for(tr, 500 + i)
        z = np.nan_to_num(dep.astype(np.float64), nan=0.5)
        pts = np.stack([(uu - sc.cx) / sc.fx * z, (vv - sc.cy) / sc.fy * z, z], -1).reshape(-1, 3).astype(np.float32)
        d_st, c_st, n = vol.organize(pts, col.reshape(-1, 4))
        assert n > W * H // 2
        got = vol.integrateStaged(tr, count=True)
        assert got == ov.integrate_culled(d_st, c_st, tr, synth.cam_from_vol_f32(tr))
        assert launch_info(vol)[0] == 1
    planes_equal(vol, ov, "staged frame")
    vol.close()


def test_a_pair_with_bgra_in_front_of_depth_shares_the_sweep_and_ends_a_staged_frame(gpu):
    """Records need no layout: a pair whose colour images lie IN FRONT of their depth images (which the planar frame cannot
    address) still takes ONE sweep.  The staged-frame contract of include/tsdf_hip.h stays what it was (integrate_device[2]
    with a colour image that does not lie behind its depth image ends a staged frame), although nothing is repacked any more."""
    capi.set_tuning("fuse2", 2)
    vol, sc = small_volume()
    ov = OracleVolume(vol._p)
    pts = np.array([[0.0, 0.0, 0.3]], np.float32)
    vol.organize(pts, np.array([[1, 2, 3, 255]], np.uint8))
    keep, pair = [], []
    for i in range(2):
        tr = pose_outside(i)
        dep, col = frame_for(tr, 900 + i)
        t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
        t[0].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
        t[1].copy_(torch.from_numpy(dep))
        keep.append(t)
        pair.append((t[1].data_ptr(), t[0].data_ptr(), tr))
        ov.integrate_culled(dep, col, tr, synth.cam_from_vol_f32(tr))
    torch.cuda.synchronize()
    fused, _ = vol.integrateCloudDevice2(pair[0], pair[1])
    assert fused and launch_info(vol)[0] == 2
    vol.synchronize()
    planes_equal(vol, ov, "pair with bgra in front of depth")
    with pytest.raises(capi.TsdfHipError):
        vol.integrateStaged(pose_outside(0))
    vol.close()


# ---- stream order -----------------------------------------------------------------------------------------------------

def test_callers_buffers_are_overwritten_behind_the_launch_in_stream_order(gpu):
    """tsdf_hip_integrate_device without a count is asynchronous on the handle's stream.  The handle is put on a stream of the
    test's own, and on that stream, with NO host synchronisation from the first frame to the last: some milliseconds of
    unrelated work (so that everything below is queued while the GPU is still busy), then per frame -- the frame is copied
    device-to-device into ONE pair of caller buffers, the launch is queued from them, and the buffers are overwritten with
    other pixels right behind it.  Every frame goes through the same caller buffers and the same record slot.  Only then the
    stream is drained: each frame must have been integrated from its own pixels, which needs the record pass and the kernel on
    the handle's stream, in order, and the record slot not rewritten before the kernel that reads it is done."""
    vol, sc = small_volume()
    ov = OracleVolume(vol._p)
    pool = []
    for i in range(6):
        tr = pose_outside(i % 3)
        dep, col = frame_for(tr, 600 + i)
        ov.integrate_culled(dep, col, tr, synth.cam_from_vol_f32(tr))
        pool.append((torch.from_numpy(dep).cuda(), torch.from_numpy(col).cuda(), tr))
    junk_d = torch.full((H, W), 0.3, dtype=torch.float32, device="cuda")  # a surface through every pixel: it would move voxels
    junk_c = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda")
    buf_d = torch.empty((H, W), dtype=torch.float32, device="cuda")      # the caller's buffers: two allocations
    buf_c = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    ballast = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # everything above is resident; from here on the host waits for nothing
    stream = torch.cuda.Stream()
    vol.setStream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        for _ in range(40):
            ballast.mul_(1.0001)
        for pd, pc, tr in pool:
            buf_d.copy_(pd, non_blocking=True)
            buf_c.copy_(pc, non_blocking=True)
            vol.integrateCloudDevice(buf_d.data_ptr(), buf_c.data_ptr(), tr)
            assert launch_info(vol)[0] == 1
            buf_d.copy_(junk_d, non_blocking=True)
            buf_c.copy_(junk_c, non_blocking=True)
        busy = not stream.query()  # (report only: whether the queue was still running when the last frame had been queued)
    stream.synchronize()
    planes_equal(vol, ov, f"six frames queued back to back (stream still busy at the end of queueing: {busy})")
    vol.close()


# ---- what does not read records ---------------------------------------------------------------------------------------

def test_colourless_volume_still_matches_the_oracle(gpu):
    vol, sc = small_volume(color=False)
    ov = OracleVolume(vol._p)
    for i in range(3):
        tr = pose_outside(i)
        dep, _ = frame_for(tr, 700 + i)
        assert vol.integrateCloud(dep, None, tr, count=True) == ov.integrate_culled(dep, None, tr, synth.cam_from_vol_f32(tr))
        assert launch_info(vol)[0] == 1
    d, w, _ = vol.download()
    assert_same_f32(d, ov.d, "d")
    assert_same_f32(w, ov.w, "w")
    vol.close()


def test_plain_family_still_matches_the_oracle(gpu):
    capi.set_tuning("plain_kernel", 1)
    vol, sc = small_volume(layout=capi.LAYOUT_F32W)
    ov = OracleVolume(vol._p)
    for i in range(3):
        tr = pose_outside(i)
        dep, col = frame_for(tr, 800 + i)
        assert vol.integrateCloud(dep, col, tr, count=True) == ov.integrate_culled(dep, col, tr, synth.cam_from_vol_f32(tr))
    planes_equal(vol, ov, "plain kernel")
    vol.close()
