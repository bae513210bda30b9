#!/usr/bin/env python3
"""alignCloud's fused reduction against what the tree offered before it, in the same run on the same volume: Scene A fused
at 512^3 from 20 frames, one 640 x 480 frame back-projected, a pose a few voxels off.

  fused        one tsdf_hip_align_system_device call on the device-resident cloud: device time by the handle's stream
               events (tsdf_hip_align_stats) and wall clock, and a 10-iteration tsdf_hip_align (upload included)
  sample+numpy the best path of the parent commit: transform on the host, vol.sample (value + gradient: 16 B per point
               come back), the gate's value test and the 29 sums in numpy -- wall clock
  per point    the C++ drop-in's getFxnAndGradient once per point (tools/time_align.cpp), on 2 000 points -- wall clock

Median of RUNS repetitions after WARMUP.  No threshold: the numbers and their ratio go to the JSON.

usage: time_align.py [--res 512] [--frames 20] [--runs 7] [--warmup 2] [--loop-points 2000] [--out profiles/align_timing.json]"""
import argparse
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpu_tsdf_amd import build as b  # noqa: E402
from cpu_tsdf_amd import capi, synth  # noqa: E402
from cpu_tsdf_amd.volume import backproject  # noqa: E402
from tools.time_occupied import fused_volume, median  # noqa: E402

F64P = C.POINTER(C.c_double)
R_MAX = 0.9


def se3_exp(xi):
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, bb, c = (1.0, 0.5, 1.0 / 6.0) if th < 1e-12 else (np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3)
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * K + bb * (K @ K)
    E[:3, 3] = (np.eye(3) + bb * K + c * (K @ K)) @ v
    return E


def sample_numpy(vol, pts, T):
    """One system the way the parent commit allows: the sums of tsdf_hip_align_system with min_weight < 0 (the weights never
    leave the device on this path)."""
    m = T[:3].astype(np.float32)
    q = np.empty_like(pts)
    for r in range(3):
        q[:, r] = ((m[r, 0] * pts[:, 0] + m[r, 1] * pts[:, 1]) + m[r, 2] * pts[:, 2]) + m[r, 3]
    ok, val, grad, _ = vol.sample(q, want_hess=False)
    use = ok & (np.abs(val) < np.float32(R_MAX))
    q, g, r = q[use].astype(np.float64), grad[use].astype(np.float64), val[use].astype(np.float64)
    J = np.concatenate([np.cross(q, g), g], 1)
    A, bvec = J.T @ J, J.T @ r
    return np.concatenate([A[np.triu_indices(6)], bvec, [r @ r, float(len(r))]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-points", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # (before the library: capi._torch_first)
    lib = capi.load()
    if lib.tsdf_hip_device_count() <= 0:
        sys.exit("time_align.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    W, H = 640, 480
    vol = fused_volume(a.res, a.frames, W, H)
    h = vol._need()
    sc = synth.Scene(a.res * 2.0 ** -8, W, H)
    T_star = synth.turntable_pose(3.5, a.frames, sc.size, tilt=0.1)
    depth = sc.depth(T_star)
    pts = backproject(depth, sc.fx, sc.fy, sc.cx, sc.cy)
    voxel = sc.size / a.res
    guess = se3_exp(np.concatenate([0.01 * np.array([0.6, -0.5, 0.62]), 3 * voxel * np.array([0.5, 0.7, -0.5])])) @ T_star
    T12 = np.ascontiguousarray(guess[:3]).reshape(12)
    n = len(pts)
    d_pts = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    out, st = np.empty(29), (C.c_uint64 * 4)()
    dev_us, wall_ms = [], []
    for r in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        capi.check(lib.tsdf_hip_align_system_device(h, d_pts.data_ptr(), n, T12.ctypes.data_as(F64P), -1.0, R_MAX, out.ctypes.data_as(F64P)),
                   "align_system_device")
        t1 = time.perf_counter()
        capi.check(lib.tsdf_hip_align_stats(h, st), "align_stats")
        if r >= a.warmup:
            dev_us.append(float(st[3]))
            wall_ms.append((t1 - t0) * 1e3)
    fused_out = out.copy()
    old_ms = []
    for r in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        old = sample_numpy(vol, pts, guess)
        if r >= a.warmup:
            old_ms.append((time.perf_counter() - t0) * 1e3)
    assert old[28] == fused_out[28], (old[28], fused_out[28])
    assert np.allclose(old, fused_out, rtol=1e-9, atol=1e-9 * np.abs(fused_out).max())
    al_ms, al_dev = [], []
    for r in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        T, it, log = vol.alignCloud(pts, guess, max_iterations=10, min_step=0.0)
        t1 = time.perf_counter()
        capi.check(lib.tsdf_hip_align_stats(h, st), "align_stats")
        if r >= a.warmup:
            al_ms.append((t1 - t0) * 1e3)
            al_dev.append(float(st[3]))
    res = {"tool": "tools/time_align.py", "commit": head, "res": a.res, "frames_fused": a.frames, "points": n, "used": int(fused_out[28]),
           "runs": a.runs, "warmup": a.warmup,
           "fused_system_device_us": median(dev_us), "fused_system_wall_ms": median(wall_ms),
           "sample_plus_numpy_wall_ms": median(old_ms),
           "sample_plus_numpy_over_fused_wall": median(old_ms) / median(wall_ms),
           "align_10_iterations_wall_ms": median(al_ms), "align_10_iterations_device_us": median(al_dev), "align_iterations": it,
           "align_cost_per_point_first_last": [float(log[0, 0] / log[0, 1]), float(log[-1, 0] / log[-1, 1])]}
    vol.close()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_align")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                              [os.path.join(ROOT, "tools", "time_align.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                               "-Wl,-rpath," + b.LIBDIR, "-o", exe])
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<6q", a.res, W, H, a.frames, n, 10))
            f.write(struct.pack("<5d", sc.size, sc.fx, sc.fy, sc.cx, sc.cy))
            for i in range(a.frames):
                tr = synth.turntable_pose(i, a.frames, sc.size)
                f.write(np.ascontiguousarray(tr, np.float64).tobytes())
                f.write(np.ascontiguousarray(sc.depth(tr), np.float32).tobytes())
            f.write(pts.tobytes())
            f.write(np.ascontiguousarray(guess, np.float64).tobytes())
        res["cpp_drop_in"] = json.loads(subprocess.check_output([exe, path, str(a.loop_points)], text=True, timeout=900).strip().splitlines()[-1])
    res["per_point_loop_extrapolated_to_the_frame_ms"] = res["cpp_drop_in"]["per_point_us"] * n / 1000.0
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
