#!/usr/bin/env python3
"""Device time of mergeVolume (tsdf_hip_merge, csrc/tsdf_merge.hip): a 512^3 volume merged into a 512^3 volume (colour,
PACKED layout, a few frames fused into each from opposite sides) under the identity and under a 30 degree turn about (1, 2, 3);
beside it, for scale, `download` + `upload` of dst alone in the same process -- a floor under ANY route that takes the voxels
through the host, whatever it does with them there.

Every figure is the median of RUNS repetitions after WARMUP unrecorded ones.  Device time is tsdf_hip_merge_stats' (HIP events
on dst's stream around the kernel).  The bytes count what the rule has to move: dst's distance word and colour | count word
read and written for every merged voxel (16 bytes), and src's two planes once (8 bytes per voxel); the eight-fold gather is
served from cache or it is not -- the figure says which.  Repeating the merge changes dst's values, not the work: the gate
looks at src alone.  The host floor is a wall clock around calls that end in a synchronise.

usage: time_merge.py [--size 512] [--frames 4] [--runs 5] [--warmup 2] [--out profiles/merge_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpu_tsdf_amd import capi, synth  # noqa: E402
from cpu_tsdf_amd.volume import TSDFVolumeOctree  # noqa: E402


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def turn(axis, angle):
    """4 x 4 rotation by `angle` about `axis` (Rodrigues)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    return T


def fused_volume(res, frames, total, W=640, H=480):
    sc = synth.Scene(res * 2.0 ** -8, W, H)
    vol = TSDFVolumeOctree()
    vol.setResolution(res, res, res)
    vol.setGridSize(sc.size, sc.size, sc.size)
    vol.setImageSize(W, H)
    vol.setCameraIntrinsics(sc.fx, sc.fy, sc.cx, sc.cy)
    vol.setSensorDistanceBounds(0.0, 3.0 * sc.size)
    vol.setIntegrateColor(True)
    vol.reset()
    assert vol.getLayout() == capi.LAYOUT_PACKED
    for i in frames:
        tr = synth.turntable_pose(i, total, sc.size)
        vol.integrateCloud(sc.depth(tr), sc.bgra(i), tr)
    vol.synchronize()
    return vol


def time_merge(dst, src, T, runs, warmup):
    res = dst.getResolution()
    us, wall, stats = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        dst.mergeVolume(src, T)
        stats = dst.mergeStats()  # waits for the merge
        t1 = time.perf_counter()
        if r >= warmup:
            us.append(stats[3]), wall.append((t1 - t0) * 1e3)
    ms = median(us) / 1e3
    moved = 16 * stats[1] + 8 * res[0] * res[1] * res[2]
    return {"device_ms": ms, "call_and_wait_wall_ms": median(wall), "voxels_in_launch_box": stats[0], "voxels_merged": stats[1],
            "bytes_dst_rmw_plus_src_once": moved, "bytes_per_second": moved / (ms * 1e-3) if ms > 0 else None, "runs": runs, "warmup": warmup}


def time_host_floor(dst, runs, warmup):
    wall = []
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        d, w, rgb = dst.download()
        dst.upload(d, w, rgb)
        dst.synchronize()
        if r >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": median(wall), "runs": runs, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # noqa: F401  (before the library: capi._torch_first)
    if capi.load().tsdf_hip_device_count() <= 0:
        sys.exit("time_merge.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    res, n = a.size, a.frames
    out = {"tool": "tools/time_merge.py", "commit": head, "grid": f"{res}^3 into {res}^3", "frames_fused_each": n, "colour": True, "layout": "PACKED"}
    dst, src = fused_volume(res, range(n), 2 * n), fused_volume(res, range(n, 2 * n), 2 * n)
    for name, T in (("identity", np.eye(4)), ("turn_30_degrees", turn((1, 2, 3), np.pi / 6))):
        out[name] = time_merge(dst, src, T, a.runs, a.warmup)
        print(json.dumps({name: out[name]}), flush=True)
    out["download_plus_upload_of_dst"] = time_host_floor(dst, a.runs, 1)
    print(json.dumps({"download_plus_upload_of_dst": out["download_plus_upload_of_dst"]}), flush=True)
    dst.close()
    src.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
