#!/usr/bin/env python3
"""Device time of shiftVolume (tsdf_hip_shift, csrc/tsdf_shift.hip) at 512^3 and 2048^3 (colour, PACKED layout, a few frames
fused so that the band flags are carried) for the shifts (0,0,1), (0,4,0), (64,0,0) and (5,3,2): one launch per plane, one
per row batch, the in-row kernel, and all three axes at once; beside it, at 512^3, the only route there was before --
`download`, a roll with fill on the host, `upload` -- for the same shift in the same process.

Every figure is the median of RUNS repetitions after WARMUP unrecorded ones.  Device time is tsdf_hip_shift_stats' (HIP events
on the handle's stream around the shift); the bytes count every voxel array once read and once written (PACKED + colour: the
distance word and the colour | count word, 8 bytes per voxel each way); the host route is a wall clock around calls that end
in a synchronise.

usage: time_shift.py [--sizes 512,2048] [--frames 4] [--runs 5] [--warmup 2] [--out profiles/shift_timing.json]"""
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

SHIFTS = [(0, 0, 1), (0, 4, 0), (64, 0, 0), (5, 3, 2)]


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def fused_volume(res, n_frames, W=640, H=480):
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
    for i in range(n_frames):
        tr = synth.turntable_pose(i, n_frames, sc.size)
        vol.integrateCloud(sc.depth(tr), sc.bgra(i), tr)
    vol.synchronize()
    return vol


def time_shift(vol, s, runs, warmup):
    """The shift and its inverse alternate, so that the volume never runs empty; both directions cost the same launches."""
    res = vol.getResolution()
    us, wall, stats = [], [], None
    for r in range(warmup + runs):
        step = s if r % 2 == 0 else tuple(-v for v in s)
        t0 = time.perf_counter()
        vol.shiftVolume(*step)
        stats = vol.shiftStats()  # waits for the shift
        t1 = time.perf_counter()
        if r >= warmup:
            us.append(stats[3]), wall.append((t1 - t0) * 1e3)
    ms = median(us) / 1e3
    moved = 2 * 8 * res[0] * res[1] * res[2]  # d + (rgb | count), read once and written once
    return {"device_ms": ms, "call_and_wait_wall_ms": median(wall), "bytes_read_plus_written": moved,
            "bytes_per_second": moved / (ms * 1e-3) if ms > 0 else None, "flags_carried": stats[2], "runs": runs, "warmup": warmup}


def roll_fill(a, s, fill):
    out = np.empty_like(a)
    out[...] = fill
    n = a.shape[:3][::-1]
    lo = [max(0, -v) for v in s]
    hi = [min(m, m - v) for m, v in zip(n, s)]
    if all(l < h for l, h in zip(lo, hi)):
        out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = a[lo[2] + s[2]:hi[2] + s[2], lo[1] + s[1]:hi[1] + s[1], lo[0] + s[0]:hi[0] + s[0]]
    return out


def time_host_route(vol, s, runs, warmup):
    wall = []
    for r in range(warmup + runs):
        step = s if r % 2 == 0 else tuple(-v for v in s)
        t0 = time.perf_counter()
        d, w, rgb = vol.download()
        vol.upload(roll_fill(d, step, -1.0), roll_fill(w, step, 0.0), roll_fill(rgb, step, 0))
        vol.synchronize()
        if r >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": median(wall), "runs": runs, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-route-at", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shift_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # noqa: F401  (before the library: capi._torch_first)
    if capi.load().tsdf_hip_device_count() <= 0:
        sys.exit("time_shift.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_shift.py", "commit": head, "frames_fused": a.frames, "colour": True, "layout": "PACKED"}
    for res in [int(v) for v in a.sizes.split(",") if v]:
        vol = fused_volume(res, a.frames)
        e = {}
        for s in SHIFTS:
            k = "shift(%d,%d,%d)" % s
            e[k] = time_shift(vol, s, a.runs, a.warmup)
            print(json.dumps({f"{res}^3": {k: e[k]}}), flush=True)
        if res == a.host_route_at:  # after the device runs: upload() drops the flags
            for s in SHIFTS:
                k = "shift(%d,%d,%d)" % s
                e[k]["download_roll_upload"] = time_host_route(vol, s, a.runs, 1)
                e[k]["speedup_over_download_roll_upload"] = e[k]["download_roll_upload"]["wall_ms"] / e[k]["call_and_wait_wall_ms"]
                print(json.dumps({f"{res}^3": {k: e[k]}}), flush=True)
        vol.close()
        out[f"{res}^3"] = e
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
