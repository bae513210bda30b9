#!/usr/bin/env python3
"""Device time of computeDistanceField (tsdf_hip_esdf, csrc/tsdf_esdf.hip): a synthetic scene (cpu_tsdf_amd/synth.py) fused
into a 256^3 and a 512^3 volume (colour, PACKED layout), then the whole-grid distance field, unlimited and truncated at 16
voxels.  Beside it, for scale: `download` of the volume alone -- the first step of ANY host transform -- and, where SciPy can
be imported, scipy.ndimage.distance_transform_edt on the downloaded site mask.

Every GPU figure is the median of RUNS repetitions after WARMUP unrecorded ones; device time is tsdf_hip_esdf_stats' (HIP
events around the three passes).  The bytes are the kernels' own count (the header of csrc/tsdf_esdf.hip): per voxel, pass x
reads d (4) and the colour | count word (4) and writes d2 (4) and a sign bit (1/8); the passes along y and z read and write
d2 (8 each); envelope traffic is not counted, so the rate is a lower bound on what moved and no roofline claim.  The fraction
is of 8 TB/s.  Report-only numbers: nothing here asserts.

usage: time_esdf.py [--sizes 256 512] [--frames 4] [--runs 5] [--warmup 2] [--out profiles/esdf_timing.json]"""
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

PEAK = 8e12  # bytes per second


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def fused_volume(res, frames, W=640, H=480):
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
    for i in range(frames):
        tr = synth.turntable_pose(i, 2 * frames, sc.size)
        vol.integrateCloud(sc.depth(tr), sc.bgra(i), tr)
    vol.synchronize()
    return vol


def time_esdf(vol, r_max, runs, warmup):
    us, wall, stats = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        vol.computeDistanceField(r_max)
        t1 = time.perf_counter()
        stats = vol.distanceFieldStats()
        if r >= warmup:
            us.append(stats[3]), wall.append((t1 - t0) * 1e3)
    ms = median(us) / 1e3
    moved = stats[0] * (4 + 4 + 4 + 8 + 8) + stats[0] // 8
    rate = moved / (ms * 1e-3) if ms > 0 else None
    return {"device_ms": ms, "call_wall_ms": median(wall), "voxels": stats[0], "sites": stats[1], "bytes_held_field_plus_scratch": stats[2],
            "bytes_moved_kernels_own_count": moved, "bytes_per_second": rate, "fraction_of_8_TB_per_s": rate / PEAK if rate else None,
            "runs": runs, "warmup": warmup}


def site_mask(d, w):
    """The rule of include/tsdf_hip.h on whole-grid arrays, min_weight 0."""
    c = np.where((w > 0) & ~np.isnan(d), np.where(d < 0, 2, 1), 0).astype(np.int8)
    site = np.zeros(c.shape, bool)
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = (c[a] != 0) & (c[b] != 0) & (c[a] != c[b])
        site[a] |= cross
        site[b] |= cross
    return site


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # noqa: F401  (before the library: capi._torch_first)
    if capi.load().tsdf_hip_device_count() <= 0:
        sys.exit("time_esdf.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    try:
        from scipy import ndimage
    except Exception:  # noqa: BLE001
        ndimage = None
    out = {"tool": "tools/time_esdf.py", "commit": head, "frames_fused": a.frames, "colour": True, "layout": "PACKED", "grids": {}}
    for res in a.sizes:
        vol = fused_volume(res, a.frames)
        g = {"unlimited": time_esdf(vol, 0, a.runs, a.warmup), "r_max_16": time_esdf(vol, 16, a.runs, a.warmup)}
        wall = []
        for r in range(1 + a.runs):
            t0 = time.perf_counter()
            d, w, _ = vol.download(want_rgb=False)
            if r >= 1:
                wall.append((time.perf_counter() - t0) * 1e3)
        g["download_d_and_w_alone"] = {"wall_ms": median(wall), "runs": a.runs, "warmup": 1}
        if ndimage is not None:
            mask = site_mask(d, w)
            t0 = time.perf_counter()
            ndimage.distance_transform_edt(~mask)
            g["scipy_distance_transform_edt_on_the_host"] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "runs": 1, "sites": int(mask.sum())}
        else:
            g["scipy_distance_transform_edt_on_the_host"] = None
        vol.close()
        out["grids"][f"{res}^3"] = g
        print(json.dumps({f"{res}^3": g}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
