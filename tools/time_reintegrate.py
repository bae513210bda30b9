#!/usr/bin/env python3
"""Time of reintegrateCloud (tsdf_hip_reintegrate_device, csrc/tsdf_reintegrate.hip) beside the two calls it replaces,
tsdf_hip_deintegrate_device under the old pose + tsdf_hip_integrate_device under the new one, IN THE SAME RUN ON THE SAME
HANDLE: PACKED layout with colour, a 640 x 480 frame resident on the device, grids of 512^3, 1024^3 and 2048^3 (a size whose
planes do not fit the device is skipped and reported as such), four other frames fused first.

The poses are the camera's pose and that pose under the correction of the tests (T . R_y(1.5 deg) . R_z(0.8 deg), T a
translation by (0.04, -0.013, 0.021) . size).  Two cameras per grid, the two of tools/time_deintegrate.py:
  turntable   the Scene A camera: the reference's frustum cull keeps every voxel; the sequence is the removal + the fast
              ALLIN integrate kernel;
  cull_bites  a principal point 60 % off centre and the camera yawed so that the grid sits beside the optical axis: the cull
              decides voxels.  The sequence is timed twice: with the integrate through k_integrate_plain (knob refcull_plain
              = 1: two plain sweeps, the regime DESIGN.md 3.21 quotes) and through the fast kernels' row intervals (the default).
A repetition re-poses old -> new and then new -> old, and likewise the sequence there and back, in turn, so the volume is the
same before every timed pair up to rounding and every side sees the same drift of the machine.  One sample is one direction:
a host clock around the call(s) and the synchronise that follows.  Every figure is the median of the samples of RUNS
repetitions after WARMUP unrecorded ones, with their minimum and maximum; for the fused call also the device time of
tsdf_hip_reintegrate_stats (HIP events on the stream around the kernel).  Nothing is counted in the timed calls.

usage: time_reintegrate.py [--sizes 512,1024,2048] [--runs 7] [--warmup 3] [--out profiles/reintegrate_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cpu_tsdf_amd import capi  # noqa: E402
from time_deintegrate import H, W, make, median, pose, timed  # noqa: E402


def correction(S):
    a, b = np.deg2rad(1.5), np.deg2rad(0.8)
    ry = np.eye(4)
    ry[0, 0], ry[0, 2], ry[2, 0], ry[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    rz = np.eye(4)
    rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = np.cos(b), -np.sin(b), np.sin(b), np.cos(b)
    t = np.eye(4)
    t[:3, 3] = (0.04 * S, -0.013 * S, 0.021 * S)
    return t @ ry @ rz


def one_camera(res, off_centre, runs, warmup, torch):
    vol, sc = make(res, off_centre)
    for i in (0, 2, 4, 6):   # content: four other frames
        tr = pose(sc, i, off_centre)
        vol.integrateCloud(sc.depth(tr), sc.bgra(i), tr)
    old = pose(sc, 1, off_centre)
    new = correction(sc.size) @ old
    dep, col = sc.depth(old), sc.bgra(1)
    t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    t[0].copy_(torch.from_numpy(dep))
    t[1].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
    torch.cuda.synchronize()
    dp, cp = t[0].data_ptr(), t[1].data_ptr()
    vol.integrateCloudDevice(dp, cp, old)   # the frame to be re-posed
    counts = vol.reintegrateCloudDevice(dp, cp, old, new, count=True)
    stats = vol.reintegrateStats()
    vol.reintegrateCloudDevice(dp, cp, new, old)

    def sequence(a, b):
        vol.deintegrateCloudDevice(dp, cp, a)
        vol.integrateCloudDevice(dp, cp, b)

    sides = [("sequence_fast_kernels", 0)] + ([("sequence_k_integrate_plain", 1)] if off_centre else [])
    ms = {name: [] for name, _ in sides}
    ms["reintegrate"], dev = [], []
    try:
        for r in range(warmup + runs):
            for name, knob in sides:   # alternating: every side sees the same drift of the machine
                capi.set_tuning("refcull_plain", knob)
                for a, b in ((old, new), (new, old)):
                    x = timed(lambda: vol.reintegrateCloudDevice(dp, cp, a, b), vol)
                    us = vol.reintegrateStats()[5]
                    if r >= warmup:
                        ms["reintegrate"].append(x), dev.append(us / 1e3)
                for a, b in ((old, new), (new, old)):
                    y = timed(lambda: sequence(a, b), vol)
                    if r >= warmup:
                        ms[name].append(y)
    finally:
        capi.set_tuning("refcull_plain", 0)
    vol.close()
    out = {"selected_by_old": stats[0], "weights_lowered": int(counts[0]), "cleared": stats[2], "observed_by_new": int(counts[1]),
           "selected_by_both": stats[4], "runs": runs, "warmup": warmup, "samples_per_figure": len(ms["reintegrate"]),
           "reintegrate_device_ms": median(dev), "reintegrate_device_ms_min_max": [min(dev), max(dev)]}
    for name in ms:
        out[name + "_call_and_wait_ms"] = median(ms[name])
        out[name + "_call_and_wait_ms_min_max"] = [min(ms[name]), max(ms[name])]
    for name, _ in sides:
        out["reintegrate_over_" + name] = out["reintegrate_call_and_wait_ms"] / out[name + "_call_and_wait_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reintegrate_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # (before the library: capi._torch_first)
    capi.use_test_library()  # the same translation units plus tsdf_hip_set_tuning: the knob refcull_plain changes between timed calls
    if capi.load().tsdf_hip_device_count() <= 0:
        sys.exit("time_reintegrate.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_reintegrate.py", "commit": head, "frame": f"{W}x{H}", "colour": True, "layout": "PACKED", "grids": {}}
    free = torch.cuda.mem_get_info()[0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for res in [int(s) for s in a.sizes.split(",") if s]:
        need = 8 * res ** 3 + (1 << 30)   # d and the colour | count word, and room for the rest
        if need > free:
            out["grids"][f"{res}^3"] = {"skipped": f"{need} bytes needed, {free} free"}
            print(json.dumps({f"{res}^3": out["grids"][f"{res}^3"]}), flush=True)
            continue
        g = out["grids"][f"{res}^3"] = {}
        for name, off in (("turntable", False), ("cull_bites", True)):
            g[name] = one_camera(res, off, a.runs, a.warmup, torch)
            print(json.dumps({f"{res}^3 {name}": g[name]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
