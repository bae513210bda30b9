#!/usr/bin/env python3
"""Time of deintegrateCloud (tsdf_hip_deintegrate_device, csrc/tsdf_deintegrate.hip) beside tsdf_hip_integrate_device of the
SAME frame on the SAME handle: PACKED layout with colour, 640 x 480 frames resident on the device, grids of 512^3, 1024^3 and
2048^3 (a size whose planes do not fit the device is skipped and reported as such).

Two cameras per grid:
  turntable   the Scene A camera: the reference's frustum cull keeps every voxel, integrate runs its fast ALLIN kernel and
              the removal tests no planes;
  cull_bites  a principal point 60 % off centre and the camera yawed so that the grid sits beside the optical axis: the cull
              decides voxels.  Here integrate is timed twice -- through k_integrate_plain (knob refcull_plain = 1: the per-voxel
              kernel k_deintegrate is modelled on, the comparison DESIGN.md 3.21 quotes) and through the fast kernels' row
              intervals (the default) -- and the removal tests the six planes per voxel like k_integrate_plain.
A repetition integrates the frame and takes it out again, so the volume is the same before every timed call (four other
frames are fused first).  Every figure is the median of RUNS repetitions after WARMUP unrecorded ones: a host clock around the
call and the synchronise that follows it, for both sides alike, and for the removal also the device time of
tsdf_hip_deintegrate_stats (HIP events on the stream around the kernel).  Nothing is counted in the timed calls.  The bytes are
what the rule moves at least: per selected voxel the distance word and the colour | count word read and the latter written
(12 bytes; the distance is written only where it moved).

usage: time_deintegrate.py [--sizes 512,1024,2048] [--runs 7] [--warmup 3] [--out profiles/deintegrate_timing.json]"""
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

W, H = 640, 480


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def make(res, off_centre):
    sc = synth.Scene(res * 2.0 ** -8, W, H)
    if off_centre:
        sc.cx += 0.6 * W / 2
    vol = TSDFVolumeOctree()
    vol.setResolution(res, res, res)
    vol.setGridSize(sc.size, sc.size, sc.size)
    vol.setImageSize(W, H)
    vol.setCameraIntrinsics(sc.fx, sc.fy, sc.cx, sc.cy)
    vol.setSensorDistanceBounds(0.0, 3.0 * sc.size)
    vol.setIntegrateColor(True)
    vol.reset()
    assert vol.getLayout() == capi.LAYOUT_PACKED
    return vol, sc


def pose(sc, i, off_centre):
    tr = synth.turntable_pose(i, 8, sc.size)
    if off_centre:
        psi = float(np.arctan(0.6 * (W / 2) / sc.fx))
        yaw = np.eye(4)
        yaw[0, 0], yaw[0, 2], yaw[2, 0], yaw[2, 2] = np.cos(psi), np.sin(psi), -np.sin(psi), np.cos(psi)
        tr = tr @ yaw
    return tr


def timed(call, vol):
    vol.synchronize()
    t0 = time.perf_counter()
    call()
    vol.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one_camera(res, off_centre, runs, warmup, torch):
    vol, sc = make(res, off_centre)
    for i in (0, 2, 4, 6):   # content: four other frames
        tr = pose(sc, i, off_centre)
        vol.integrateCloud(sc.depth(tr), sc.bgra(i), tr)
    tr = pose(sc, 1, off_centre)
    dep, col = sc.depth(tr), sc.bgra(1)
    t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    t[0].copy_(torch.from_numpy(dep))
    t[1].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
    torch.cuda.synchronize()
    dp, cp = t[0].data_ptr(), t[1].data_ptr()
    selected = vol.integrateCloudDevice(dp, cp, tr, count=True)
    removed = vol.deintegrateCloudDevice(dp, cp, tr, count=True)
    sides = [("integrate_fast_kernels", 0)] + ([("integrate_k_integrate_plain", 1)] if off_centre else [])
    ms = {name: [] for name, _ in sides}
    ms["deintegrate"], dev = [], []
    try:
        for r in range(warmup + runs):
            for name, knob in sides:   # alternating: every side sees the same drift of the machine
                capi.set_tuning("refcull_plain", knob)
                a = timed(lambda: vol.integrateCloudDevice(dp, cp, tr), vol)
                b = timed(lambda: vol.deintegrateCloudDevice(dp, cp, tr), vol)
                us = vol.deintegrateStats()[3]
                if r >= warmup:
                    ms[name].append(a), ms["deintegrate"].append(b), dev.append(us / 1e3)
    finally:
        capi.set_tuning("refcull_plain", 0)
    vol.close()
    out = {"voxels_selected": int(selected), "weights_lowered": int(removed), "runs": runs, "warmup": warmup,
           "deintegrate_device_ms": median(dev), "deintegrate_device_ms_min_max": [min(dev), max(dev)],
           "bytes_at_least": 12 * int(selected)}
    for name in ms:
        out[name + "_call_and_wait_ms"] = median(ms[name])
        out[name + "_call_and_wait_ms_min_max"] = [min(ms[name]), max(ms[name])]
    out["bytes_per_second_at_least"] = out["bytes_at_least"] / (out["deintegrate_device_ms"] * 1e-3) if out["deintegrate_device_ms"] > 0 else None
    base = "integrate_k_integrate_plain" if off_centre else "integrate_fast_kernels"
    out["deintegrate_over_" + base] = out["deintegrate_call_and_wait_ms"] / out[base + "_call_and_wait_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deintegrate_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # (before the library: capi._torch_first)
    capi.use_test_library()  # the same translation units plus tsdf_hip_set_tuning: the knob refcull_plain changes between timed calls
    if capi.load().tsdf_hip_device_count() <= 0:
        sys.exit("time_deintegrate.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_deintegrate.py", "commit": head, "frame": f"{W}x{H}", "colour": True, "layout": "PACKED", "grids": {}}
    free = torch.cuda.mem_get_info()[0]
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
