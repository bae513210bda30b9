#!/usr/bin/env python3
"""Time of castRays (tsdf_hip_cast_rays_device, csrc/tsdf_castrays.hip) and the measurement that decides its ray order
(DESIGN.md 3.23): PACKED layout with colour, grids of 512^3, 1024^3 and 2048^3 (a size whose planes do not fit the device is
skipped and reported as such) fused from six 640 x 480 frames, and the 307 200 rays of a 640 x 480 view of that volume, computed
on the host in renderView's operation order and resident on the device.  Four variants, in turn within every repetition so
that each sees the same drift of the machine:
  a  image order with TSDF_HIP_RAYS_AS_GIVEN       (beside renderView of the same view in the same run)
  b  image order without the flag                  (the library's default order)
  c  the same rays under a fixed random permutation, with the flag
  d  the permuted rays without the flag
One sample is the device time of tsdf_hip_cast_rays_stats: HIP events on the handle's stream around the call's kernels, the
key kernel and the sort included where the library orders the rays.  renderView is a host clock around tsdf_hip_raycast into
pinned memory and the wait -- its kernel plus the read-back of the 9.8 MB image, which the device form of castRays does not
make.  Every figure is the median of RUNS samples after WARMUP unrecorded ones, with their minimum and maximum.  The results
of all four variants are compared byte for byte with renderView's before anything is timed.
The decision rule, evaluated over the recorded runs and written into the file:
  ordered_path_wins    d is faster than c at every size and their min-max intervals do not overlap
  as_given_pays        b is slower than a at some size and their min-max intervals do not overlap
profiles/castrays_timing.json is the run that decided: the library then sorted the rays by a Morton key of their entry cell
when the flag was absent, d did not beat c, and that path was deleted.  On the library as it is the flag
changes nothing, so b repeats a and d repeats c; the four variants stay so that a new ordering can be judged by the same rule.

usage: time_castrays.py [--sizes 512,1024,2048] [--runs 9] [--warmup 3] [--out profiles/castrays_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cpu_tsdf_amd import capi, synth  # noqa: E402
from time_deintegrate import H, W, make, median, timed  # noqa: E402


def view_rays(p, trans):
    """Origin and rotated direction of every pixel of renderView(trans, 1), float32, in ray_direction's operation order."""
    rot = trans[:3, :3].astype(np.float32)
    x = np.tile(np.arange(W, dtype=np.float64), H)
    y = np.repeat(np.arange(H, dtype=np.float64), W)
    a = ((x - p.cx) / p.fx).astype(np.float32)
    b = ((y - p.cy) / p.fy).astype(np.float32)
    c = np.ones_like(a)
    n = np.sqrt(a * a + (b * b + c * c))
    a, b, c = a / n, b / n, c / n
    du = np.stack([rot[k, 0] * a + (rot[k, 1] * b + rot[k, 2] * c) for k in range(3)], axis=1).astype(np.float32)
    org = np.tile(trans[:3, 3].astype(np.float32), (len(du), 1))
    return np.ascontiguousarray(org), np.ascontiguousarray(du)


def one_grid(res, runs, warmup, torch):
    vol, sc = make(res, False)
    for i in range(6):
        tr = synth.turntable_pose(i, 8, sc.size)
        vol.integrateCloud(sc.depth(tr), sc.bgra(i), tr)
    tr = np.asarray(synth.turntable_pose(1, 8, sc.size), np.float64)
    org, du = view_rays(vol._p, tr)
    n = len(du)
    perm = np.random.RandomState(0).permutation(n)
    dev = {"image": (torch.from_numpy(org).cuda(), torch.from_numpy(du).cuda()),
           "permuted": (torch.from_numpy(org[perm]).cuda(), torch.from_numpy(du[perm]).cuda())}
    t_out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    variants = {"a_image_as_given": ("image", True), "b_image_default": ("image", False),
                "c_permuted_as_given": ("permuted", True), "d_permuted_default": ("permuted", False)}

    def cast(which, as_given):
        o, d = dev[which]
        vol.castRaysDevice(o.data_ptr(), d.data_ptr(), 0, n, t_out.data_ptr(), as_given=as_given)

    want = vol.renderView(tr, 1, camera_frame=False, pinned=True).reshape(-1, 8).copy()
    identical = True
    for name, (which, as_given) in variants.items():
        cast(which, as_given)
        vol.synchronize()
        got = t_out.cpu().numpy()
        ref = want if which == "image" else want[perm]
        identical = identical and bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    hits = vol.castRaysStats()[1]
    us = {name: [] for name in variants}
    view_ms = []
    for r in range(warmup + runs):
        for name, (which, as_given) in variants.items():
            cast(which, as_given)
            x = vol.castRaysStats()[3]
            if r >= warmup:
                us[name].append(x / 1e3)
        y = timed(lambda: vol.renderView(tr, 1, camera_frame=False, pinned=True), vol)
        if r >= warmup:
            view_ms.append(y)
    vol.close()
    out = {"rays": n, "hits": hits, "equal_to_renderView_byte_for_byte": identical, "runs": runs, "warmup": warmup,
           "renderView_call_and_wait_ms": median(view_ms), "renderView_call_and_wait_ms_min_max": [min(view_ms), max(view_ms)]}
    for name in variants:
        out[name + "_device_ms"] = median(us[name])
        out[name + "_device_ms_min_max"] = [min(us[name]), max(us[name])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "castrays_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # (before the library: capi._torch_first)
    if capi.load().tsdf_hip_device_count() <= 0:
        sys.exit("time_castrays.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_castrays.py", "commit": head, "view": f"{W}x{H}", "colour": True, "layout": "PACKED", "grids": {}}
    free = torch.cuda.mem_get_info()[0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for res in [int(s) for s in a.sizes.split(",") if s]:
        need = 8 * res ** 3 + (1 << 30)   # d and the colour | count word, and room for the rest
        if need > free:
            out["grids"][f"{res}^3"] = {"skipped": f"{need} bytes needed, {free} free"}
            print(json.dumps({f"{res}^3": out["grids"][f"{res}^3"]}), flush=True)
            continue
        g = out["grids"][f"{res}^3"] = one_grid(res, a.runs, a.warmup, torch)
        print(json.dumps({f"{res}^3": g}), flush=True)
    done = [g for g in out["grids"].values() if "skipped" not in g]
    out["decision"] = {
        "ordered_path_wins": bool(done) and all(g["d_permuted_default_device_ms_min_max"][1] < g["c_permuted_as_given_device_ms_min_max"][0] for g in done),
        "as_given_pays": any(g["b_image_default_device_ms_min_max"][0] > g["a_image_as_given_device_ms_min_max"][1] for g in done)}
    print(json.dumps({"decision": out["decision"]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
