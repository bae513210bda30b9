#!/usr/bin/env python3
"""The `integrate` program's --flatten on the host (cpu_tsdf::mesh_post::flattenVertices, one thread) against the GPU pass
(tsdf_hip_mesh_flatten, csrc/tsdf_flatten.hip), on the SAME fetched mesh in the same run: Scene A fused at 512^3.

Per size: the marching-cubes mesh is fetched once; tools/time_flatten.cpp (compiled here against the drop-in) times both
passes, wall clock, on prefixes of it and on the full mesh (the mesh is in Morton order: a prefix is a compact piece of
surface) -- this is what the program pays: upload, device pass, download and the host's tail included -- and where the
crossover of mesh_post::kFlattenHostBelowVertices shows; then tsdf_hip_march_flatten on the device-resident mesh, by HIP
events (tsdf_hip_mesh_flatten_stats), median of RUNS repetitions after WARMUP.  The host pass is the yardstick: timed on the
same host in the same run.

usage: time_flatten.py [--sizes 512] [--frames 20] [--runs 5] [--warmup 2] [--host-max 3000000] [--prefix-max 3000000]
                       [--out profiles/flatten_timing.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpu_tsdf_amd import build as b  # noqa: E402
from cpu_tsdf_amd import capi  # noqa: E402
from tools.time_occupied import fused_volume, median  # noqa: E402

MIN_DIST = 0.0001  # the program's default (src/prog/integrate.cpp:103)


def build_timer(tmp):
    exe = os.path.join(tmp, "time_flatten")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tools", "time_flatten.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                           "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def device_resident(vol, runs, warmup):
    """tsdf_hip_march + tsdf_hip_march_flatten: the soup never leaves the GPU."""
    lib, h = capi.load(), vol._need()
    dev, st = [], None
    for r in range(warmup + runs):
        n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(lib.tsdf_hip_march(h, 2.0, 0, C.byref(n)), "march")
        capi.check(lib.tsdf_hip_march_flatten(h, MIN_DIST, C.byref(m), C.byref(k)), "march_flatten")
        st = (C.c_uint64 * 4)()
        capi.check(lib.tsdf_hip_mesh_flatten_stats(st), "mesh_flatten_stats")
        if r >= warmup:
            dev.append(st[3] / 1000.0)
    ms, cells = (C.c_float * 3)(), C.c_uint64(0)
    capi.check(lib.tsdf_hip_march_timing(h, ms, C.byref(cells)), "march_timing")
    return {"vertices": int(st[0]), "vertices_out": int(st[1]), "faces": int(n.value), "faces_out": int(k.value), "rounds": int(st[2]),
            "flatten_device_ms": median(dev), "march_device_ms": float(sum(ms)), "runs": runs, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-max", type=int, default=3000000, help="largest prefix (faces) the one-thread host pass is timed on")
    ap.add_argument("--prefix-max", type=int, default=3000000, help="largest prefix (faces) handed to the program path at all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flatten_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # noqa: F401  (before the library: capi._torch_first)
    lib = capi.load()
    if lib.tsdf_hip_device_count() <= 0:
        sys.exit("time_flatten.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_flatten.py", "commit": head, "frames_fused": a.frames, "min_dist": MIN_DIST}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_timer(tmp)
        for res in [int(s) for s in a.sizes.split(",") if s]:
            vol = fused_volume(res, a.frames)
            h = vol._need()
            n = C.c_uint64(0)
            capi.check(lib.tsdf_hip_march(h, 2.0, 0, C.byref(n)), "march")
            nt = int(n.value)
            verts = np.empty((nt, 9), np.float32)
            capi.check(lib.tsdf_hip_march_fetch(h, capi.as_f32p(verts), None, None), "march_fetch")
            e = {"device_resident": device_resident(vol, a.runs, a.warmup)}
            vol.close()
            path = os.path.join(tmp, f"mesh{res}.bin")
            n_file = min(nt, a.prefix_max)  # (the timing program builds a PolygonMesh per pass: host memory, not the GPU, bounds it)
            with open(path, "wb") as f:
                f.write(np.int64(n_file).tobytes())
                f.write(verts[:n_file].tobytes())
            del verts
            counts = sorted({c for c in (300, 1000, 2000, 3000, 5000, 7000, 10000, 30000, 100000, 1000000) if c < nt} | {min(nt, a.prefix_max)})
            txt = subprocess.check_output([exe, path, repr(MIN_DIST), str(a.host_max)] + [str(c) for c in counts], text=True, timeout=1500)
            os.remove(path)
            e["program_path_by_prefix"] = [json.loads(ln) for ln in txt.splitlines() if ln.strip()]
            both = [p for p in e["program_path_by_prefix"] if p["host_pass_wall_ms"] >= 0]
            losing = [p["vertices"] for p in both if p["gpu_backed_pass_wall_ms"] > p["host_pass_wall_ms"]]
            e["gpu_backed_pass_loses_up_to_vertices"] = max(losing) if losing else 0
            e["rounds_full_mesh"] = e["program_path_by_prefix"][-1]["rounds"]
            out[f"{res}^3"] = e
            print(json.dumps({f"{res}^3": e}), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:  # (after every size: a larger one may not fit the time at hand)
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
