#!/usr/bin/env python3
"""The programs' --normals on the host (cpu_tsdf::mesh_post::meshNormals, one thread) against the GPU pass
(tsdf_hip_mesh_normals, csrc/tsdf_normals.hip), on the SAME mesh in the same run: Scene A fused at 512^3, marched and
flattened on the GPU.

The indexed mesh is fetched once; tools/time_normals.cpp (compiled here against the drop-in) times both passes, wall clock,
best of three each, on prefixes of it and on the full mesh (flatten keeps the marching order: a prefix is a compact piece of
surface) -- this is what the program pays: upload, device pass and download included -- and where the crossover of
mesh_post::kNormalsHostBelowVertices shows.  Then tsdf_hip_march_normals on the device-resident meshes -- the indexed one and
the soup -- by HIP events (tsdf_hip_mesh_normals_stats), median of RUNS repetitions after WARMUP.  The host pass is the
yardstick: timed on the same host in the same run.

usage: time_normals.py [--sizes 512] [--frames 20] [--runs 5] [--warmup 2] [--out profiles/normals_timing.json]"""
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

PREFIXES = (300, 1000, 3000, 10000, 30000, 100000, 300000, 1000000)


def build_timer(tmp):
    exe = os.path.join(tmp, "time_normals")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tools", "time_normals.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                           "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def marched(lib, h, flatten):
    n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    capi.check(lib.tsdf_hip_march(h, 2.0, 0, C.byref(n)), "march")
    if flatten:
        capi.check(lib.tsdf_hip_march_flatten(h, 1e-4, C.byref(m), C.byref(k)), "march_flatten")
    return int(n.value), int(m.value), int(k.value)


def device_resident(lib, h, flatten, runs, warmup):
    """tsdf_hip_march (+ _march_flatten) + _march_normals: the mesh never leaves the GPU."""
    dev, st, faces = [], None, 0
    for r in range(warmup + runs):
        nt, m, k = marched(lib, h, flatten)
        faces = k if flatten else nt
        capi.check(lib.tsdf_hip_march_normals(h, None, None), "march_normals")
        st = (C.c_uint64 * 4)()
        capi.check(lib.tsdf_hip_mesh_normals_stats(st), "mesh_normals_stats")
        if r >= warmup:
            dev.append(st[3] / 1000.0)
    return {"vertices": int(st[0]), "faces": faces, "skipped_faces": int(st[1]), "zero_normals": int(st[2]), "normals_device_ms": median(dev),
            "runs": runs, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # noqa: F401  (before the library: capi._torch_first)
    lib = capi.load()
    if lib.tsdf_hip_device_count() <= 0:
        sys.exit("time_normals.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_normals.py", "commit": head, "frames_fused": a.frames}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_timer(tmp)
        for res in [int(s) for s in a.sizes.split(",") if s]:
            vol = fused_volume(res, a.frames)
            h = vol._need()
            e = {"device_resident_soup": device_resident(lib, h, False, a.runs, a.warmup),
                 "device_resident_indexed": device_resident(lib, h, True, a.runs, a.warmup)}
            print(json.dumps({f"{res}^3 resident": e}), flush=True)
            _, m, k = marched(lib, h, True)
            verts, faces = np.empty((m, 3), np.float32), np.empty((k, 3), np.uint32)
            capi.check(lib.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(verts), None, faces.ctypes.data_as(C.POINTER(C.c_uint32)), None), "fetch_indexed")
            vol.close()
            path = os.path.join(tmp, f"mesh{res}.bin")
            with open(path, "wb") as f:
                f.write(np.asarray([m, k], np.int64).tobytes())
                f.write(verts.tobytes())
                f.write(faces.tobytes())
            counts = sorted({c for c in PREFIXES if c < m} | {m})
            txt = subprocess.check_output([exe, path] + [str(c) for c in counts], text=True, timeout=1500)
            os.remove(path)
            e["program_path_by_prefix"] = [json.loads(ln) for ln in txt.splitlines() if ln.strip()]
            losing = [p["vertices"] for p in e["program_path_by_prefix"] if p["gpu_backed_pass_wall_ms"] > p["host_pass_wall_ms"]]
            e["gpu_backed_pass_loses_up_to_vertices"] = max(losing) if losing else 0
            out[f"{res}^3"] = e
            print(json.dumps({f"{res}^3": e}), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
