#!/usr/bin/env python3
"""The programs' --decimate on the host (cpu_tsdf::mesh_post::decimateMesh, one thread) against the GPU pass
(tsdf_hip_mesh_decimate, csrc/tsdf_decimate.hip), on the SAME fetched mesh in the same run: Scene A fused at 512^3.

The marching-cubes mesh is fetched once; tools/time_decimate.cpp (compiled here against the drop-in) times both passes, wall
clock, on prefixes of it and on the full mesh (the mesh is in Morton order: a prefix is a compact piece of surface), with a
cell of --cell-voxels voxels -- this is what the program pays: upload, device pass, download and the host's tail included --
and where the crossover of mesh_post::kDecimateHostBelowVertices shows.  Then, per --resident-sizes entry,
tsdf_hip_march_decimate on the device-resident mesh for cells of 2, 4 and 8 voxels, by HIP events
(tsdf_hip_mesh_decimate_stats), median of RUNS repetitions after WARMUP.  The host pass is the yardstick: timed on the same
host in the same run.

usage: time_decimate.py [--sizes 512] [--resident-sizes 2048] [--frames 20] [--runs 5] [--warmup 2] [--cell-voxels 2]
                        [--host-max 3000000] [--prefix-max 3000000] [--out profiles/decimate_timing.json]"""
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

RESIDENT_CELLS = (2, 4, 8)  # voxels


def build_timer(tmp):
    exe = os.path.join(tmp, "time_decimate")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tools", "time_decimate.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                           "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def voxel_of(vol, res):
    return float(vol._p.size[0]) / res


def device_resident(vol, res, runs, warmup):
    """tsdf_hip_march + tsdf_hip_march_decimate: the soup never leaves the GPU."""
    lib, h = capi.load(), vol._need()
    out = []
    for cells in RESIDENT_CELLS:
        dev, st = [], None
        for r in range(warmup + runs):
            n, m, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            capi.check(lib.tsdf_hip_march(h, 2.0, 0, C.byref(n)), "march")
            capi.check(lib.tsdf_hip_march_decimate(h, cells * voxel_of(vol, res), C.byref(m), C.byref(k)), "march_decimate")
            st = (C.c_uint64 * 4)()
            capi.check(lib.tsdf_hip_mesh_decimate_stats(st), "mesh_decimate_stats")
            if r >= warmup:
                dev.append(st[3] / 1000.0)
        ms, n_cells = (C.c_float * 3)(), C.c_uint64(0)
        capi.check(lib.tsdf_hip_march_timing(h, ms, C.byref(n_cells)), "march_timing")
        out.append({"cell_voxels": cells, "vertices": int(st[0]), "vertices_out": int(st[1]), "faces": int(n.value), "faces_out": int(k.value),
                    "duplicate_faces": int(st[2]), "decimate_device_ms": median(dev), "march_device_ms": float(sum(ms)), "runs": runs,
                    "warmup": warmup})
        print(json.dumps({f"{res}^3 resident": out[-1]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512", help="grids whose fetched mesh goes through the program path, by prefix")
    ap.add_argument("--resident-sizes", default="2048", help="grids on which only the device-resident pass is timed")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cell-voxels", type=float, default=2.0, help="cell size of the program path, in voxels")
    ap.add_argument("--host-max", type=int, default=3000000, help="largest prefix (faces) the one-thread host pass is timed on")
    ap.add_argument("--prefix-max", type=int, default=3000000, help="largest prefix (faces) handed to the program path at all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decimate_timing.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: the median of at least five runs")
    import torch  # noqa: F401  (before the library: capi._torch_first)
    lib = capi.load()
    if lib.tsdf_hip_device_count() <= 0:
        sys.exit("time_decimate.py: no HIP device -- timings come from the GPU or not at all")
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        head = os.environ.get("TSDF_GIT_HEAD", "unknown")
    out = {"tool": "tools/time_decimate.py", "commit": head, "frames_fused": a.frames, "program_path_cell_voxels": a.cell_voxels}

    def write():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # (after every size: a larger one may not fit the time at hand)
            json.dump(out, f, indent=1)
            f.write("\n")

    with tempfile.TemporaryDirectory() as tmp:
        exe = build_timer(tmp)
        for res in [int(s) for s in a.sizes.split(",") if s]:
            vol = fused_volume(res, a.frames)
            h = vol._need()
            cell = a.cell_voxels * voxel_of(vol, res)
            n = C.c_uint64(0)
            capi.check(lib.tsdf_hip_march(h, 2.0, 0, C.byref(n)), "march")
            nt = int(n.value)
            verts = np.empty((nt, 9), np.float32)
            capi.check(lib.tsdf_hip_march_fetch(h, capi.as_f32p(verts), None, None), "march_fetch")
            e = {"cell_size": cell, "device_resident": device_resident(vol, res, a.runs, a.warmup)}
            vol.close()
            path = os.path.join(tmp, f"mesh{res}.bin")
            n_file = min(nt, a.prefix_max)  # (the timing program builds a PolygonMesh per pass: host memory, not the GPU, bounds it)
            with open(path, "wb") as f:
                f.write(np.int64(n_file).tobytes())
                f.write(verts[:n_file].tobytes())
            del verts
            counts = sorted({c for c in (300, 1000, 2000, 3000, 5000, 7000, 10000, 30000, 100000, 1000000) if c < nt} | {min(nt, a.prefix_max)})
            txt = subprocess.check_output([exe, path, repr(cell), str(a.host_max)] + [str(c) for c in counts], text=True, timeout=1500)
            os.remove(path)
            e["program_path_by_prefix"] = [json.loads(ln) for ln in txt.splitlines() if ln.strip()]
            both = [p for p in e["program_path_by_prefix"] if p["host_pass_wall_ms"] >= 0]
            losing = [p["vertices"] for p in both if p["gpu_backed_pass_wall_ms"] > p["host_pass_wall_ms"]]
            e["gpu_backed_pass_loses_up_to_vertices"] = max(losing) if losing else 0
            out[f"{res}^3"] = e
            print(json.dumps({f"{res}^3": e}), flush=True)
            write()
        for res in [int(s) for s in a.resident_sizes.split(",") if s]:
            vol = fused_volume(res, a.frames)
            out[f"{res}^3"] = {"device_resident": device_resident(vol, res, a.runs, a.warmup)}
            vol.close()
            write()


if __name__ == "__main__":
    main()
