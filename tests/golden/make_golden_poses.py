#!/usr/bin/env python3
"""Generate tests/golden/reference_poses_32.npz and reference_poses_32_d.npz from the REFERENCE's own code (oracle/_ref):
integrateCloud and renderView under the rolled / top-down / axis-aligned pose family of tests/pose_cases.py, which no other
fixture touches (their pose builders keep `down = (0, 1, 0)`).

Scene: Scene A, 32^3 grid of 2^-8 m voxels, 160x120 frames, colour on, sensor range 4 S, dense-mode octree; the ten
poses of the family in order, one frame each (tests.pose_cases.frame: noisy depth with NaN pixels).  Stored after EVERY
frame: d, w and rgb; and the reference's renderView of the final volume from roll90, axis_y and diag at radius 1.6 S.
Two files, because together they come to 1.5 MB and no new file of this repository may exceed 1 MiB:
reference_poses_32.npz holds the poses, w, rgb and the views, reference_poses_32_d.npz the ten distance grids."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cpu_tsdf_amd import synth  # noqa: E402
from oracle.refbind import RefVolume, available  # noqa: E402
from tests import pose_cases  # noqa: E402

RES, W, H = 32, 160, 120
MAX_FILE = 1 << 20
VIEWS = ("roll90", "axis_y", "diag")
VIEW_RADIUS = 1.6


def main():
    assert available(), "build oracle/_ref first (make -C oracle ref)"
    sc = synth.scene_a(RES, W, H)
    rv = RefVolume(RES, sc.size, W, H, sc.fx, sc.fy, sc.cx, sc.cy, 0.0, pose_cases.RANGE_FACTOR * sc.size, color=True, dense=True)
    fam = pose_cases.poses(sc.size)
    out = {"res": RES, "width": W, "height": H, "size": np.float32(sc.size), "names": np.array(list(fam)),
           "poses": np.stack(list(fam.values()))}
    dist = {}
    for i, tr in enumerate(fam.values()):
        dep, col = pose_cases.frame(sc, i, tr)
        rv.integrate(dep, col, tr)
        d, w, rgb, leaf, _ = rv.dump_dense()
        assert (leaf == np.float32(sc.size / RES)).all()
        dist[f"d{i}"], out[f"w{i}"], out[f"rgb{i}"] = d, w.astype(np.uint8), rgb
        assert np.array_equal(w, w.astype(np.uint8).astype(np.float32))
    views = pose_cases.poses(sc.size, VIEW_RADIUS)
    out["view_names"] = np.array(VIEWS)
    out["view_poses"] = np.stack([views[n] for n in VIEWS])
    for k, n in enumerate(VIEWS):
        out[f"view{k}"] = rv.render_view(views[n], 1)[0][..., :6]
    for name, arrays in (("reference_poses_32.npz", out), ("reference_poses_32_d.npz", dist)):
        path = os.path.join(ROOT, "tests", "golden", name)
        np.savez_compressed(path, **arrays)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) <= MAX_FILE, path


if __name__ == "__main__":
    main()
