#!/usr/bin/env python3
"""Product-vs-oracle hunt for the second integrate family: setColorMode("RGBNormalized") (k_integrate_rgbn),
setColorMode("LAB") (k_lab_image + k_integrate_lab) and the two weightings (k_integrate_plain modes 2 and 4: by depth,
by variance, both; with and without colour).  The model is fuzz_product_vs_oracle.py; the oracle is the CULLED one
(OracleVolume's planes=, pinned to the compiled reference by tests/test_oracle_culled_modes.py), because the product
applies the reference's frustum cull on every frame.  Each case draws grids whose x count is not a multiple of 4 and
non-cubic grids, 0.125 - 12 m volumes (past 10 m weight_by_depth gives w_new = 0 and fresh voxels 0/0), off-centre
principal points on narrow cameras in about half the cases (the cull bites), zmin > 0, asymmetric truncation, small and
large weight limits, both transformPoint orders, one handle / a Z-slab handle with a halo / 2-3 slab handles on GPU 0, and
one entry point (host sync, pipelined with pairing off or on, device frames, integrate_device2).  Frames carry NaN, inf
and 0 depths, random colours with black pixels, and revisit poses so the variance weighting acts.

After the sequence, bit for bit: d, w, rgb of every voxel; the per-frame observation counts (entry points that count);
downloadColorState / downloadVarianceState (single handles); renderView and renderColoredView; getFxn / gradient /
Hessian; marching cubes with colour at several w_min (for LAB also the bytes against the oracle's lab2rgb of the downloaded
L, A, B).  Needs a GPU.  One line per case, exit status 1 on any difference.
usage: python tests/evidence/fuzz_product_colour_modes.py [--cases 100] [--seed 1]"""
import argparse
import ctypes as C
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cpu_tsdf_amd import capi, synth  # noqa: E402
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, TSDFVolumeOctree  # noqa: E402
from oracle import oracle  # noqa: E402
from oracle.oracle import OracleVolume  # noqa: E402
from tests.evidence.fuzz_oracle_vs_reference import same  # noqa: E402

MODES = ["RGBNormalized", "LAB", "by_depth", "by_variance", "by_depth+by_variance"]
ENTRIES = ["sync", "pipelined", "paired", "device", "device2"]


def draw(rng):
    """One random case (a dict run_case takes)."""
    mode = MODES[rng.randint(len(MODES))]
    color = mode in ("RGBNormalized", "LAB") or bool(rng.randint(2))
    nx = int(rng.choice([16, 33, 45, 64, 70, 96, 130]))
    res3 = (nx, nx, nx)
    if rng.rand() < 0.4:   # non-cubic: other counts along y and z, cubic voxels
        res3 = (nx, int(rng.choice([nx // 2 + 1, nx, nx + 7])), int(rng.choice([nx // 2 + 3, nx + 10])))
    size = float(rng.choice([0.125, 0.3, 1.0, 3.0, 12.0]))
    W, H = [(48, 36), (64, 48), (80, 60), (160, 120)][rng.randint(4)]
    off = bool(rng.rand() < 0.5)
    if off:   # narrow camera, principal point 15-40 % off centre: the reference's cull drops voxels that project into the image
        f = float(rng.uniform(1.0, 1.6)) * W
        cx = W / 2 - 0.5 + rng.choice([-1, 1]) * float(rng.uniform(0.15, 0.4)) * W / 2
        cy = H / 2 - 0.5 + rng.choice([-1, 1]) * float(rng.uniform(0.0, 0.4)) * H / 2
    else:
        f = float(rng.uniform(0.5, 1.6)) * W
        cx, cy = W / 2 - 0.5 + float(rng.uniform(-0.1, 0.1)) * W / 2, H / 2 - 0.5 + float(rng.uniform(-0.1, 0.1)) * H / 2
    handle = ["one", "zslab", "multi"][rng.randint(3)]
    zb = int(rng.randint(0, res3[2] // 2))
    ze = int(rng.randint(zb + 1, res3[2] + 1))
    return dict(
        mode=mode, color=color, res3=res3, size3=tuple(size * r / nx for r in res3), W=W, H=H,
        fx=f, fy=f * float(rng.uniform(0.95, 1.05)), cx=cx, cy=cy,
        zmin=float(rng.choice([0.0, 0.05, 0.3])) * size, zmax=float(rng.uniform(1.5, 4.0)) * size * max(res3) / nx,
        pos=float(rng.uniform(0.03, 0.25)) * size, neg=float(rng.uniform(0.03, 0.25)) * size,
        wmax=float(rng.choice([0.5, 1.0, 2.0, 3.5, 100.0, 255.0])), order=int(rng.randint(2)),
        handle=handle, n_dev=int(rng.choice([2, 3])), zslab=(zb, ze, int(rng.randint(0, 3))),
        entry=ENTRIES[rng.randint(len(ENTRIES))], n_poses=int(rng.randint(1, 4)),
        n_frames=int(rng.randint(7, 12)) if "by_variance" in mode else int(rng.randint(2, 6)),
        seed=int(rng.randint(1 << 30)), off_centre=off)


def make_product(c):
    v = TSDFVolumeOctree()
    v.setResolution(*c["res3"])
    v.setGridSize(*c["size3"])
    v.setImageSize(c["W"], c["H"])
    v.setCameraIntrinsics(c["fx"], c["fy"], c["cx"], c["cy"])
    v.setSensorDistanceBounds(c["zmin"], c["zmax"])
    v.setDepthTruncationLimits(c["pos"], c["neg"])
    v.setWeightTruncationLimit(c["wmax"])
    v.setIntegrateColor(c["color"])
    v.setTransformOrder(c["order"])
    if c["mode"] in ("RGBNormalized", "LAB"):
        v.setColorMode(c["mode"])
    else:
        v.setWeighting("by_depth" in c["mode"], "by_variance" in c["mode"])
    if c["handle"] == "zslab":
        v.setZSlab(*c["zslab"])
    elif c["handle"] == "multi":
        v.setDevices([0] * c["n_dev"])
    v.reset()
    if c["entry"] == "paired":
        v.setFramePairing(True)
    return v


def oracle_step(ov, c, dep, col, T, planes, zr):
    """One frame through the oracle form of the case's mode (planes None = no cull)."""
    col = col if c["color"] else None
    mode = c["mode"]
    if mode == "RGBNormalized":
        return ov.integrate_rgbn(dep, col, T, *zr, planes=planes)
    if mode == "LAB":
        return ov.integrate_lab(dep, col, T, *zr, planes=planes)
    if "by_variance" in mode:
        return ov.integrate_variance(dep, col, T, "by_depth" in mode, *zr, planes=planes)
    return ov.integrate(dep, col, T, *zr, weight_by_depth=True, planes=planes)


def frames(c):
    rng = np.random.RandomState(c["seed"])
    size = min(c["size3"])   # (the scene's sphere sits in the grid's smallest extent)
    W, H = c["W"], c["H"]
    sc = synth.Scene(size, W, H, sphere=float(rng.uniform(0.15, 0.35)), box=float(rng.uniform(0.35, 0.49)))
    sc.fx, sc.fy, sc.cx, sc.cy = c["fx"], c["fy"], c["cx"], c["cy"]
    sc.h = np.array([0.47 * s3 for s3 in c["size3"]]) * float(rng.uniform(0.8, 1.0))
    poses = []
    for _ in range(c["n_poses"]):
        eye = rng.normal(size=3)
        eye *= float(rng.uniform(*c.get("eye", (0.9, 2.2)))) * size / np.linalg.norm(eye)
        poses.append(synth.look_at_pose(eye, target=rng.uniform(-0.15, 0.15, 3) * size))
    out = []
    for i in range(c["n_frames"]):
        tr = poses[i % len(poses)]
        dep = sc.depth(tr, noise_seed=int(rng.randint(1 << 30)), noise_sigma=float(rng.choice([0.002, 0.01, 0.03])) * size)
        junk = rng.rand(H, W)
        dep[junk < 0.03] = np.nan
        dep[(junk >= 0.03) & (junk < 0.04)] = 0.0
        dep[(junk >= 0.04) & (junk < 0.05)] = np.inf
        col = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
        col[rng.rand(H, W) < 0.04, :3] = 0
        out.append((tr, dep, col))
    return out, rng


def oracle_colours(ov, cloud, trans):
    """renderColoredView's colours from the oracle: each hit moved back by trans in float (as the front end does) and the
    colour of the oracle voxel containing it (oracle_containing); misses 0, 0, 0."""
    rgb = np.zeros(cloud.shape[:2] + (3,), np.uint8)
    hit = ~np.isnan(cloud[..., 2])
    m = np.asarray(trans, np.float64).astype(np.float32)
    p = cloud[..., :3][hit]
    q = np.empty_like(p)
    for r in range(3):
        q[:, r] = (m[r, 0] * p[:, 0] + (m[r, 1] * p[:, 1] + m[r, 2] * p[:, 2])) + m[r, 3]
    idx = (C.c_int * 3)()
    out = np.zeros((len(q), 3), np.uint8)
    L = oracle.lib()
    for i, (x, y, z) in enumerate(q):
        if L.oracle_containing(C.byref(ov.p), float(x), float(y), float(z), idx):
            out[i] = ov.rgb[idx[2], idx[1], idx[0]]
    rgb[hit] = out
    return rgb


def run_case(c, check_cull=False):
    """Run one case; returns (list of what differs, info dict)."""
    import torch
    v = make_product(c)
    ov = OracleVolume(v._p)
    ov_plain = OracleVolume(v._p) if check_cull else None
    zr = (c["zslab"][0], c["zslab"][1]) if c["handle"] == "zslab" else (0, 0)
    seq, rng = frames(c)
    what, kept = [], []
    counts_gpu, counts_cpu = [], []
    entry = c["entry"]
    i = 0
    while i < len(seq):
        tr, dep, col = seq[i]
        colv = col if c["color"] else None
        T = synth.cam_from_vol_f32(tr)
        if entry == "device2" and i + 1 < len(seq):
            tr2, dep2, col2 = seq[i + 1]
            fa, fb = device_frame(dep, colv), device_frame(dep2, col2 if c["color"] else None)
            kept += [fa, fb]
            _, n = v.integrateCloudDevice2((fa[0].data_ptr(), fa[1].data_ptr() if c["color"] else 0, tr),
                                           (fb[0].data_ptr(), fb[1].data_ptr() if c["color"] else 0, tr2), count=True)
            counts_gpu += n
            for t, dp, cl in ((tr, dep, col), (tr2, dep2, col2)):
                counts_cpu.append(oracle_step(ov, c, dp, cl, synth.cam_from_vol_f32(t), ov.reference_cull_planes(t), zr))
                if ov_plain is not None:
                    oracle_step(ov_plain, c, dp, cl, synth.cam_from_vol_f32(t), None, zr)
            i += 2
            continue
        if entry in ("device", "device2"):
            f = device_frame(dep, colv)
            kept.append(f)
            counts_gpu.append(v.integrateCloudDevice(f[0].data_ptr(), f[1].data_ptr() if c["color"] else 0, tr, count=True))
        elif entry in ("pipelined", "paired"):
            v.integrateCloud(dep, colv, tr, pipelined=True)
        else:
            counts_gpu.append(v.integrateCloud(dep, colv, tr, count=True))
        n = oracle_step(ov, c, dep, col, T, ov.reference_cull_planes(tr), zr)
        if entry not in ("pipelined", "paired"):
            counts_cpu.append(n)
        if ov_plain is not None:
            oracle_step(ov_plain, c, dep, col, T, None, zr)
        i += 1
    v.synchronize()
    torch.cuda.synchronize()
    del kept
    if counts_gpu != counts_cpu:
        what.append("n_observed")
    zb, ze = zr if c["handle"] == "zslab" else (0, c["res3"][2])
    d, w, rgb = v.download()
    if not (same(d, ov.d[zb:ze]) and same(w, ov.w[zb:ze])):
        what.append("voxels")
    if c["color"] and not np.array_equal(rgb, ov.rgb[zb:ze]):
        what.append("rgb")
    if c["handle"] != "multi":
        if c["mode"] in ("RGBNormalized", "LAB"):
            cs = v.downloadColorState()
            if not all(same(cs[k], ov.cn[k][zb:ze]) for k in range(len(cs))):
                what.append("colour state")
        if "by_variance" in c["mode"]:
            nx, ny, _ = c["res3"]
            M, ns = np.empty((ze - zb, ny, nx), np.float32), np.empty((ze - zb, ny, nx), np.int32)
            capi.check(capi.load().tsdf_hip_download_variance_state(v._need(), 0, 0, zb, nx, ny, ze - zb, capi.as_f32p(M),
                                                                    ns.ctypes.data_as(C.POINTER(C.c_int32))), "download_variance_state")
            if not (same(M, ov.M[zb:ze]) and np.array_equal(ns, ov.nsample[zb:ze])):
                what.append("variance state")
    if c["mode"] == "LAB" and c["handle"] != "multi":   # the bytes every reader shows are LAB2RGB of the stored means
        touched = ov.w[zb:ze] != 0
        if not np.array_equal(oracle.lab2rgb(np.moveaxis(v.downloadColorState(), 0, -1)[touched]), rgb[touched]):
            what.append("lab2rgb")
    size = min(c["size3"])
    if c["handle"] != "zslab":   # the queries need the whole grid
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k in range(2):
                r = float(rng.uniform(0.3, 2.0)) * size
                eye = rng.normal(size=3)
                eye *= r / np.linalg.norm(eye)
                tr = synth.look_at_pose(eye, target=rng.uniform(-0.2, 0.2, 3) * size)
                try:
                    if not same(v.renderView(tr, 1 + k, camera_frame=False), ov.raycast(tr, 1 + k)):
                        what.append(f"renderView{k}")
                    if c["color"]:
                        cloud, crgb = v.renderColoredView(tr, 1 + k)
                        if not np.array_equal(crgb, oracle_colours(ov, cloud, tr)):
                            what.append(f"renderColoredView{k}")
                except capi.TsdfHipError as e:
                    what.append(f"render{k} raised: {e}")
            for wmin in (0.0, 0.5, 1.0, float(rng.choice([1.5, 2.5]))):
                mc = MarchingCubesTSDFOctree()
                mc.setInputTSDF(v)
                mc.setMinWeight(wmin)
                mc.setColorByRGB(c["color"])
                mesh = mc.reconstruct()
                v_m, c_m, _ = ov.march(wmin, 1 if c["color"] else 0)
                if not same(mesh["vertices"], v_m) or (c["color"] and not np.array_equal(mesh["rgb"], c_m)):
                    what.append(f"mesh(w>={wmin})")
            pts = (rng.uniform(-0.55, 0.55, (400, 3)) * np.array(c["size3"])).astype(np.float32)
            ok, val, grad, hess = v.sample(pts)
            ook, oval, ograd, ohess = ov.sample(pts)
            if not (np.array_equal(ok, ook) and same(val[ok], oval[ok]) and same(grad[ok], ograd[ok]) and same(hess[ok], ohess[ok])):
                what.append("getFxn")
    v.close()
    info = dict(observed=int((ov.w[zb:ze] != 0).sum()), nan=int(np.isnan(ov.d).sum()), frac=float(((ov.w % 1) != 0).mean()),
                observed_x256=int((ov.w[zb:ze, :, 256:] != 0).sum()))   # (voxels of a row's second 256-thread block)
    if ov_plain is not None:
        info["cull_removed"] = not (np.array_equal(ov.w.view(np.uint32), ov_plain.w.view(np.uint32))
                                    and np.array_equal(ov.d.view(np.uint32), ov_plain.d.view(np.uint32)))
    return what, info


def device_frame(dep, col):
    """[depth | bgra] in one device allocation, as tsdf_hip_integrate_device2 wants it."""
    import torch
    H, W = dep.shape
    t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    t[0].copy_(torch.from_numpy(dep))
    if col is not None:
        t[1].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
    return t


def describe(c):
    hd = {"one": "one", "zslab": "zslab[%d,%d)+%d" % c["zslab"], "multi": f"multi{c['n_dev']}"}[c["handle"]]
    return (f"{c['mode']:<20s} colour {int(c['color'])} res {'x'.join(map(str, c['res3'])):>11s} size {min(c['size3']):6.3f} "
            f"{c['W']}x{c['H']} f {c['fx']:6.1f} c ({c['cx'] - (c['W'] / 2 - 0.5):+5.1f},{c['cy'] - (c['H'] / 2 - 0.5):+5.1f}) "
            f"z [{c['zmin']:.2f},{c['zmax']:.1f}] trunc {c['pos']:.3f}/{c['neg']:.3f} wmax {c['wmax']} order {c['order']} {hd:<16s} "
            f"{c['entry']:<9s} frames {c['n_frames']:2d}/{c['n_poses']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    capi.use_test_library()
    rng = np.random.RandomState(a.seed)
    bad, bit = [], 0
    for case in range(a.cases):
        c = draw(rng)
        what, info = run_case(c, check_cull=c["off_centre"])
        bit += bool(info.get("cull_removed"))
        print(f"case {case:4d}: {describe(c)} {'cull-bites' if info.get('cull_removed') else '':10s} observed {info['observed']:8d} "
              f"nan {info['nan']:6d} frac {info['frac']:.2f}  {'DIFF ' + ','.join(what) if what else 'ok'}", flush=True)
        if what:
            bad.append((case, what))
    print(f"{a.cases} cases, seed {a.seed}: {len(bad)} with differences {bad[:20]}; the cull removed voxels in {bit} cases")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
