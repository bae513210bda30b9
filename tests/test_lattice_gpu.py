"""GPU tier: every reader of the volume, the storage paths and integrateCloud on the degenerate voxel values of
tests/lattice_cases.py -- exact zeros of either sign, denormals, +-1 and its neighbours below, NaN, +-Inf, weights at and
around the thresholds -- against the plain model of tests/sequence_model.py (the oracle, which tests/test_oracle_lattice.py
pins to the compiled reference on the same values).

Every case is one configuration (PACKED with and without colour, F32W with colour), one grid (32^3, or 50 x 37 x 41 with
pitch != nx and odd row and plane counts), one handle or a three-slab set on one device, and one family.  Each test uploads
the family into the product and into a Model, asserts from the MODEL's answer that the comparison is not an empty one
(tests/lattice_cases.FLOORS), and only then calls the product."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch  # at collection time, i.e. before libtsdf_hip.so brings in the system's HIP runtime (see tests/conftest.py)

from cpu_tsdf_amd import capi, synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, transform_cloud_with_normals
from oracle import oracle as O
from tests import align_cases, flatten_cases, shift_cases
from tests import lattice_cases as L
from tests.common import assert_same_f32, make_volume
from tests.sequence_model import Model, assert_same_mesh, compare, slab_starts
from tests.test_occupied_gpu import check as check_occupied

pytestmark = pytest.mark.gpu

SIZE, W, H = 0.125, 80, 60
CONFIGS = {"packed_colour": (capi.LAYOUT_AUTO, True), "packed_plain": (capi.LAYOUT_AUTO, False), "f32w_colour": (capi.LAYOUT_F32W, True)}
GRIDS = {"32": (32, 32, 32), "50x37x41": (50, 37, 41)}
HANDLES = {"one_handle": None, "set_0_0_0": [0, 0, 0]}
CASES = list(itertools.product(CONFIGS, GRIDS, HANDLES, L.FAMILIES))
IDS = ["-".join(c) for c in CASES]
every_case = pytest.mark.parametrize("config,grid,handle,family", CASES, ids=IDS)
FLOORS = L.FLOORS
_MEMO = {}


def memo(key, fn):
    """An expensive answer of the model (the Python loops of the cleanup and flatten oracles), computed once per process."""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


class Case:
    """One product volume and the model of the same voxels."""

    def __init__(self, config, grid, handle, family, quiet_nans=False, weighting=None):
        layout, self.color = CONFIGS[config]
        self.key = (config, grid, family)
        self.family, self.res3, self.single = family, GRIDS[grid], HANDLES[handle] is None
        self.random = family.startswith("random")
        self.vol, self.sc = make_volume(32, W, H, color=self.color, res3=self.res3, size3=(SIZE,) * 3, trunc=L.TRUNC[family],
                                        max_weight=L.MAX_WEIGHT)
        self.vol.setLayout(layout)
        if weighting:
            self.vol.setWeighting(*weighting)
        if not self.single:
            self.vol.setDevices(HANDLES[handle])
        self.vol.reset()
        self.f32w = layout == capi.LAYOUT_F32W
        assert self.vol.getLayout() == (capi.LAYOUT_F32W if self.f32w else capi.LAYOUT_PACKED)
        self.model = Model(self.vol._p, mode="by_depth" if weighting else None)
        d, w, rgb = L.build(family, self.res3, self.color, self.f32w)
        if quiet_nans:
            d = L.with_quiet_nans(d)
        self.arrays = (d, w, rgb)
        self.model.upload(d, w, rgb)
        self.vol.upload(d, w, rgb)
        self.voxel = SIZE / self.res3[0]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.vol.close()

    def download_equals(self, want, what):
        d, w, rgb = self.vol.download()
        L.assert_same_bits(d, want[0], f"{what}: d")
        L.assert_same_bits(w, want[1], f"{what}: w")
        if self.color:
            assert np.array_equal(rgb, want[2]), f"{what}: rgb"

    def marcher(self, w_min, mode):
        mc = MarchingCubesTSDFOctree()
        mc.setInputTSDF(self.vol)
        mc.setMinWeight(w_min)
        mc.setColorByRGB(mode == 1)
        mc.setColorByConfidence(mode == 2)
        return mc


def want_mesh(model, w_min, mode):
    """The soup reconstruct(want_cells=True) returns in colour mode 0, 1 or 2 (Model.mesh knows the volume's own mode only)."""
    verts, rgb, cells = model.ov.march(w_min, mode)
    n = len(cells)
    return {"vertices": verts, "polygons": np.arange(3 * n, dtype=np.int32).reshape(n, 3), "rgb": rgb if mode else None, "cells": cells}


# ---- 1. storage keeps bits ------------------------------------------------------------------------------------------------
@every_case
def test_storage_keeps_every_bit(gpu, tmp_path, config, grid, handle, family):
    """download, get_planes_device -> set_planes_device (one handle), save -> load, shiftVolume: the sign of zero, the
    denormals and the payload and sign of two planted quiet NaNs come back as they went in."""
    with Case(config, grid, handle, family, quiet_nans=True) as c:
        vol, (d, w, rgb) = c.vol, c.arrays
        nx, ny, nz = c.res3
        bits = d.view(np.uint32)
        for word, (x, y, z) in L.QUIET_NANS:
            assert bits[z, y, x] == word
        assert (bits == 0x80000000).any() or not c.random
        c.download_equals(c.arrays, "after upload")
        if c.single:
            lib, dev = capi.load(), torch.device("cuda", 0)
            dt = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
            wt = torch.empty_like(dt)
            ct = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev) if c.color else None
            args = (C.c_void_p(dt.data_ptr()), C.c_void_p(wt.data_ptr()), C.c_void_p(ct.data_ptr()) if c.color else None)
            torch.cuda.synchronize()
            capi.check(lib.tsdf_hip_get_planes_device(vol._need(), 0, nz, *args), "get_planes_device")
            vol.synchronize()
            L.assert_same_bits(dt.cpu().numpy(), d, "planes on the device: d")
            L.assert_same_bits(wt.cpu().numpy(), w, "planes on the device: w")
            vol.reset()
            capi.check(lib.tsdf_hip_set_planes_device(vol._need(), 0, nz, *args), "set_planes_device")
            vol.synchronize()
            c.download_equals(c.arrays, "after get_planes_device -> set_planes_device")
        path = str(tmp_path / "lattice.vol")
        if nx == ny == nz and nx & (nx - 1) == 0:
            vol.save(path)
            vol.load(path)
            c.download_equals(c.arrays, "after save -> load")
        else:   # the .vol octree format has no place for such a grid: refused, and the volume is left as it was
            with pytest.raises(capi.TsdfHipError) as e:
                vol.save(path)
            assert e.value.code == capi.E_UNSUPPORTED
            c.download_equals(c.arrays, "after a refused save")
        s = (1, -2, 3)   # (on a set: planes move from slab to slab)
        vol.shiftVolume(*s)
        want = shift_cases.shifted_volume(d, w, rgb, s)
        c.download_equals(want, f"after shift {s}")
        if not c.single:
            starts = slab_starts(nz)
            s2 = (0, 0, -(starts[1] - starts[0] + 1))   # past a whole slab, the other way
            vol.shiftVolume(*s2)
            c.download_equals(shift_cases.shifted_volume(*want, s2), f"after shift {s} and {s2}")


# ---- 2. marching cubes ---------------------------------------------------------------------------------------------------
@every_case
def test_marching_cubes(gpu, config, grid, handle, family):
    with Case(config, grid, handle, family) as c:
        wants = {}
        for w_min, floor in ((0.0, "triangles_w0"), (2.0, "triangles_w2"), (2.5, "triangles_w2.5")):
            for mode in (0, 1, 2) if c.color else (0, 2):
                wants[(w_min, mode)] = want = want_mesh(c.model, w_min, mode)
                assert len(want["cells"]) >= (FLOORS[floor] if c.random else 1), (w_min, len(want["cells"]))
        if c.random:
            assert L.two_equal_vertices(wants[(0.0, 0)]["vertices"]).mean() >= FLOORS["share_two_equal_vertices"]
        if family == "denormal_shell":   # the signs of the denormals decide: normal-range values give another mesh
            twin = Model(c.vol._p)
            twin.upload(L.normal_shell(c.res3), c.arrays[1], c.arrays[2])
            assert not np.array_equal(twin.ov.march(0.0, 0)[2], wants[(0.0, 0)]["cells"])
        for flush_at in (512, 0):
            try:
                capi.set_tuning("mc_flush_at", flush_at)
                for (w_min, mode), want in wants.items():
                    got = c.marcher(w_min, mode).reconstruct(want_cells=True)
                    assert_same_mesh(got, want, f"w_min {w_min} mode {mode} mc_flush_at {flush_at}")
            finally:
                capi.set_tuning("mc_flush_at", 512)


# ---- 3. setCleanup and setFlatten ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post", ["cleanup", "flatten", "cleanup_then_flatten"])
@every_case
def test_cleanup_and_flatten(gpu, config, grid, handle, family, post):
    """Coincident vertices (a vertex exactly on a corner belongs to several edges) and zero-area faces are the input."""
    with Case(config, grid, handle, family) as c:
        w_min = L.POST_W_MIN
        cl = L.cleanup_setting(c.model) if "cleanup" in post else None
        fl = flatten_cases.MD if "flatten" in post else None
        soup = len(c.model.ov.march(w_min, 0)[2])
        assert soup >= (FLOORS["triangles_w2.5"] if c.random else 1)
        want = memo(c.key + (post,), lambda: c.model.mesh(w_min, cl, fl))
        kept = len(want["cells"]) / soup
        if c.random and post == "cleanup":
            assert FLOORS["cleanup_kept"] <= kept <= 1 - FLOORS["cleanup_dropped"], kept
        elif c.random and post == "flatten":
            assert 1 - kept >= FLOORS["flatten_dropped"], kept
        else:
            assert len(want["cells"]) > 0
        mc = c.marcher(w_min, 1 if c.color else 0)
        if cl:
            mc.setCleanup(*cl)
        if fl:
            mc.setFlatten(fl)
        assert_same_mesh(mc.reconstruct(want_cells=True), want, post)


# ---- 4. renderView -----------------------------------------------------------------------------------------------------------
def voxel_colours(ov, pts):
    """Per point the colour of the voxel the oracle's octree descent finds it in, and whether there is one."""
    rgb, found = np.zeros((len(pts), 3), np.uint8), np.zeros(len(pts), bool)
    idx = (C.c_int * 3)()
    for k, (x, y, z) in enumerate(np.asarray(pts, np.float32)):
        if O.lib().oracle_containing(C.byref(ov.p), x, y, z, idx):
            found[k] = True
            rgb[k] = ov.rgb[idx[2], idx[1], idx[0]]
    return rgb, found


@every_case
def test_render_view(gpu, config, grid, handle, family):
    with Case(config, grid, handle, family) as c:
        poses = L.poses(SIZE)
        wants = {(k, ds): c.model.raycast(tr, ds) for k, tr in enumerate(poses) for ds in (1, 2, 3)}
        hits = [int(np.isfinite(wants[(k, 1)][..., 0]).sum()) for k in range(len(poses))]
        if c.random:
            assert min(hits) >= FLOORS["hits_per_pose"], hits
            if family == "random_nonfinite":
                assert sum(int(np.isnan(wants[(k, 1)][..., 6]).sum()) for k in range(len(poses))) >= FLOORS["nan_t_rays"]
        else:
            assert hits[L.FRONT] >= 1000, hits
        for (k, ds), want in wants.items():
            got = c.vol.renderView(poses[k], ds, camera_frame=False)
            assert got.shape == (H // ds, W // ds, 8)
            assert_same_f32(got, want, f"renderView pose {k} ds {ds}")
        if c.color:
            tr = poses[L.FRONT]
            cloud, rgb = c.vol.renderColoredView(tr, 1)
            want_cloud = transform_cloud_with_normals(wants[(L.FRONT, 1)], synth.eigen_affine_inverse(tr))
            assert_same_f32(cloud[..., :6], want_cloud[..., :6], "renderColoredView cloud")
            hit = ~np.isnan(cloud[..., 2])
            m, p = tr.astype(np.float32), cloud[..., :3][hit]   # tsdf_volume_octree.cpp:441, as renderColoredView restates it
            q = np.stack([(m[r, 0] * p[:, 0] + (m[r, 1] * p[:, 1] + m[r, 2] * p[:, 2])) + m[r, 3] for r in range(3)], 1)
            want_rgb, found = voxel_colours(c.model.ov, q)
            want_rgb[~found] = 0
            assert found.sum() >= 1000 and len(np.unique(want_rgb[found], axis=0)) > 20
            assert np.array_equal(rgb[hit], want_rgb), "renderColoredView colours at the hits"
            assert not rgb[~hit].any()


# ---- 5. sample -----------------------------------------------------------------------------------------------------------------
@every_case
def test_sample(gpu, config, grid, handle, family):
    with Case(config, grid, handle, family) as c:
        pts = L.sample_points(c.model.ov)
        ok, val, grad, hess = c.model.sample(pts)
        assert len(pts) == 4000 and FLOORS["sample_ok"][0] <= ok.mean() <= FLOORS["sample_ok"][1], ok.mean()
        if family == "random_nonfinite":
            assert np.isnan(val[ok]).sum() >= FLOORS["sample_nan_ok"]
        got = c.vol.sample(pts)
        assert np.array_equal(got[0], ok), "ok mask"
        for g, w_, name in zip(got[1:], (val, grad, hess), ("getFxn", "getGradient", "getHessian")):
            assert_same_f32(g[ok], w_[ok], name)


# ---- 6. getOccupiedVoxelIndices ---------------------------------------------------------------------------------------------------
@every_case
def test_occupied(gpu, config, grid, handle, family):
    with Case(config, grid, handle, family) as c:
        nx, ny, nz = c.res3
        whole = c.model.occupied()
        listed = len(whole[0]) / (nx * ny * nz)
        if c.random:
            assert listed >= FLOORS["occupied_listed"] and 1 - listed >= FLOORS["occupied_left_out"], listed
        else:
            assert 0 < listed < 1
        check_occupied(c.vol, whole, what="whole grid")
        box = (3, 1, 2, nx - 5, ny - 3, nz - 4)
        want = c.model.occupied(box)
        assert 0 < len(want[0]) < len(whole[0])
        check_occupied(c.vol, want, box=box, what=f"box {box}")


# ---- 7. alignmentSystem -----------------------------------------------------------------------------------------------------------
@every_case
def test_alignment_system(gpu, config, grid, handle, family):
    with Case(config, grid, handle, family) as c:
        pts = L.align_points(family, SIZE)
        T = align_cases.se3_exp(np.array([0.01, -0.02, 0.015, 0.3 * c.voxel, -0.2 * c.voxel, 0.4 * c.voxel]))
        for min_weight in (0.0, 2.0):
            want = c.model.alignment(c.vol, pts, T, min_weight, 0.9)
            n_used = int(want["used"].sum())
            assert len(pts) == 1500 and 10 <= n_used < int(want["ok"].sum()), (min_weight, n_used, int(want["ok"].sum()))
            out, used = c.vol.alignmentSystem(pts, T, min_weight, 0.9, want_used=True)
            assert np.array_equal(used, want["used"]), f"used, min_weight {min_weight}"
            align_cases.assert_system(out, want, f"min_weight {min_weight}")


# ---- 8. integrate on top ------------------------------------------------------------------------------------------------------------
def integrate_two_frames(c):
    for i in range(2):
        tr = synth.turntable_pose(i, 8, c.sc.size)
        dep, col = c.sc.depth(tr), (c.sc.bgra(i) if c.color else None)
        want = c.model.integrate(dep, col, tr)
        assert want > 1000
        assert c.vol.integrateCloud(dep, col, tr, count=True) == want, f"observed voxels of frame {i}"
        compare(c.vol, c.model.ov, f"after frame {i}")
    assert (c.model.ov.w == L.MAX_WEIGHT).any() and (c.arrays[1] == 99).any()   # 99 and 100 met the saturation


@every_case
def test_integrate_on_top(gpu, config, grid, handle, family):
    with Case(config, grid, handle, family) as c:
        integrate_two_frames(c)


@pytest.mark.parametrize("family", L.FAMILIES)
def test_integrate_on_top_weighted_by_depth(gpu, family):
    with Case("f32w_colour", "32", "one_handle", family, weighting=(True, False)) as c:
        integrate_two_frames(c)
