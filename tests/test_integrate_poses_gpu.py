"""GPU tier: the integrate kernels under the pose family of tests/pose_cases.py -- cameras rolled about the optical axis,
looking along the volume's y axis, and exactly axis-aligned -- against the culled CPU oracle, which
tests/test_oracle_poses.py pins to the reference on the same family.

Every kernel restates pcl::transformPoint by hand, split into a per-thread x part and a per-block row part.  The poses the
rest of the suite uses to confirm WHICH instance ran have exact zeros in cam_from_vol[0][1], [1][0], [1][2] and [2][1], so
a wrong index, summation order or pair half in those terms adds an exact zero there and goes unnoticed.  Here every one of
the ten frames has those entries away from zero or at +-1, all ten go into ONE volume in family order, and
tsdf_hip_last_launch_info confirms the instance after every launch.  Bar: bit equality of d, w, rgb and of the
observed-voxel counts on the frames that count."""
import functools

import numpy as np
import pytest

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests import pose_cases
from tests.common import assert_same_f32, make_volume
from tests.test_integrate_gpu import compare, launch_info

pytestmark = pytest.mark.gpu
W, H = 160, 120
LAYOUTS = (capi.LAYOUT_PACKED, capi.LAYOUT_F32W)


def family_volume(res, color, order=0, wmax=100.0, **kw):
    """Scene A at `res`, 160x120, sensor range 4 S: every pose of the family sees the whole grid inside the ALLIN border."""
    sc = synth.scene_a(res, W, H)
    return make_volume(res, W, H, color=color, order=order, max_weight=wmax, zmax=pose_cases.RANGE_FACTOR * sc.size, **kw)


@functools.lru_cache(maxsize=None)
def family_frames(res):
    """[(name, pose, depth, bgra)] of the ten frames, computed once per grid size."""
    sc = synth.scene_a(res, W, H)
    return tuple((name, tr) + pose_cases.frame(sc, i, tr) for i, (name, tr) in enumerate(pose_cases.poses(sc.size).items()))


@functools.lru_cache(maxsize=None)
def family_oracle(res, color, order, wmax):
    """The culled oracle after the ten frames and its per-frame counts; shared, never modified."""
    vol, _ = family_volume(res, color, order, wmax)
    ov = OracleVolume(vol._p)
    counts = [ov.integrate_culled(dep, col if color else None, tr, synth.cam_from_vol_f32(tr)) for _, tr, dep, col in family_frames(res)]
    for a in (ov.d, ov.w) + ((ov.rgb,) if color else ()):
        a.setflags(write=False)
    return ov, counts


def run_family(vol, res, color, counts, expect, hit=None, tag=()):
    """The ten frames into `vol`, counting on the even ones; `expect(info)` judges tsdf_hip_last_launch_info after every
    launch."""
    got = []
    for i, (name, tr, dep, col) in enumerate(family_frames(res)):
        count = i % 2 == 0
        n = vol.integrateCloud(dep, col if color else None, tr, count=count)
        assert (n == counts[i]) if count else (n is True), (tag, name, n, counts[i])
        info = launch_info(vol)
        assert expect(info), (tag, name, info)
        got.append(n)
        if hit is not None:
            hit.add(tag + (count,))
    return got


def wmax_of(order):
    """One variant per kind passes the weight limit within the ten frames."""
    return 4.0 if order == 1 else 100.0


def restore_knobs():
    capi.set_tuning("fast_projection", -1)
    capi.set_tuning("allin", 1)
    capi.set_tuning("pipe", 1)
    capi.set_tuning("fuse2", 1)
    capi.set_tuning("rows_per_block", 64)
    capi.set_tuning("cull", 1)


# ---- a. every instance, confirmed ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("order", [0, 1])
def test_general_and_all_inside_instances_equal_the_oracle(gpu, order, color):
    """k_integrate's general and ALLIN instances (the latter with the packed-pair projection), both layouts, certified
    and exact projection, counting or not: 12 instances per (transform order, colour), 48 in all."""
    res = 32
    ov, counts = family_oracle(res, color, order, wmax_of(order))
    hit = set()
    try:
        capi.set_tuning("pipe", 0)
        for layout in LAYOUTS:
            for fp in (1, 0):
                for kind in ("general", "allin"):
                    if kind == "allin" and not fp:
                        continue  # the ALLIN instances exist only with the certified projection
                    capi.set_tuning("fast_projection", fp)
                    capi.set_tuning("allin", int(kind == "allin"))
                    vol, _ = family_volume(res, color, order, wmax_of(order))
                    vol.setLayout(layout)
                    vol.reset()
                    want0 = int(kind == "allin")
                    run_family(vol, res, color, counts, lambda info: info[0] == want0 and info[1] == fp and info[2] == 0 and not info[4],
                               hit, (layout, fp, kind))
                    assert vol.getLayout() == layout
                    compare(vol, ov)
                    vol.close()
    finally:
        restore_knobs()
    assert hit == {(layout, fp, kind, count) for layout in LAYOUTS for fp, kind in ((1, "general"), (0, "general"), (1, "allin"))
                   for count in (True, False)}, sorted(hit)


@pytest.mark.parametrize("color", [False, True], ids=["k_integrate_p", "k_integrate"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("res", [32, 64])
def test_pipelined_row_loop_instances_equal_the_oracle(gpu, res, order, color):
    """Knob pipe on: k_integrate_p without colour, k_integrate's own ALLIN instance with it; their row part (s_yt) is filled
    per block: at 32^3, and at 64^3 where a block walks several row steps and free-space / quiet waves occur."""
    ov, counts = family_oracle(res, color, order, wmax_of(order))
    hit = set()
    try:
        capi.set_tuning("fast_projection", 1)
        capi.set_tuning("allin", 1)
        capi.set_tuning("pipe", 1)
        vol, _ = family_volume(res, color, order, wmax_of(order))
        vol.reset()
        run_family(vol, res, color, counts, lambda info: info[0] == 1 and info[1] == 1 and info[2] == 0 and info[4] == (not color), hit, ("kp",))
        compare(vol, ov)
        vol.close()
    finally:
        restore_knobs()
    assert hit == {("kp", True), ("kp", False)}


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("order", [0, 1])
def test_two_frame_sweep_instances_equal_the_oracle(gpu, order, color):
    """k_integrate2 through integrateCloudDevice2: the family in consecutive pairs, so that the two frames of one sweep
    are rolled differently (frame B's transform travels separately from frame A's)."""
    import torch
    res = 32
    ov, counts = family_oracle(res, color, order, wmax_of(order))
    fr = family_frames(res)
    hit = set()
    try:
        capi.set_tuning("fuse2", 2)
        vol, _ = family_volume(res, color, order, wmax_of(order))
        vol.reset()
        keep = []
        for k in range(len(fr) // 2):
            pair = []
            for i in (2 * k, 2 * k + 1):
                _, tr, dep, col = fr[i]
                t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
                t[0].copy_(torch.from_numpy(dep))
                if color:
                    t[1].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
                keep.append(t)
                pair.append((t[0].data_ptr(), t[1].data_ptr() if color else 0, tr))
            count = k % 2 == 0
            fused, n = vol.integrateCloudDevice2(pair[0], pair[1], count=count)
            assert fused and launch_info(vol)[0] == 2, (k, fused, launch_info(vol))
            assert (n == counts[2 * k:2 * k + 2]) if count else (n is None), (k, n, counts[2 * k:2 * k + 2])
            hit.add(("k2", count))
        compare(vol, ov)
        vol.close()
    finally:
        restore_knobs()
    assert hit == {("k2", True), ("k2", False)}


# ---- b. forced vs unforced ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
def test_forced_and_unforced_instances_agree_plane_for_plane(gpu, color):
    """64^3, the same ten frames: ALLIN on / off, the pipelined row loop on / off, 8 and 64 rows per block -- identical
    planes and counts, and all of them the oracle's."""
    res, wmax = 64, 4.0
    ov, counts = family_oracle(res, color, 0, wmax)
    outs = {}
    try:
        for name, allin, pipe, rpb in (("allin", 1, 0, 64), ("general", 0, 0, 64), ("pipe", 1, 1, 64), ("pipe rows 8", 1, 1, 8),
                                       ("allin rows 8", 1, 0, 8)):
            capi.set_tuning("allin", allin)
            capi.set_tuning("pipe", pipe)
            capi.set_tuning("rows_per_block", rpb)
            vol, _ = family_volume(res, color, 0, wmax)
            vol.reset()
            got = run_family(vol, res, color, counts, lambda info: info[0] == allin and info[4] == bool(pipe and not color), tag=(name,))
            compare(vol, ov)
            outs[name] = (vol.download(), got)
            vol.close()
    finally:
        restore_knobs()
    base, base_n = outs["allin"]
    assert base[1].max() == wmax
    for name, (planes, got) in outs.items():
        assert got == base_n, name
        for a, b in zip(planes, base):
            assert (a is None and b is None) or np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


# ---- c. partly visible grids --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("order", [0, 1])
def test_row_intervals_with_a_rolled_camera_inside_the_grid(gpu, order, color):
    """The camera inside the grid (the `rows` kind of test_every_reachable_k_integrate_instance_equals_the_oracle) with the
    family's `down` vectors in turn: k_rows' intervals and the LIVE instance under roll."""
    res = 32
    downs = pose_cases.downs()
    sc = synth.scene_a(res, W, H)
    fr = []
    for i, down in enumerate(downs):
        tr = synth.look_at_pose((0.02 * (i % 4), 0.01, -0.03), target=(0.05, 0.0, 1.0), down=down)
        assert np.isfinite(tr).all()
        fr.append((tr,) + pose_cases.frame(sc, i, tr))
    vol, _ = make_volume(res, W, H, color=color, order=order, max_weight=wmax_of(order))
    ov = OracleVolume(vol._p)
    counts = [ov.integrate_culled(dep, col if color else None, tr, synth.cam_from_vol_f32(tr)) for tr, dep, col in fr]
    assert min(counts) > 100 and max(counts) < res ** 3 // 4   # something, never much: the camera sits inside
    hit = set()
    try:
        capi.set_tuning("pipe", 0)
        for layout in LAYOUTS:
            for fp in (1, 0):
                capi.set_tuning("fast_projection", fp)
                vol, _ = make_volume(res, W, H, color=color, order=order, max_weight=wmax_of(order))
                vol.setLayout(layout)
                vol.reset()
                for i, (tr, dep, col) in enumerate(fr):
                    n = vol.integrateCloud(dep, col if color else None, tr, count=(i % 2 == 0))
                    assert (n == counts[i]) if i % 2 == 0 else (n is True), (layout, fp, i, n, counts[i])
                    info = launch_info(vol)
                    assert info[0] == 0 and info[1] == fp and info[2] in (1, 2) and not info[4], (layout, fp, i, info)
                    hit.add((layout, fp, i % 2 == 0))
                compare(vol, ov)
                vol.close()
    finally:
        restore_knobs()
    assert hit == {(layout, fp, count) for layout in LAYOUTS for fp in (1, 0) for count in (True, False)}, sorted(hit)


# The `cull` kind of test_every_reachable_k_integrate_instance_equals_the_oracle is a turntable camera yawed so that the grid
# sits beside the optical axis, where the reference's pyramid (1.1 x the field of view AROUND THE AXIS) cuts the image of a
# principal point 60 % off centre.  Rolling that camera about its optical axis swings the grid out of the cut: measured on
# the oracle, the cull drops 600 voxels per frame at 0 degrees, 360 at +-20, 195 at +-30, 45 at +-40 and none from +-50 on.
# So "yaw, roll" keeps the rolls at which it still bites; "roll, yaw" turns the camera about the line of sight to the grid
# first and yaws afterwards, which leaves the grid where the cut is at ANY roll (600 voxels per frame dropped at 90 and -135).
CULL_CASES = (("yaw, roll", 30.0), ("yaw, roll", 40.0), ("yaw, roll", -20.0), ("roll, yaw", 90.0), ("roll, yaw", -135.0))


def cull_frames(sc, how, roll):
    psi = float(np.arctan(0.6 * (W / 2) / sc.fx))
    yaw = np.eye(4)
    yaw[0, 0], yaw[0, 2], yaw[2, 0], yaw[2, 2] = np.cos(psi), np.sin(psi), -np.sin(psi), np.cos(psi)
    rot = pose_cases.roll_about_optical_axis(roll)
    out = []
    for i in range(4):
        tr = synth.turntable_pose(2 * i + 1, 8, sc.size) @ (yaw @ rot if how == "yaw, roll" else rot @ yaw)
        out.append((tr,) + pose_cases.frame(sc, i, tr))
    return out


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("how,roll", CULL_CASES)
def test_reference_cull_through_the_row_intervals_with_a_rolled_camera(gpu, how, roll, color):
    """Where the reference's frustum cull bites under roll: checked on the oracle first, in EVERY frame.  A frame in which it
    drops a voxel is one whose six planes cannot keep the whole slab, so the launch must be the LIVE instance with the exact
    half of the row intervals (launch_info[2] == 2), as in the unrolled `cull` kind."""
    res = 32
    try:
        capi.set_tuning("pipe", 0)
        for order in (0, 1):
            for layout in LAYOUTS:
                for fp in (1, 0):
                    capi.set_tuning("fast_projection", fp)
                    vol, sc = make_volume(res, W, H, color=color, order=order, max_weight=wmax_of(order))
                    sc.cx += 0.6 * W / 2
                    vol.setCameraIntrinsics(sc.fx, sc.fy, sc.cx, sc.cy)
                    vol.setLayout(layout)
                    vol.reset()
                    oc, oa = OracleVolume(vol._p), OracleVolume(vol._p)
                    for i, (tr, dep, col) in enumerate(cull_frames(sc, how, roll)):
                        c = col if color else None
                        want = oc.integrate_culled(dep, c, tr, synth.cam_from_vol_f32(tr))
                        assert want < oa.integrate(dep, c, synth.cam_from_vol_f32(tr)), (how, roll, i)   # the cull bites
                        n = vol.integrateCloud(dep, c, tr, count=(i % 2 == 0))
                        assert (n == want) if i % 2 == 0 else (n is True), (order, layout, fp, i, n, want)
                        info = launch_info(vol)
                        assert info[0] == 0 and info[1] == fp and info[2] == 2 and not info[4], (order, layout, fp, i, info)
                    compare(vol, oc)
                    vol.close()
    finally:
        restore_knobs()


@pytest.mark.parametrize("slab", [None, (7, 31)])
def test_brick_cull_random_rolled_poses_equal_no_cull(gpu, slab):
    """test_brick_cull_random_poses_equal_no_cull's idea under roll: random eyes in and around the wide grid of
    test_cull_sub_grid_offsets_on_a_wide_grid with random `down` vectors (none within 20 degrees of the view direction):
    forced cull == no cull, byte for byte, counts included -- and both the culled oracle's."""
    rng = np.random.RandomState(23)
    res3, size3 = (2304, 72, 40), (9.0, 0.3, 0.16)
    sc = synth.Scene(1.0, W, H)
    poses = []
    while len(poses) < 14:
        eye = np.array([rng.uniform(-5.0, 5.0), rng.uniform(-0.3, 0.3), rng.uniform(-0.4, 0.4)])
        tgt = np.array([rng.uniform(-4.5, 4.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05)])
        down = rng.normal(size=3)
        view = (tgt - eye) / np.linalg.norm(tgt - eye)
        if abs(np.dot(down / np.linalg.norm(down), view)) > np.cos(np.radians(20.0)):
            continue
        poses.append(synth.look_at_pose(eye, target=tgt, down=down))
    assert max(abs(synth.cam_from_vol_f32(tr)[1]) for tr in poses) > 0.5   # really rolled
    depths = [np.full((H, W), d, np.float32) for d in rng.uniform(0.2, 1.4, len(poses))]
    res = []
    try:
        for cull in (2, 0):
            capi.set_tuning("cull", cull)
            vol, _ = make_volume(64, W, H, color=True, res3=res3, size3=size3, zmin=0.05, zmax=1.5)
            if slab:
                vol.setZSlab(*slab)
            vol.reset()
            counts = [vol.integrateCloud(dep, sc.bgra(i), tr, count=True) for i, (tr, dep) in enumerate(zip(poses, depths))]
            res.append((vol.download(), counts))
            vol.close()
    finally:
        restore_knobs()
    assert res[0][1] == res[1][1] and sum(res[0][1]) > 10000, res[0][1]
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert 0.0 < (res[0][0][1] > 0).mean() < 0.95
    ov = OracleVolume(vol._p)
    zb, ze = slab or (0, 0)
    want = [ov.integrate_culled(dep, sc.bgra(i), tr, synth.cam_from_vol_f32(tr), zb, ze) for i, (tr, dep) in enumerate(zip(poses, depths))]
    assert res[0][1] == want
    zs = slice(*slab) if slab else slice(None)
    d, w, rgb = res[0][0]
    assert_same_f32(d, ov.d[zs], "d")
    assert np.array_equal(w, ov.w[zs]) and np.array_equal(rgb, ov.rgb[zs])


# ---- d. slabs and sets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
def test_z_slab_handle_under_the_family(gpu, color):
    """setZSlab(7, 23): topdown, axis_y and frombelow_rolled look across the slab's planes, axis_z along them."""
    res, zb, ze = 32, 7, 23
    ov, _ = family_oracle(res, color, 0, 100.0)
    vol, _ = family_volume(res, color)
    slab_ov = OracleVolume(vol._p)
    vol.setZSlab(zb, ze)
    vol.reset()
    for i, (name, tr, dep, col) in enumerate(family_frames(res)):
        c = col if color else None
        want = slab_ov.integrate_culled(dep, c, tr, synth.cam_from_vol_f32(tr), zb, ze)
        n = vol.integrateCloud(dep, c, tr, count=(i % 2 == 0))
        assert (n == want) if i % 2 == 0 else (n is True), (name, n, want)
    d, w, rgb = vol.download()
    assert_same_f32(d, ov.d[zb:ze], "slab d")
    assert_same_f32(w, ov.w[zb:ze], "slab w")
    assert not color or np.array_equal(rgb, ov.rgb[zb:ze])
    assert_same_f32(slab_ov.d[zb:ze], ov.d[zb:ze], "slab oracle vs whole oracle")
    vol.close()


@pytest.mark.parametrize("color", [False, True])
def test_device_set_under_the_family(gpu, color):
    """setDevices([0, 0, 0]): three slabs behind one handle, counts summed over the slabs."""
    res = 32
    ov, counts = family_oracle(res, color, 0, 100.0)
    vol, _ = family_volume(res, color)
    vol.setDevices([0, 0, 0])
    vol.reset()
    assert len(vol.slabs()) == 3
    for i, (name, tr, dep, col) in enumerate(family_frames(res)):
        n = vol.integrateCloud(dep, col if color else None, tr, count=(i % 2 == 0))
        assert (n == counts[i]) if i % 2 == 0 else (n is True), (name, n, counts[i])
    compare(vol, ov)
    vol.close()


# ---- e. renderView ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", [1, 2])
def test_render_view_from_rolled_poses(gpu, ds):
    """renderView of the fused 64^3 volume from rolled and axis-aligned cameras at radius 1.6 S against the oracle's
    raycast (pinned to the reference's renderView from these poses by tests/test_oracle_poses.py)."""
    res = 64
    ov, counts = family_oracle(res, True, 0, 100.0)
    vol, sc = family_volume(res, True)
    vol.reset()
    run_family(vol, res, True, counts, lambda info: True)
    compare(vol, ov)
    views = pose_cases.poses(sc.size, 1.6)
    for name in ("roll90", "axis_y", "diag", "roll-135"):
        got, want = vol.renderView(views[name], ds, camera_frame=False), ov.raycast(views[name], ds)
        hitm = np.isfinite(want[..., 0])
        assert hitm.sum() > 100, (name, int(hitm.sum()))
        assert np.array_equal(np.isfinite(got[..., 0]), hitm), name
        assert np.array_equal(got[hitm].view(np.uint32), want[hitm].view(np.uint32)), name
    vol.close()
