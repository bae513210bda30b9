"""The launches of tests/test_integrate_counters_gpu.py: one list of cases, and the code that runs a case and reads every
counter back, shared by the test and by the recorder of tests/golden/integrate_counters.json (a plain module: no pytest).

A case = one kernel family, selected through the tuning knobs and confirmed by tsdf_hip_last_launch_info after each launch:
a 64^3 grid, 160x120 frames, three noisy frames with NaN holes, counting on every launch, 64 and 40 rows per block (at 40
the last block of a column has 24 of its 40 rows)."""
import ctypes as C
import functools

import numpy as np

from cpu_tsdf_amd import capi, synth
from tests.common import make_volume

RES, W, H = 64, 160, 120
ROWS_PER_BLOCK = (64, 40)
# name -> colour, layout, knob pipe, knob fuse2, camera inside the grid, what tsdf_hip_last_launch_info must say:
# (kernel in the low byte of out[0], the pipelined row loop, row intervals)
CASES = {
    "k_integrate packed": (False, capi.LAYOUT_PACKED, 0, 1, False, (1, False, False)),
    "k_integrate packed colour": (True, capi.LAYOUT_PACKED, 0, 1, False, (1, False, False)),
    "k_integrate f32w": (False, capi.LAYOUT_F32W, 0, 1, False, (1, False, False)),
    "k_integrate live": (True, capi.LAYOUT_PACKED, 0, 1, True, (0, False, True)),
    "k_integrate_p": (False, capi.LAYOUT_PACKED, 1, 1, False, (1, True, False)),
    "k_integrate2": (False, capi.LAYOUT_PACKED, 1, 2, False, (2, False, False)),
    "k_integrate2 colour": (True, capi.LAYOUT_PACKED, 1, 2, False, (2, False, False)),
}
PAIRS = ((0, 1), (2, 0))  # the k_integrate2 cases: two sweeps over the three frames


def restore_knobs():
    """The knobs' defaults, as the suite's other modules put them back (the test library has no hook that reads a knob)."""
    capi.set_tuning("pipe", 1)
    capi.set_tuning("fuse2", 1)
    capi.set_tuning("rows_per_block", 64)


@functools.lru_cache(maxsize=None)
def frames(inside):
    """[(pose, depth, bgra)]: Scene A seen from three turntable poses (or from inside the grid), depth noise, and in every
    frame a band of rows and a lattice of pixels without a return."""
    sc = synth.scene_a(RES, W, H)
    out = []
    for i in range(3):
        tr = synth.look_at_pose((0.02 * i, 0.01, -0.03), target=(0.05, 0.0, 1.0)) if inside else synth.turntable_pose(i, 8, sc.size)
        dep = sc.depth(tr, noise_seed=777 + i)
        dep[20 + 30 * i:26 + 30 * i, :] = np.nan
        dep[(7 * i) % 50::53, ::3] = np.nan
        dep.setflags(write=False)
        out.append((tr, dep, sc.bgra(i)))
    return tuple(out)


def sequence(name):
    """The frames a case integrates, in order (what an oracle has to follow)."""
    fr = frames(CASES[name][4])
    return [fr[i] for pair in PAIRS for i in pair] if CASES[name][3] == 2 else list(fr)


def _detail(vol):
    lib, h = capi.load(), vol._need()
    info, cd, rd = (C.c_int32 * 4)(), (C.c_uint64 * 2)(), (C.c_uint64 * 3)()
    capi.check(lib.tsdf_hip_last_launch_info(h, info), "last_launch_info")
    capi.check(lib.tsdf_hip_last_count_detail(h, cd), "last_count_detail")
    capi.check(lib.tsdf_hip_last_read_detail(h, rd), "last_read_detail")
    family = (int(info[0]) & 0xff, bool(int(info[0]) & 0x100), int(info[2]) != 0)
    return family, int(info[3]), [int(x) for x in cd], [int(x) for x in rd]


def run(name, rows_per_block):
    """The case's launches on a fresh volume.  Returns (records, blocks): one record per launch -- the observation count the
    call returned (a pair for k_integrate2), tsdf_hip_last_count_detail and tsdf_hip_last_read_detail -- and the blocks each
    launch had; the kernel family is asserted."""
    import torch
    color, layout, pipe, fuse2, inside, want = CASES[name]
    fr = frames(inside)
    out, blocks = [], []
    vol = None
    try:
        capi.set_tuning("pipe", pipe)
        capi.set_tuning("fuse2", fuse2)
        capi.set_tuning("rows_per_block", rows_per_block)
        vol, _ = make_volume(RES, W, H, color=color)
        vol.setLayout(layout)
        vol.reset()
        if fuse2 == 2:
            dev = []
            for tr, dep, col in fr:
                t = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
                t[0].copy_(torch.from_numpy(np.array(dep)))
                t[1].view(torch.uint8).view(H, W, 4).copy_(torch.from_numpy(col))
                dev.append((t, (t[0].data_ptr(), t[1].data_ptr() if color else 0, tr)))
            for ia, ib in PAIRS:
                fused, n = vol.integrateCloudDevice2(dev[ia][1], dev[ib][1], count=True)
                family, nb, cd, rd = _detail(vol)
                assert fused and family == want, (name, rows_per_block, fused, family)
                out.append({"n": n, "count_detail": cd, "read_detail": rd})
                blocks.append(nb)
        else:
            for tr, dep, col in fr:
                n = vol.integrateCloud(dep, col if color else None, tr, count=True)
                family, nb, cd, rd = _detail(vol)
                assert family == want, (name, rows_per_block, family)
                out.append({"n": n, "count_detail": cd, "read_detail": rd})
                blocks.append(nb)
    finally:
        restore_knobs()
        if vol is not None:
            vol.close()
    return out, blocks
