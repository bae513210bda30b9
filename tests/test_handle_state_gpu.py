"""GPU tier: what tsdf_hip_occupied, tsdf_hip_march_cleanup and tsdf_hip_march_flatten keep per handle lives IN the handle
(tsdf_hip_volume::occ / mp / fl, the mc_valid and mc_counts_pass fields): it dies with the handle, a new handle starts
without any of it, nothing stays allocated, and tsdf_hip_march_stats reports the flags as it always did.  One handle and a
two-slab set on device 0, on a 64^3 PACKED colour volume with 4 turntable frames: the smallest grid on which march,
occupied, cleanup and flatten all leave something behind."""
import ctypes as C

import pytest

from cpu_tsdf_amd import capi
from tests import flatten_cases as fc
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
RES = 64
FACE_DIST, MIN_NB = 1.5 * 2.0 ** -8, 3  # links of up to 1.5 voxels (the volume is 0.25 m across)
SHAPES = [None, [0, 0]]
IDS = ["one_handle", "set_0_0"]


def new_volume(devices):
    vol, sc = make_volume(RES, color=True)
    if devices:
        vol.setDevices(devices)
    vol.reset()
    assert vol.getLayout() == capi.LAYOUT_PACKED
    return vol, sc


def fuse(vol, sc):
    for i, tr, dep, col in frames(sc, 4, 8):
        vol.integrateCloud(dep, col, tr)
    vol.synchronize()


def feature_calls(lib, h):
    """march, occupied, cleanup, flatten: every one leaves a non-empty result on the handle."""
    n, occ, kept, m, k = (C.c_uint64(0) for _ in range(5))
    capi.check(lib.tsdf_hip_march(h, 1.0, 1, C.byref(n)), "march")
    capi.check(lib.tsdf_hip_occupied(h, None, C.byref(occ)), "occupied")
    capi.check(lib.tsdf_hip_march_cleanup(h, FACE_DIST, MIN_NB, C.byref(kept)), "march_cleanup")
    capi.check(lib.tsdf_hip_march_flatten(h, fc.MD, C.byref(m), C.byref(k)), "march_flatten")
    assert n.value > 1000 and occ.value > 1000 and 0 < kept.value <= n.value and 0 < m.value < 3 * kept.value and k.value > 0
    capi.check(lib.tsdf_hip_march_fetch_indexed(h, None, None, None, None), "march_fetch_indexed")
    st = (C.c_uint64 * 4)()
    capi.check(lib.tsdf_hip_occupied_stats(h, st), "occupied_stats")
    assert st[0] == occ.value and st[1] > 0


def march_stats(lib, h):
    st = (C.c_uint64 * 4)()
    capi.check(lib.tsdf_hip_march_stats(h, st), "march_stats")
    return [int(v) for v in st]


@pytest.mark.parametrize("devices", SHAPES, ids=IDS)
def test_state_dies_with_the_handle(gpu, devices):
    vol, sc = new_volume(devices)
    fuse(vol, sc)
    feature_calls(gpu, vol._need())
    old = vol._need().value
    vol.reset()  # destroy, and at once create the same shape: very likely at the same address
    h = vol._need()
    print("handle address reused:", h.value == old)
    n, m, k = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    st = (C.c_uint64 * 4)(9, 9, 9, 9)
    try:
        assert gpu.tsdf_hip_occupied_fetch(h, None, None, None, None) == capi.E_INVALID
        assert gpu.tsdf_hip_march_cleanup(h, FACE_DIST, MIN_NB, C.byref(n)) == capi.E_INVALID
        assert gpu.tsdf_hip_march_flatten(h, fc.MD, C.byref(m), C.byref(k)) == capi.E_INVALID
        assert gpu.tsdf_hip_march_fetch_indexed(h, None, None, None, None) == capi.E_INVALID
        capi.check(gpu.tsdf_hip_occupied_stats(h, st), "occupied_stats")
        assert list(st) == [0, 0, 0, 0]
    finally:
        vol.close()


@pytest.mark.parametrize("devices", SHAPES, ids=IDS)
def test_nothing_is_left_behind(gpu, devices):
    """Free device memory after the destroy of nine create / fuse / march / occupied / cleanup / flatten / destroy cycles.
    The footprint of what the four calls allocate is measured on the first (warm-up) cycle; a state object that outlived
    its handle would cost that much per cycle, eight times between the first destroy and the ninth.  Allowed: half of one."""
    import torch
    free = lambda: (torch.cuda.synchronize(), torch.cuda.mem_get_info()[0])[1]  # noqa: E731
    free()
    after_destroy, footprint = [], None
    for cycle in range(9):
        vol, sc = new_volume(devices)
        try:
            fuse(vol, sc)
            before = free()
            feature_calls(gpu, vol._need())
            if cycle == 0:
                footprint = before - free()
        finally:
            vol.close()
        after_destroy.append(free())
    print("footprint", footprint, "free after each destroy", after_destroy)
    assert footprint > 0
    assert after_destroy[0] - after_destroy[8] <= footprint // 2, (footprint, after_destroy)


def test_march_flags_read_as_before(gpu):
    """tsdf_hip_march_stats out[3]: bit 0 the band flags decided what classify read, bit 1 the corner weights were not
    gathered -- fields of the handle now, no longer bit 63 of the byte count in out[2]."""
    vol, sc = new_volume(None)
    try:
        fuse(vol, sc)  # flag-keeping launches only
        h, n = vol._need(), C.c_uint64(0)
        capi.check(gpu.tsdf_hip_march(h, 0.0, 1, C.byref(n)), "march")
        st = march_stats(gpu, h)
        assert st[3] == 3 and 0 < st[2] < 2 ** 63 and st[1] == n.value > 1000
        vol.device_planes()  # hands out raw pointers: band_exact goes, and with it both elisions
        capi.check(gpu.tsdf_hip_march(h, 0.0, 1, C.byref(n)), "march")
        after = march_stats(gpu, h)
        assert after[3] & 1 == 0 and after[3] == 0 and st[2] <= after[2] < 2 ** 63 and after[1] == st[1]
    finally:
        vol.close()


def test_march_flags_of_a_set_read_as_before(gpu):
    vol, sc = new_volume([0, 0])
    try:
        fuse(vol, sc)
        h, n = vol._need(), C.c_uint64(0)
        capi.check(gpu.tsdf_hip_march(h, 0.0, 1, C.byref(n)), "march")
        st = march_stats(gpu, h)
        # a bit of out[3] on a set means EVERY slab set it: the flags decided what each slab's classify read (bit 0), and no slab
        # gathered corner weights (bit 1) -- the lower slab neither, whose top cells end on a halo plane: that plane is a fresh
        # copy of a plane the upper slab's own integrate launches wrote.  The single-handle twin above reads 3 as well
        assert st[3] == 3 and 0 < st[2] < 2 ** 63 and st[1] == n.value > 1000
    finally:
        vol.close()
