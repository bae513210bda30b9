"""CPU tier: the boundary of shiftVolume -- include/tsdf_hip.h declares the two entry points, both builds of the library
export them, the ctypes table and the Python class carry them, the ABI version did not move, and calls without a handle or
a shift are refused, not crashed.  The roll-with-fill helper the GPU tests compare against is checked against np.roll."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import TSDFVolumeOctree
from tests import shift_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tsdf_hip_shift", "tsdf_hip_shift_stats"]


def _header():
    txt = open(os.path.join(ROOT, "include", "tsdf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_declares_the_entry_points():
    txt = _header()
    assert re.search(r"\bint\s+tsdf_hip_shift\s*\(\s*tsdf_handle\s+\w+\s*,\s*const\s+int32_t\s+\w+\[3\]\s*\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_shift_stats\s*\(\s*tsdf_handle\s+\w+\s*,\s*uint64_t\s+\w+\[4\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)


def test_both_libraries_export_them():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"


def test_ctypes_table_and_python_class_carry_them():
    for name in ENTRY_POINTS:
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in cpu_tsdf_amd/capi.py"
        assert len(capi.SIGNATURES[name][1]) == 2
    assert list(inspect.signature(TSDFVolumeOctree.shiftVolume).parameters) == ["self", "sx", "sy", "sz"]
    assert list(inspect.signature(TSDFVolumeOctree.shiftStats).parameters) == ["self"]


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_calls_without_a_handle_or_a_shift_are_refused_not_crashed():
    lib = capi.load()
    s = (C.c_int32 * 3)(1, 2, 3)
    out = (C.c_uint64 * 4)()
    assert lib.tsdf_hip_shift(None, s) == capi.E_INVALID
    assert lib.tsdf_hip_shift(None, None) == capi.E_INVALID
    assert lib.tsdf_hip_shift_stats(None, out) == capi.E_INVALID
    # a NULL shift on a live handle needs a device: tests/test_shift_gpu.py::test_errors_and_no_ops


def test_the_helper_is_a_roll_with_fill():
    rng = np.random.RandomState(3)
    a = rng.randint(1, 100, (5, 6, 7)).astype(np.float32)
    for s in [(0, 0, 0), (1, 0, 0), (-2, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 2), (0, 0, -4), (3, -2, 1), (7, 0, 0), (0, -6, 0), (0, 0, 9), (-20, 1, 1)]:
        got = sc.shifted(a, s, -1.0)
        big = np.full((15, 18, 21), -1.0, np.float32)  # the grid in the middle of a grid three times its size: a roll cannot wrap
        big[5:10, 6:12, 7:14] = a
        c = tuple(max(-n, min(n, v)) for v, n in zip(s, (7, 6, 5)))
        want = np.roll(big, (-c[2], -c[1], -c[0]), axis=(0, 1, 2))[5:10, 6:12, 7:14]
        assert np.array_equal(got, want), s
        assert int((got == -1.0).sum()) == sc.reset_count(a.shape, s), s
    rgb = rng.randint(1, 255, (5, 6, 7, 3)).astype(np.uint8)
    got = sc.shifted(rgb, (1, 2, -1), 0)
    assert np.array_equal(got[1:, :4, :6], rgb[:4, 2:, 1:]) and not got[0].any() and not got[:, 4:].any() and not got[:, :, 6:].any()
