"""CPU tier: the boundary of reintegrateCloud -- include/tsdf_hip.h declares the three entry points and states the definition
above them, both libraries export them (and the product still nothing that is not tsdf_hip_*), the ctypes table and the
Python class carry them, the ABI version did not move, and calls without a handle are refused, not crashed."""
import ctypes as C
import inspect
import os
import re
import subprocess

from cpu_tsdf_amd import capi
from cpu_tsdf_amd.volume import TSDFVolumeOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tsdf_hip_reintegrate", "tsdf_hip_reintegrate_device", "tsdf_hip_reintegrate_stats"]
# ... const float cam_from_vol_old[12], const float *planes_old, const float cam_from_vol_new[12], const float *planes_new, uint64_t *n)
TAIL = (r"\s*const\s+float\s+cam_from_vol_old\[12\]\s*,\s*const\s+float\s*\*\s*planes_old\s*,\s*const\s+float\s+cam_from_vol_new\[12\]\s*,"
        r"\s*const\s+float\s*\*\s*planes_new\s*,\s*uint64_t\s*\*\s*n\s*\)")


def _header():
    txt = open(os.path.join(ROOT, "include", "tsdf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_declares_the_entry_points():
    txt = _header()
    assert re.search(r"\bint\s+tsdf_hip_reintegrate\s*\(\s*tsdf_handle\s+h\s*,\s*const\s+float\s*\*\s*depth\s*,\s*const\s+uint8_t\s*\*\s*bgra\s*," + TAIL, txt)
    assert re.search(r"\bint\s+tsdf_hip_reintegrate_device\s*\(\s*tsdf_handle\s+h\s*,\s*const\s+float\s*\*\s*d_depth\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*d_bgra\s*," + TAIL, txt)
    assert re.search(r"\bint\s+tsdf_hip_reintegrate_stats\s*\(\s*tsdf_handle\s+h\s*,\s*uint64_t\s+out\[6\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)


def test_the_header_states_the_definition_above_them():
    """The definition is ours (the reference has no such call): it stands where the other extensions state theirs."""
    txt = open(os.path.join(ROOT, "include", "tsdf_hip.h")).read()
    block = txt[:txt.index("int tsdf_hip_reintegrate(")].rsplit("/*", 1)[1]
    for phrase in ("NOT IN THE REFERENCE", "tsdf_hip_deintegrate", "planes_new", "tsdf_hip_create_multi"):
        assert phrase in block, phrase


def test_both_libraries_export_them_and_the_product_nothing_foreign():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"
        foreign = sorted(n for n in have if not n.startswith("tsdf_hip_"))
        assert not foreign, (os.path.basename(path), foreign)


def test_ctypes_table_and_python_class_carry_them():
    assert len(capi.SIGNATURES["tsdf_hip_reintegrate"][1]) == 8
    assert len(capi.SIGNATURES["tsdf_hip_reintegrate_device"][1]) == 8
    assert len(capi.SIGNATURES["tsdf_hip_reintegrate_stats"][1]) == 2
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(TSDFVolumeOctree.reintegrateCloud) == ["self", "depth", "bgra", "old_trans", "new_trans", "count"]
    assert params(TSDFVolumeOctree.reintegrateCloudDevice) == ["self", "depth_ptr", "bgra_ptr", "old_trans", "new_trans", "count"]
    assert params(TSDFVolumeOctree.reintegrateStats) == ["self"]
    sig = inspect.signature(TSDFVolumeOctree.reintegrateCloud)
    assert [sig.parameters[k].default for k in ("bgra", "old_trans", "new_trans", "count")] == [None, None, None, False]


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_calls_without_a_handle_are_refused_not_crashed():
    lib = capi.load()
    T = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    n = (C.c_uint64 * 2)(7, 9)
    out = (C.c_uint64 * 6)()
    assert lib.tsdf_hip_reintegrate(None, None, None, T, None, T, None, n) == capi.E_INVALID
    assert lib.tsdf_hip_reintegrate_device(None, None, None, T, None, T, None, n) == capi.E_INVALID
    assert (n[0], n[1]) == (7, 9)
    assert lib.tsdf_hip_reintegrate_stats(None, out) == capi.E_INVALID
    # every refusal that needs a live handle: tests/test_reintegrate_gpu.py::test_refusals_leave_the_planes_alone
