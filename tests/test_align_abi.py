"""CPU tier: the boundary of alignCloud -- include/tsdf_hip.h declares the four entry points, both builds of the library
export them, the ctypes table and the Python and C++ classes carry them, the ABI version did not move, bad arguments are
refused before any device is touched -- and the host arithmetic of tsdf_hip_align (cpu_tsdf_amd/csrc/tsdf_se3.h: the SE(3)
exponential, the Cholesky step) against numpy.

The exponential reaches the test through tests/harness/se3.cpp, a host program that includes the header tsdf_align.hip
includes, NOT through a tsdf_hip_selftest_* hook: tests/test_abi.py pins the hooks of include/tsdf_hip_test.h to the 18 it
has, and the arithmetic needs no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from cpu_tsdf_amd import capi, volume
from cpu_tsdf_amd.volume import TSDFVolumeOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tsdf_hip_align_system", "tsdf_hip_align_system_device", "tsdf_hip_align", "tsdf_hip_align_stats"]
F64P = C.POINTER(C.c_double)


def _header(name="tsdf_hip.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_declares_the_entry_points():
    txt = _header()
    w, s, a = r"\s+\w+\s*", r"\s*\*\s*\w+\s*", r"\s+\w+\s*\[\s*{}\s*\]\s*"
    assert re.search(r"\bint\s+tsdf_hip_align_system\s*\(\s*tsdf_handle" + w + r",\s*const\s+float" + s + r",\s*size_t" + w + r",\s*const\s+double" +
                     a.format(12) + r",\s*float" + w + r",\s*float" + w + r",\s*double" + a.format(29) + r",\s*uint8_t" + s + r",\s*float" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_align_system_device\s*\(\s*tsdf_handle" + w + r",\s*const\s+float" + s + r",\s*size_t" + w +
                     r",\s*const\s+double" + a.format(12) + r",\s*float" + w + r",\s*float" + w + r",\s*double" + a.format(29) + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_align\s*\(\s*tsdf_handle" + w + r",\s*const\s+float" + s + r",\s*size_t" + w + r",\s*const\s+double" +
                     a.format(12) + r",\s*float" + w + r",\s*float" + w + r",\s*int" + w + r",\s*double" + w + r",\s*double" + a.format(12) +
                     r",\s*int32_t" + s + r",\s*double" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_align_stats\s*\(\s*tsdf_handle" + w + r",\s*uint64_t\s+\w+\[4\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)
    assert re.search(r"TSDF_HIP_ALIGN_NO_POINTS\s*=\s*7\b", txt) and re.search(r"TSDF_HIP_ALIGN_RANK_DEFICIENT\s*=\s*8\b", txt)
    # the declaration says what is not the reference's, and what every reading entry point says
    full = open(os.path.join(ROOT, "include", "tsdf_hip.h")).read()
    assert "NOT IN THE REFERENCE" in full and "the reference's getFxn ignores weights" in full and "held back by frame pairing" in full
    assert "align" not in _header("tsdf_hip_test.h").lower()


def test_both_libraries_export_them():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"


def test_ctypes_table_and_python_classes_carry_them():
    for name, n_args in zip(ENTRY_POINTS, (9, 7, 11, 2)):
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in cpu_tsdf_amd/capi.py"
        assert len(capi.SIGNATURES[name][1]) == n_args
    assert capi.SIGNATURES["tsdf_hip_align"][1][3:8] == [F64P, C.c_float, C.c_float, C.c_int, C.c_double]
    assert (capi.ALIGN_NO_POINTS, capi.ALIGN_RANK_DEFICIENT) == (7, 8)
    sig = inspect.signature(TSDFVolumeOctree.alignmentSystem)
    assert list(sig.parameters) == ["self", "points", "trans", "min_weight", "r_max", "want_used", "want_points"]
    assert [sig.parameters[k].default for k in ("min_weight", "r_max", "want_used", "want_points")] == [0.0, 0.9, False, False]
    sig = inspect.signature(TSDFVolumeOctree.alignCloud)
    assert list(sig.parameters) == ["self", "points", "guess", "max_iterations", "min_weight", "r_max", "min_step"]
    assert [sig.parameters[k].default for k in ("max_iterations", "min_weight", "r_max", "min_step")] == [10, 0.0, 0.9, 1e-7]
    assert list(inspect.signature(volume.backproject).parameters) == ["depth", "fx", "fy", "cx", "cy"]


def test_backproject_is_the_stated_arithmetic():
    rng = np.random.RandomState(5)
    dep = rng.uniform(0.3, 2.0, (7, 9)).astype(np.float32)
    dep[2, 3] = dep[6, 8] = np.nan
    fx, fy, cx, cy = 131.25, 129.5, 4.3, 3.1
    got = volume.backproject(dep, fx, fy, cx, cy)
    want = [[np.float32((u - cx) / fx * float(dep[v, u])), np.float32((v - cy) / fy * float(dep[v, u])), dep[v, u]]
            for v in range(7) for u in range(9) if not np.isnan(dep[v, u])]
    assert got.dtype == np.float32 and got.shape == (7 * 9 - 2, 3) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, np.array(want, np.float32))


def test_cpp_class_declares_the_members():
    txt = open(os.path.join(ROOT, "include", "cpu_tsdf", "tsdf_volume_octree.h")).read()
    assert re.search(r"template\s*<\s*typename\s+PointT\s*>\s*bool\s+alignCloud\s*\(\s*const\s+pcl::PointCloud<PointT>\s*&\s*cloud\s*,\s*const\s+Eigen::Affine3d\s*&"
                     r"\s*guess\s*,\s*Eigen::Affine3d\s*&\s*refined\s*,\s*int\s+max_iterations\s*=\s*10\s*,\s*float\s+min_weight\s*=\s*0\.f\s*,"
                     r"\s*float\s+r_max\s*=\s*0\.9f\s*,\s*double\s+min_step\s*=\s*1e-7\s*\)\s*const\s*;", txt)
    assert re.search(r"bool\s+getAlignmentSystem\s*\(\s*const\s+float\s*\*\s*xyz\s*,\s*size_t\s+n\s*,\s*const\s+Eigen::Affine3d\s*&\s*trans\s*,\s*double\s+out\[29\]\s*,"
                     r"\s*float\s+min_weight\s*=\s*0\.f\s*,\s*float\s+r_max\s*=\s*0\.9f\s*\)\s*const\s*;", txt)
    assert "virtual" not in txt.split("alignCloud")[1].split("const float UNOBSERVED_VOXEL")[0]


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    assert b"gate" in lib.tsdf_hip_error_string(capi.ALIGN_NO_POINTS) and b"freedoms" in lib.tsdf_hip_error_string(capi.ALIGN_RANK_DEFICIENT)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    lib = capi.load()
    xyz = np.zeros((4, 3), np.float32)
    T = np.eye(4)[:3].copy().reshape(12)
    out, ref = np.full(29, 7.0), np.full(12, 7.0)
    it = C.c_int32(7)
    xp, tp, op, rp = capi.as_f32p(xyz), T.ctypes.data_as(F64P), out.ctypes.data_as(F64P), ref.ctypes.data_as(F64P)
    # no handle: refused whatever else is passed -- nothing to run on
    assert lib.tsdf_hip_align_system(None, xp, 4, tp, 0.0, 0.9, op, None, None) == capi.E_INVALID
    assert lib.tsdf_hip_align_system_device(None, xp, 4, tp, 0.0, 0.9, op) == capi.E_INVALID
    assert lib.tsdf_hip_align(None, xp, 4, tp, 0.0, 0.9, 10, 1e-7, rp, C.byref(it), None) == capi.E_INVALID
    assert lib.tsdf_hip_align_stats(None, None) == capi.E_INVALID
    assert np.all(out == 7.0) and np.all(ref == 7.0) and it.value == 7


# ---- the host arithmetic -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def se3(tmp_path_factory):
    from cpu_tsdf_amd import build as b
    d = tmp_path_factory.mktemp("se3")
    exe = str(d / "se3")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-I" + b.CSRC, os.path.join(ROOT, "tests", "harness", "se3.cpp"),
                           "-o", exe])

    def run(mode, rows):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rows, np.float64).tofile(src)
        subprocess.run([exe, mode, src, dst], check=True, timeout=60)
        return np.fromfile(dst, np.float64).reshape(len(rows), -1)
    return run


def expm_series(xi):
    """exp of the 4 x 4 twist matrix by its power series after scaling and squaring (numpy only), in extended precision:
    the squarings double the rounding error each time, which long double (2^-64) absorbs and double would not."""
    M = np.zeros((4, 4), np.longdouble)
    wx, wy, wz = xi[:3]
    M[:3, :3] = [[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]]
    M[:3, 3] = xi[3:]
    k = max(0, int(np.ceil(np.log2(max(np.abs(M).sum(1).max(), 1e-300)))) + 4)
    A = M / np.longdouble(2.0) ** k
    E, term = np.eye(4, dtype=np.longdouble), np.eye(4, dtype=np.longdouble)
    for j in range(1, 30):
        term = term @ A / np.longdouble(j)
        E = E + term
    for _ in range(k):
        E = E @ E
    assert np.finfo(np.longdouble).eps < 2e-19
    return E.astype(np.float64)


TWISTS = np.array([[0, 0, 0, 0.3, -0.2, 0.1], [0, 0, 0, 0, 0, 0], [1e-13, -2e-13, 1e-13, 0.5, 0.25, -1.0], [1e-9, 2e-9, -1e-9, 0.1, 0.2, 0.3],
                   [1e-5, 0, 3e-5, -0.4, 0.2, 0.9], [0.018, -0.015, 0.0186, 0.0059, 0.0082, -0.0059], [0.3, -0.2, 0.5, 0.1, -0.7, 0.2],
                   [1.0, 2.0, -1.5, 0.3, 0.3, 0.3], [0, 0, 3.0, 1.0, 0, 0]], np.float64)


def test_se3_exponential_equals_the_matrix_exponential(se3):
    got = se3("exp", TWISTS)
    assert np.sum(np.linalg.norm(TWISTS[:, :3], axis=1) == 0) == 2
    for xi, T in zip(TWISTS, got):
        want = expm_series(xi)
        err = np.abs(T.reshape(3, 4) - want[:3]).max()
        assert err <= 1e-15 * max(1.0, np.abs(want).max()), (xi, err)
    assert np.array_equal(got[1].reshape(3, 4), np.eye(4)[:3])


def _sys29(A, b, c=1.0, n=10.0):
    return np.concatenate([A[np.triu_indices(6)], b, [c, n]])


def test_cholesky_step_solves_the_normal_equations_and_refuses_a_missing_freedom(se3):
    rng = np.random.RandomState(11)
    rows, want = [], []
    for k in range(6):
        J = rng.normal(size=(40, 6)) * np.array([0.1, 0.1, 0.1, 1, 1, 1]) * 10.0 ** rng.uniform(-1, 1)
        A, b = J.T @ J, J.T @ rng.normal(size=40)
        rows.append(_sys29(A, b))
        want.append((np.linalg.solve(A, -b), np.linalg.cond(A)))
    got = se3("solve", np.array(rows))
    for g, (x, cond) in zip(got, want):
        assert g[0] == 0
        assert np.abs(g[1:] - x).max() <= 50 * cond * 2.0 ** -53 * np.abs(x).max(), (g, x, cond)
    # one plane z = const: g = (0, 0, 1), J = (y, -x, 0, 0, 0, 1) -- three freedoms unconstrained; the same with rounding noise
    # of 1e-7 relative in the gradient; no point at all; a NaN
    q = rng.uniform(-0.1, 0.1, (200, 3))
    J = np.stack([q[:, 1], -q[:, 0], 0 * q[:, 0], 0 * q[:, 0], 0 * q[:, 0], 1 + 0 * q[:, 0]], 1)
    Jn = J + 1e-7 * rng.normal(size=J.shape)
    bad = [_sys29(J.T @ J, J.T @ q[:, 2]), _sys29(Jn.T @ Jn, Jn.T @ q[:, 2]), np.zeros(29), _sys29(np.full((6, 6), np.nan), np.zeros(6))]
    assert np.all(se3("solve", np.array(bad))[:, 0] == 1)
