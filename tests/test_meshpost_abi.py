"""CPU tier: the boundary of cleanupMesh on the GPU -- include/tsdf_hip.h declares the entry points, both builds of the
library export them, the ctypes table and the Python classes carry them, the ABI version did not move, and bad arguments are
refused before any device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from cpu_tsdf_amd import capi, volume
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tsdf_hip_mesh_cleanup", "tsdf_hip_march_cleanup", "tsdf_hip_mesh_cleanup_stats"]


def _header(name="tsdf_hip.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_declares_the_entry_points():
    txt = _header()
    assert re.search(r"\bint\s+tsdf_hip_mesh_cleanup\s*\(\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*const\s+uint32_t\s*\*\s*"
                     r"\w+\s*,\s*uint64_t\s+\w+\s*,\s*float\s+\w+\s*,\s*int\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_march_cleanup\s*\(\s*tsdf_handle\s+\w+\s*,\s*float\s+\w+\s*,\s*int\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_mesh_cleanup_stats\s*\(\s*uint64_t\s+\w+\[4\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)
    # no test hook came with it
    assert "cleanup" not in _header("tsdf_hip_test.h")


def test_both_libraries_export_them():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"


def test_ctypes_table_and_python_classes_carry_them():
    for name in ENTRY_POINTS:
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in cpu_tsdf_amd/capi.py"
    assert len(capi.SIGNATURES["tsdf_hip_mesh_cleanup"][1]) == 9
    assert len(capi.SIGNATURES["tsdf_hip_march_cleanup"][1]) == 4
    assert len(capi.SIGNATURES["tsdf_hip_mesh_cleanup_stats"][1]) == 1
    sig = inspect.signature(MarchingCubesTSDFOctree.setCleanup)
    assert list(sig.parameters) == ["self", "face_dist", "min_neighbors"]
    assert sig.parameters["face_dist"].default == 0.02 and sig.parameters["min_neighbors"].default == 5
    assert callable(getattr(MarchingCubesTSDFOctree, "clearCleanup", None))
    sig = inspect.signature(volume.cleanup_mesh)
    assert list(sig.parameters) == ["vertices", "polygons", "face_dist", "min_neighbors", "device"]
    assert [sig.parameters[k].default for k in ("polygons", "face_dist", "min_neighbors", "device")] == [None, 0.02, 5, 0]
    mc = MarchingCubesTSDFOctree()
    mc.setCleanup()
    assert mc._cleanup == (0.02, 5)
    mc.clearCleanup()
    assert mc._cleanup is None


def test_cpp_class_declares_the_setters():
    txt = open(os.path.join(ROOT, "include", "cpu_tsdf", "marching_cubes_tsdf_octree.h")).read()
    assert re.search(r"void\s+setCleanup\s*\(\s*float\s+face_dist\s*=\s*0\.02f\s*,\s*int\s+min_neighbors\s*=\s*5\s*\)", txt)
    assert re.search(r"void\s+clearCleanup\s*\(\s*\)", txt)


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    lib = capi.load()
    n = C.c_uint64(7)
    assert lib.tsdf_hip_march_cleanup(None, 0.02, 5, C.byref(n)) == capi.E_INVALID
    assert lib.tsdf_hip_mesh_cleanup_stats(None) == capi.E_INVALID
    verts = np.zeros((6, 3), np.float32)
    keep = np.zeros(2, np.uint8)
    vp, kp = capi.as_f32p(verts), capi.as_u8p(keep)

    def call(v=vp, nv=6, nf=2, dist=0.02, mn=5, k=kp, device=0):
        return lib.tsdf_hip_mesh_cleanup(device, v, nv, None, nf, dist, mn, k, C.byref(n))

    for bad in (0.0, -0.02, float("nan"), float("inf")):
        assert call(dist=bad) == capi.E_INVALID, bad
    assert call(mn=-1) == capi.E_INVALID
    assert call(v=None) == capi.E_INVALID
    assert call(k=None) == capi.E_INVALID
    assert call(nv=5) == capi.E_INVALID          # a soup of 2 faces needs 6 vertices
    assert call(nf=(1 << 31) + 1) == capi.E_INVALID  # face indices are 32-bit
    assert call(device=-1) == capi.E_INVALID
    assert n.value == 0
    # no face: nothing to do, whatever else is passed, and no device needed
    n.value = 7
    assert call(v=None, nv=0, nf=0, k=None) == capi.OK and n.value == 0
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.tsdf_hip_mesh_cleanup_stats(out) == capi.OK and list(out) == [0, 0, 0, 0]


def test_cpp_class_keeps_the_size_it_had(tmp_path):
    """the drop-in classes keep their size and layout between releases of the shell library, so a binary
    compiled against an earlier header and only re-linked keeps working.  The mesher holds what the reference's holds -- the
    volume pointer, two flags, the minimum weight -- and nothing else: setCleanup's arguments live in the shell library."""
    from cpu_tsdf_amd import build as b
    src = tmp_path / "layout.cpp"
    src.write_text("""
#include <cpu_tsdf/marching_cubes_tsdf_octree.h>
struct AsBefore : public pcl::MarchingCubes<pcl::PointXYZ> {
  void voxelizeData() override {}
  void performReconstruction(pcl::PolygonMesh &) override {}
  void performReconstruction(pcl::PointCloud<pcl::PointXYZ> &, std::vector<pcl::Vertices> &) override {}
  cpu_tsdf::TSDFVolumeOctree::ConstPtr tsdf_volume_;
  bool color_by_confidence_, color_by_rgb_;
  float w_min_;
};
static_assert(sizeof(cpu_tsdf::MarchingCubesTSDFOctree) == sizeof(AsBefore), "MarchingCubesTSDFOctree changed its size");
int main() { return 0; }
""")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + ["-fsyntax-only", str(src)])
