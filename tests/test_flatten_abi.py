"""CPU tier: the boundary of flattenVertices on the GPU -- include/tsdf_hip.h declares the four entry points, both builds of
the library export them, the ctypes table and the Python and C++ classes carry them, the ABI version did not move, no test
hook came along, and bad arguments are refused before any device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from cpu_tsdf_amd import capi, volume
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tsdf_hip_mesh_flatten", "tsdf_hip_march_flatten", "tsdf_hip_march_fetch_indexed", "tsdf_hip_mesh_flatten_stats"]
U32P = C.POINTER(C.c_uint32)


def _header(name="tsdf_hip.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_declares_the_entry_points():
    txt = _header()
    w, s = r"\s+\w+\s*", r"\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+tsdf_hip_mesh_flatten\s*\(\s*int" + w + r",\s*const\s+float" + s + r",\s*uint64_t" + w + r",\s*const\s+uint32_t" + s +
                     r",\s*uint64_t" + w + r",\s*float" + w + r",\s*uint32_t" + s + r",\s*uint32_t" + s + r",\s*uint64_t" + s + r",\s*uint32_t" + s +
                     r",\s*uint64_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_march_flatten\s*\(\s*tsdf_handle" + w + r",\s*float" + w + r",\s*uint64_t" + s + r",\s*uint64_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_march_fetch_indexed\s*\(\s*tsdf_handle" + w + r",\s*float" + s + r",\s*uint8_t" + s + r",\s*uint32_t" + s +
                     r",\s*uint64_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_mesh_flatten_stats\s*\(\s*uint64_t\s+\w+\[4\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)
    # the comment states the rules and the cost
    full = open(os.path.join(ROOT, "include", "tsdf_hip.h")).read()
    assert "integrate.cpp:103-150" in full and "HIGHEST-indexed seed" in full and "Rounds = the depth" in full
    # no test hook came with it
    assert "flatten" not in _header("tsdf_hip_test.h").lower()


def test_both_libraries_export_them():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"


def test_ctypes_table_and_python_classes_carry_them():
    for name, n_args in zip(ENTRY_POINTS, (11, 4, 5, 1)):
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in cpu_tsdf_amd/capi.py"
        assert len(capi.SIGNATURES[name][1]) == n_args
    sig = inspect.signature(MarchingCubesTSDFOctree.setFlatten)
    assert list(sig.parameters) == ["self", "min_dist"] and sig.parameters["min_dist"].default == 0.0001
    assert callable(getattr(MarchingCubesTSDFOctree, "clearFlatten", None))
    sig = inspect.signature(volume.flatten_mesh)
    assert list(sig.parameters) == ["vertices", "polygons", "min_dist", "device"]
    assert [sig.parameters[k].default for k in ("polygons", "min_dist", "device")] == [None, 0.0001, 0]
    mc = MarchingCubesTSDFOctree()
    assert mc._flatten is None
    mc.setFlatten()
    assert mc._flatten == 0.0001
    mc.clearFlatten()
    assert mc._flatten is None
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        try:
            mc.setFlatten(bad)
        except ValueError:
            continue
        raise AssertionError(f"setFlatten({bad}) was accepted")


def test_cpp_class_declares_the_setters_and_the_program_uses_the_auto_pass():
    txt = open(os.path.join(ROOT, "include", "cpu_tsdf", "marching_cubes_tsdf_octree.h")).read()
    assert re.search(r"void\s+setFlatten\s*\(\s*float\s+min_dist\s*=\s*0\.0001f\s*\)", txt)
    assert re.search(r"void\s+clearFlatten\s*\(\s*\)", txt)
    post = open(os.path.join(ROOT, "cpu_tsdf_amd", "csrc", "prog", "mesh_post.h")).read()
    assert re.search(r"inline\s+int\s+flattenVerticesGpu\s*\(\s*pcl::PolygonMesh\s*&\s*mesh\s*,\s*float\s+min_dist\s*=\s*0\.0001f\s*,\s*int\s+device\s*=\s*0\s*\)", post)
    assert re.search(r"inline\s+int\s+flattenVerticesAuto\s*\(", post) and "TSDF_HIP_HOST_MESH_POST" in post
    prog = open(os.path.join(ROOT, "cpu_tsdf_amd", "csrc", "prog", "integrate.cpp")).read()
    assert "flattenVerticesAuto(mesh)" in prog


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    lib = capi.load()
    m, k = C.c_uint64(7), C.c_uint64(7)
    assert lib.tsdf_hip_march_flatten(None, 1e-4, C.byref(m), C.byref(k)) == capi.E_INVALID
    assert lib.tsdf_hip_march_fetch_indexed(None, None, None, None, None) == capi.E_INVALID
    assert lib.tsdf_hip_mesh_flatten_stats(None) == capi.E_INVALID
    verts = np.zeros((6, 3), np.float32)
    remap, seeds = np.zeros(6, np.uint32), np.zeros(6, np.uint32)
    faces = np.zeros((2, 3), np.uint32)
    vp, rp, sp, fp = capi.as_f32p(verts), remap.ctypes.data_as(U32P), seeds.ctypes.data_as(U32P), faces.ctypes.data_as(U32P)

    def call(v=vp, nv=6, f=None, nf=2, md=1e-4, device=0, nov=C.byref(m), nof=C.byref(k)):
        return lib.tsdf_hip_mesh_flatten(device, v, nv, f, nf, md, rp, sp, nov, fp, nof)

    for bad in (0.0, -1e-4, float("nan"), float("inf")):
        assert call(md=bad) == capi.E_INVALID, bad
    assert call(device=-1) == capi.E_INVALID
    assert call(v=None) == capi.E_INVALID
    assert call(nov=None) == capi.E_INVALID          # seeds are asked for: the count has to go somewhere
    assert call(nof=None) == capi.E_INVALID
    assert call(nv=5) == capi.E_INVALID              # a soup of 2 faces needs 6 vertices
    assert call(nv=(1 << 31) + 1) == capi.E_INVALID  # indices are 32-bit
    assert call(f=fp, nf=(1 << 31) + 1) == capi.E_INVALID
    assert call(nv=0, f=fp, nf=2) == capi.E_INVALID  # every face names a vertex >= n_verts
    assert m.value == 0 and k.value == 0
    # no vertex: nothing to do, and no device needed
    m.value = k.value = 7
    assert call(v=None, nv=0, nf=0) == capi.OK and m.value == 0 and k.value == 0
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.tsdf_hip_mesh_flatten_stats(out) == capi.OK and list(out) == [0, 0, 0, 0]


def test_cpp_class_keeps_the_size_it_had(tmp_path):
    """As tests/test_meshpost_abi.py checks for setCleanup: setFlatten's argument lives in the shell library, not in the
    object, and both setters link."""
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
int main() {
  cpu_tsdf::MarchingCubesTSDFOctree mc;
  mc.setFlatten();
  mc.setFlatten(0.5f);
  mc.clearFlatten();
  return 0;
}
""")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [str(src), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                                                                            "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    subprocess.run([exe], check=True, timeout=60)
