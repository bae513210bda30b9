"""CPU tier: the boundary of decimateMesh on the GPU -- include/tsdf_hip.h declares the three entry points, both builds of the
library export them, the ctypes table and the Python and C++ classes carry them, the ABI version did not move, no test hook
came along, and every refusal that needs no device is given before one is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from cpu_tsdf_amd import capi, volume
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tsdf_hip_mesh_decimate", "tsdf_hip_march_decimate", "tsdf_hip_mesh_decimate_stats"]
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
    assert re.search(r"\bint\s+tsdf_hip_mesh_decimate\s*\(\s*int" + w + r",\s*const\s+float" + s + r",\s*const\s+uint8_t" + s + r",\s*uint64_t" + w +
                     r",\s*const\s+uint32_t" + s + r",\s*uint64_t" + w + r",\s*float" + w + r",\s*uint32_t" + s + r",\s*float" + s + r",\s*uint8_t" + s +
                     r",\s*uint32_t" + s + r",\s*uint64_t" + s + r",\s*uint32_t" + s + r",\s*uint64_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_march_decimate\s*\(\s*tsdf_handle" + w + r",\s*float" + w + r",\s*uint64_t" + s + r",\s*uint64_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_mesh_decimate_stats\s*\(\s*uint64_t\s+\w+\[4\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)
    # the comment states the rules and the cost
    full = open(os.path.join(ROOT, "include", "tsdf_hip.h")).read()
    assert "one add at a time in ascending input index" in full and "ONE lane walks each cluster" in full
    # no test hook came with it
    assert "decimate" not in _header("tsdf_hip_test.h").lower()


def test_both_libraries_export_them():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"
    # the product library's export table still equals the header
    declared = set(re.findall(r"\b(tsdf_hip_\w+)\s*\(", _header()))
    assert _exported(capi.PRODUCT_LIB_PATH) == declared


def test_ctypes_table_and_python_classes_carry_them():
    for name, n_args in zip(ENTRY_POINTS, (14, 4, 1)):
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in cpu_tsdf_amd/capi.py"
        assert len(capi.SIGNATURES[name][1]) == n_args
    sig = inspect.signature(MarchingCubesTSDFOctree.setDecimate)
    assert list(sig.parameters) == ["self", "cell_size"]
    assert callable(getattr(MarchingCubesTSDFOctree, "clearDecimate", None))
    sig = inspect.signature(volume.decimate_mesh)
    assert list(sig.parameters) == ["vertices", "polygons", "colors", "cell_size", "device"]
    assert sig.parameters["polygons"].default is None and sig.parameters["colors"].default is None and sig.parameters["device"].default == 0
    mc = MarchingCubesTSDFOctree()
    assert mc._decimate is None
    mc.setDecimate(0.25)
    assert mc._decimate == 0.25
    mc.clearDecimate()
    assert mc._decimate is None
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        try:
            mc.setDecimate(bad)
        except ValueError:
            continue
        raise AssertionError(f"setDecimate({bad}) was accepted")


def test_cpp_class_declares_the_setters_and_the_programs_use_the_auto_pass():
    txt = open(os.path.join(ROOT, "include", "cpu_tsdf", "marching_cubes_tsdf_octree.h")).read()
    assert re.search(r"void\s+setDecimate\s*\(\s*float\s+cell_size\s*\)", txt)
    assert re.search(r"void\s+clearDecimate\s*\(\s*\)", txt)
    assert "flatten is SKIPPED" in txt
    post = open(os.path.join(ROOT, "cpu_tsdf_amd", "csrc", "prog", "mesh_post.h")).read()
    assert re.search(r"inline\s+int\s+decimateMesh\s*\(\s*pcl::PolygonMesh\s*&\s*mesh\s*,\s*float\s+cell_size", post)
    assert re.search(r"inline\s+int\s+decimateMeshGpu\s*\(\s*pcl::PolygonMesh\s*&\s*mesh\s*,\s*float\s+cell_size\s*,\s*int\s+device\s*=\s*0\s*\)", post)
    assert re.search(r"inline\s+int\s+decimateMeshAuto\s*\(", post) and "kDecimateHostBelowVertices" in post
    for prog in ("integrate.cpp", "tsdf2mesh.cpp"):
        src = open(os.path.join(ROOT, "cpu_tsdf_amd", "csrc", "prog", prog)).read()
        assert "decimateMeshAuto(mesh" in src and "decimate" in src


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_refusals_that_need_no_device_and_the_empty_mesh():
    lib = capi.load()
    m, k = C.c_uint64(7), C.c_uint64(7)
    assert lib.tsdf_hip_march_decimate(None, 0.1, C.byref(m), C.byref(k)) == capi.E_INVALID
    assert lib.tsdf_hip_mesh_decimate_stats(None) == capi.E_INVALID
    verts = np.zeros((6, 3), np.float32)
    rgb = np.zeros((6, 3), np.uint8)
    remap, counts = np.zeros(6, np.uint32), np.zeros(6, np.uint32)
    out_v, out_c = np.zeros((6, 3), np.float32), np.zeros((6, 3), np.uint8)
    faces = np.zeros((2, 3), np.uint32)
    vp, cp, rp, np_, fp = capi.as_f32p(verts), capi.as_u8p(rgb), remap.ctypes.data_as(U32P), counts.ctypes.data_as(U32P), faces.ctypes.data_as(U32P)
    ovp, ocp = capi.as_f32p(out_v), capi.as_u8p(out_c)

    def call(v=vp, c=cp, nv=6, f=None, nf=2, cell=0.1, device=0, oc=ocp, nov=C.byref(m), nof=C.byref(k)):
        return lib.tsdf_hip_mesh_decimate(device, v, c, nv, f, nf, cell, rp, ovp, oc, np_, nov, fp, nof)

    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert call(cell=bad) == capi.E_INVALID, bad
    assert call(device=-1) == capi.E_INVALID
    assert call(v=None) == capi.E_INVALID
    assert call(c=None) == capi.E_INVALID            # colours out are asked for: colours in have to come from somewhere
    assert call(nov=None) == capi.E_INVALID          # vertices out are asked for: the count has to go somewhere
    assert call(nof=None) == capi.E_INVALID
    assert call(nv=5) == capi.E_INVALID              # a soup of 2 faces needs 6 vertices
    assert call(nv=(1 << 31) + 1) == capi.E_INVALID  # indices are 32-bit
    assert call(f=fp, nf=(1 << 31) + 1) == capi.E_INVALID
    assert call(nv=0, f=fp, nf=2) == capi.E_INVALID  # every face names a vertex >= n_verts
    assert m.value == 0 and k.value == 0
    assert "tsdf_hip_mesh_decimate" in capi.load().tsdf_hip_last_error().decode()
    # no vertex: nothing to do, and no device needed
    m.value = k.value = 7
    assert call(v=None, c=None, oc=None, nv=0, nf=0) == capi.OK and m.value == 0 and k.value == 0
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.tsdf_hip_mesh_decimate_stats(out) == capi.OK and list(out) == [0, 0, 0, 0]


def test_cpp_class_keeps_the_size_it_had(tmp_path):
    """As tests/test_flatten_abi.py checks for setFlatten: setDecimate's argument lives in the shell library, not in the
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
  mc.setDecimate(0.5f);
  mc.setDecimate(0.25f);
  mc.clearDecimate();
  return 0;
}
""")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [str(src), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                                                                            "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    subprocess.run([exe], check=True, timeout=60)
