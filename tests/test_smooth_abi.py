"""CPU tier: the boundary of smoothMesh on the GPU -- include/tsdf_hip.h declares the three entry points, both builds of the
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
ENTRY_POINTS = ["tsdf_hip_mesh_smooth", "tsdf_hip_march_smooth", "tsdf_hip_mesh_smooth_stats"]
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
    assert re.search(r"\bint\s+tsdf_hip_mesh_smooth\s*\(\s*int" + w + r",\s*const\s+float" + s + r",\s*uint64_t" + w + r",\s*const\s+uint32_t" + s +
                     r",\s*uint64_t" + w + r",\s*float" + w + r",\s*float" + w + r",\s*int" + w + r",\s*int" + w + r",\s*float" + s + r",\s*uint8_t" + s +
                     r",\s*uint32_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_march_smooth\s*\(\s*tsdf_handle" + w + r",\s*float" + w + r",\s*float" + w + r",\s*int" + w + r",\s*int" + w +
                     r",\s*uint64_t" + s + r"\)", txt)
    assert re.search(r"\bint\s+tsdf_hip_mesh_smooth_stats\s*\(\s*uint64_t\s+\w+\[4\]\s*\)", txt)
    assert re.search(r"#define\s+TSDF_HIP_ABI_VERSION\s+14\b", txt)
    # the comment states the rule, the refusals and the cost
    full = " ".join(open(os.path.join(ROOT, "include", "tsdf_hip.h")).read().replace("\n * ", " ").split())
    for words in ("x'_i = (float)(p + f * (m - p))", "one add at a time over N(i) in ascending index", "flatten or decimate first",
                  "ONE lane walks each vertex's neighbour list so that the adds keep the host's order", "A marched mesh has degree 4-8",
                  "a vertex with thousands of neighbours makes one lane walk them all, twice per iteration", "iterations outside [0, 1000]"):
        assert words in full, words
    # no test hook came with it
    assert "smooth" not in _header("tsdf_hip_test.h").lower()


def test_both_libraries_export_them():
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        have = _exported(path)
        for name in ENTRY_POINTS:
            assert name in have, f"{name} is not exported by {os.path.basename(path)}"
    declared = set(re.findall(r"\b(tsdf_hip_\w+)\s*\(", _header()))
    assert _exported(capi.PRODUCT_LIB_PATH) == declared


def test_ctypes_table_and_python_classes_carry_them():
    for name, n_args in zip(ENTRY_POINTS, (12, 6, 1)):
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in cpu_tsdf_amd/capi.py"
        assert len(capi.SIGNATURES[name][1]) == n_args
    args = capi.SIGNATURES["tsdf_hip_mesh_smooth"][1]
    assert args[5] is C.c_float and args[6] is C.c_float and args[7] is C.c_int and args[8] is C.c_int
    sig = inspect.signature(MarchingCubesTSDFOctree.setSmooth)
    assert list(sig.parameters) == ["self", "iterations", "lam", "mu", "keep_boundary"]
    assert [sig.parameters[k].default for k in ("lam", "mu", "keep_boundary")] == [0.5, -0.53, True]
    assert callable(getattr(MarchingCubesTSDFOctree, "clearSmooth", None))
    sig = inspect.signature(volume.smooth_mesh)
    assert list(sig.parameters) == ["vertices", "polygons", "lam", "mu", "iterations", "keep_boundary", "device"]
    assert [sig.parameters[k].default for k in ("lam", "mu", "iterations", "keep_boundary", "device")] == [0.5, -0.53, 10, True, 0]
    mc = MarchingCubesTSDFOctree()
    assert mc._smooth is None
    mc.setSmooth(3)
    assert mc._smooth == (3, 0.5, -0.53, True)
    mc.setSmooth(0, 1.0, -1.0, False)
    assert mc._smooth == (0, 1.0, -1.0, False)
    mc.clearSmooth()
    assert mc._smooth is None
    for bad in ((-1,), (1001,), (3, 0.0), (3, 1.5), (3, float("nan")), (3, 0.5, 0.1), (3, 0.5, -1.5), (3, 0.5, float("inf"))):
        try:
            mc.setSmooth(*bad)
        except ValueError:
            continue
        raise AssertionError(f"setSmooth{bad} was accepted")
    try:
        volume.smooth_mesh(np.zeros((3, 3), np.float32), None)
    except ValueError as e:
        assert "flatten or decimate first" in str(e)
    else:
        raise AssertionError("smooth_mesh accepted a soup")


def test_cpp_class_declares_the_setters_and_the_host_pass_is_there():
    txt = open(os.path.join(ROOT, "include", "cpu_tsdf", "marching_cubes_tsdf_octree.h")).read()
    assert re.search(r"void\s+setSmooth\s*\(\s*int\s+iterations\s*,\s*float\s+lambda\s*=\s*0\.5f\s*,\s*float\s+mu\s*=\s*-0\.53f\s*,\s*bool\s+keep_boundary\s*=\s*true\s*\)", txt)
    assert re.search(r"void\s+clearSmooth\s*\(\s*\)", txt)
    post = open(os.path.join(ROOT, "cpu_tsdf_amd", "csrc", "prog", "mesh_post.h")).read()
    assert re.search(r"inline\s+int\s+smoothArrays\s*\(\s*const\s+float\s*\*\s*xyz", post)
    assert re.search(r"inline\s+int\s+smoothMesh\s*\(\s*pcl::PolygonMesh\s*&\s*mesh", post)
    assert re.search(r"inline\s+int\s+smoothMeshGpu\s*\(\s*pcl::PolygonMesh\s*&\s*mesh", post)
    assert re.search(r"inline\s+int\s+smoothMeshAuto\s*\(", post) and "kSmoothHostBelowVertices" in post and "TSDF_HIP_HOST_MESH_POST" in post


def test_abi_version_is_still_14():
    lib = capi.load()
    assert lib.tsdf_hip_abi_version() == 14
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_refusals_that_need_no_device_and_the_empty_mesh():
    lib = capi.load()
    nf = C.c_uint64(7)
    assert lib.tsdf_hip_march_smooth(None, 0.5, -0.53, 3, 1, C.byref(nf)) == capi.E_INVALID
    assert lib.tsdf_hip_mesh_smooth_stats(None) == capi.E_INVALID
    verts = np.arange(18, dtype=np.float32).reshape(6, 3)
    out = np.full((6, 3), 7, np.float32)
    fixed, degree = np.full(6, 9, np.uint8), np.full(6, 9, np.uint32)
    faces = np.asarray([[0, 1, 2], [3, 4, 5]], np.uint32)
    vp, op, fp = capi.as_f32p(verts), capi.as_f32p(out), faces.ctypes.data_as(U32P)

    def call(v=vp, nv=6, f=fp, nf=2, lam=0.5, mu=-0.53, it=3, keep=1, o=op, device=0):
        return lib.tsdf_hip_mesh_smooth(device, v, nv, f, nf, lam, mu, it, keep, o, capi.as_u8p(fixed), degree.ctypes.data_as(U32P))

    def refused(what, **kw):
        assert call(**kw) == capi.E_INVALID, kw
        text = lib.tsdf_hip_last_error().decode()
        assert what in text, (kw, text)

    for bad in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        refused("lambda", lam=bad)
    for bad in (0.001, -1.0001, float("nan"), float("-inf")):
        refused("mu", mu=bad)
    for bad in (-1, 1001):
        refused("iterations", it=bad)
    refused("2^31", nv=(1 << 31) + 1)
    refused("2^31", nf=(1 << 31) + 1)
    refused("NULL", v=None)
    refused("NULL", o=None)
    refused("flatten or decimate first", f=None)
    assert call(device=-1) == capi.E_INVALID
    refused(">= n_verts", nv=0)  # every face names a vertex >= n_verts
    assert (out == 7).all() and (fixed == 9).all() and (degree == 9).all()  # nothing was written
    # no vertex: nothing to do, and no device needed
    assert call(v=None, o=None, f=None, nv=0, nf=0) == capi.OK
    st = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.tsdf_hip_mesh_smooth_stats(st) == capi.OK and list(st) == [0, 0, 0, 0]


def test_cpp_class_keeps_the_size_it_had(tmp_path):
    """As tests/test_decimate_abi.py checks for setDecimate: setSmooth's arguments live in the shell library, not in the
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
  mc.setSmooth(10);
  mc.setSmooth(3, 0.6f, -0.61f, false);
  mc.clearSmooth();
  return 0;
}
""")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [str(src), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                                                                            "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    subprocess.run([exe], check=True, timeout=60)
