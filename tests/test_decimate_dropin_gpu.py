"""GPU tier: decimateMesh above the C ABI.  cpu_tsdf::MarchingCubesTSDFOctree with setDecimate, through
tests/harness/meshdec.cpp on a volume the Python binding saved, must return the Python path's mesh byte for byte (which
tests/test_decimate_gpu.py pins to the model); and the `integrate` program with --decimate must write the model applied to the
mesh it writes without the option, whichever of the two passes of csrc/prog/mesh_post.h runs, and the unchanged mesh without
it.  tsdf2mesh likewise."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree
from tests import decimate_cases as dc
from tests import sequence_util as su
from tests.test_decimate_oracle import build_harness
from tests.test_flatten_oracle import read_mesh
from tests.test_meshpost_gpu import RES, V_FD, fused_volume
from tests.test_programs import COMMON, H, SIZE, W
from tests.test_programs import RES as PROG_RES

pytestmark = pytest.mark.gpu
VOXEL = 0.25 / RES


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshdec"))


@pytest.fixture(scope="module")
def saved_volume(gpu, tmp_path_factory):
    vol = fused_volume()
    path = str(tmp_path_factory.mktemp("decvol") / "fused.vol")
    vol.save(path)
    yield vol, path
    vol.close()


@pytest.mark.parametrize("cleanup,flatten", [(None, 0.0), ((V_FD, 40), 0.0), (None, 1e-4)], ids=["plain", "cleanup", "flatten_skipped"])
def test_cpp_class_with_set_decimate_equals_the_python_path(harness, saved_volume, tmp_path, cleanup, flatten):
    vol, path = saved_volume
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if cleanup:
        mc.setCleanup(*cleanup)
    mc.setDecimate(2 * VOXEL)
    want = mc.reconstruct()
    assert 2 <= len(want["vertices"]) and 1 <= len(want["polygons"])
    out = str(tmp_path / "out.bin")
    fd, mn = cleanup if cleanup else (0.0, -1)
    subprocess.run([harness, "volume", path, out, repr(2 * VOXEL), "1.0", "1", repr(float(fd)), str(mn), repr(float(flatten))], check=True, timeout=120)
    raw = open(out, "rb").read()
    (xyz, polys, step, blob), at = read_mesh(raw, 0)
    assert at == len(raw)
    assert np.array_equal(xyz, want["vertices"].view(np.uint32)), "the C++ class' vertices differ from the Python path's"
    assert np.array_equal(polys, want["polygons"]), "the C++ class' polygons differ from the Python path's"
    bgr = np.frombuffer(blob, np.uint8).reshape(-1, step)[:, 16:19]
    assert np.array_equal(bgr[:, ::-1], want["rgb"]), "the C++ class' colours differ from the Python path's"


def test_gpu_backed_pass_equals_the_host_pass_byte_for_byte(harness, tmp_path):
    """decimateMesh and decimateMeshGpu on copies of one coloured PolygonMesh, whatever decimateMeshAuto would choose."""
    from tests.test_decimate_oracle import write_mesh
    verts, faces, rgb, cell, _ = dc.cases()["snapped_indexed"]
    want = dc.model("snapped_indexed")
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, verts, faces, rgb)
    subprocess.run([harness, "mesh", src, out, repr(float(np.float32(cell)))], check=True, timeout=120)
    raw = open(out, "rb").read()
    host, at = read_mesh(raw, 0)
    gpu_mesh, at = read_mesh(raw, at)
    assert at == len(raw)
    assert host[2] == gpu_mesh[2] and host[3] == gpu_mesh[3], "the point cloud blobs differ"
    assert np.array_equal(host[1], gpu_mesh[1]), "the polygons differ"
    assert np.array_equal(host[0], want.vertices.view(np.uint32)) and np.array_equal(host[1], want.polygons)
    bgr = np.frombuffer(host[3], np.uint8).reshape(-1, host[2])[:, 16:19]
    assert np.array_equal(bgr[:, ::-1], want.rgb)


@pytest.fixture(scope="module")
def sequence(gpu):
    if not os.path.exists(su.OUR_INTEGRATE):
        from cpu_tsdf_amd import build as b
        b.build_programs()
    d = su.digit_free_dir("decimate")
    su.make_sequence(os.path.join(d, "in"), n_frames=4, width=W, height=H)
    yield d
    shutil.rmtree(d, ignore_errors=True)


def run_integrate(d, tag, extra, env=None):
    args = ["--in", os.path.join(d, "in")] + COMMON + ["--color", "--out", os.path.join(d, tag)] + extra
    full = dict(os.environ)
    full.update(env or {})
    out = subprocess.run([su.OUR_INTEGRATE] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=full)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    return os.path.join(d, tag, "mesh.ply")


def test_integrate_program_with_decimate_writes_the_model_of_its_plain_mesh(sequence):
    d = sequence
    cell = 2 * SIZE / PROG_RES  # two voxels
    plain = run_integrate(d, "plain", [])
    again = run_integrate(d, "again", [])
    assert open(plain, "rb").read() == open(again, "rb").read()
    v, c, f = su.read_ply(plain)
    assert len(f) > 200 and c is not None
    want = dc.Dec(v, f, c, cell)
    assert len(want.counts) >= 2 and (want.counts > 1).any() and want.degenerate.any() and want.keep.any()
    gpu_pass = run_integrate(d, "auto", ["--decimate", cell])  # (decimateMeshAuto: the host pass below its crossover)
    host_pass = run_integrate(d, "host", ["--decimate", cell], env={"TSDF_HIP_HOST_MESH_POST": "1"})
    assert open(gpu_pass, "rb").read() == open(host_pass, "rb").read(), "decimateMeshAuto and the host pass wrote different files"
    v2, c2, f2 = su.read_ply(gpu_pass)
    assert np.array_equal(v2.view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(c2, want.rgb)
    assert np.array_equal(f2, want.polygons)
    assert len(v2) < len(v) and len(f2) < len(f)
    # a cell size the program must refuse
    args = ["--in", os.path.join(d, "in")] + COMMON + ["--out", os.path.join(d, "bad"), "--decimate", 0.0]
    rc, log = su.run(su.OUR_INTEGRATE, args)
    assert rc == 1 and "--decimate" in log


def test_tsdf2mesh_with_decimate(sequence):
    d = sequence
    args = ["--in", os.path.join(d, "in")] + COMMON + ["--color", "--save-tsdf", "--out", os.path.join(d, "vol")]
    rc, log = su.run(su.OUR_INTEGRATE, args)
    assert rc == 0, log[-2000:]
    cell = 2 * SIZE / PROG_RES
    plain, dec = os.path.join(d, "t_plain.ply"), os.path.join(d, "t_dec.ply")
    for out, extra in ((plain, []), (dec, ["--decimate", cell])):
        rc, log = su.run(su.OUR_TSDF2MESH, [os.path.join(d, "vol", "volume.tsdf"), out] + extra)
        assert rc == 0, log[-2000:]
    v, c, f = su.read_ply(plain)
    assert len(f) > 200 and c is None
    want = dc.Dec(v, f, None, cell)
    assert len(want.counts) >= 2 and (want.counts > 1).any() and want.degenerate.any() and want.keep.any()
    v2, c2, f2 = su.read_ply(dec)
    assert c2 is None
    assert np.array_equal(v2.view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(f2, want.polygons)
