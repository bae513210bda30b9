"""GPU tier: smoothMesh above the C ABI.  cpu_tsdf::MarchingCubesTSDFOctree with setSmooth, through
tests/harness/meshsmooth.cpp on a volume the Python binding saved, must return the Python path's mesh and the model's
(tests/smooth_cases.py) after the global transform; the two passes of csrc/prog/mesh_post.h must write the same blob; and the
`integrate` and `tsdf2mesh` programs with --smooth must write the model applied to the mesh they write without the option,
whichever pass runs, and the unchanged mesh without it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cpu_tsdf_amd import synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, flatten_mesh, transform_points_f64
from tests import sequence_util as su
from tests import smooth_cases as sc
from tests.test_flatten_oracle import read_mesh
from tests.test_programs import COMMON, H, W
from tests.test_smooth_gpu import ARGS, VOXEL, fused_volume
from tests.test_smooth_oracle import args, build_harness, write_mesh

pytestmark = pytest.mark.gpu
U32 = np.uint32
RES = 64  # (the .vol format needs a cubic power-of-two grid)


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshsmooth"))


@pytest.fixture(scope="module")
def saved_volume(gpu, tmp_path_factory):
    vol = fused_volume(res=RES)
    vol.setGlobalTransform(synth.turntable_pose(2, 8, RES * VOXEL))
    path = str(tmp_path_factory.mktemp("smoothvol") / "fused.vol")
    vol.save(path)
    yield vol, path
    vol.close()


def reconstruct(vol, decimate, smooth, transform=True):
    g = vol.getGlobalTransform()
    if not transform:
        vol.setGlobalTransform(np.eye(4))
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if decimate:
        mc.setDecimate(decimate)
    else:
        mc.setFlatten()
    if smooth:
        mc.setSmooth(ARGS[2], ARGS[0], ARGS[1], bool(ARGS[3]))
    try:
        return mc.reconstruct()
    finally:
        vol.setGlobalTransform(g)


@pytest.mark.parametrize("decimate", [0.0, 2 * VOXEL], ids=["flatten_by_default", "decimate"])
def test_cpp_class_with_set_smooth_equals_the_python_path_and_the_model(harness, saved_volume, tmp_path, decimate):
    vol, path = saved_volume
    assert not np.array_equal(vol.getGlobalTransform(), np.eye(4))
    want = reconstruct(vol, decimate, True)
    before = reconstruct(vol, decimate, False, transform=False)  # the indexed mesh in the volume frame
    model = sc.Model(before["vertices"], before["polygons"], *ARGS)
    assert 0 < model.n_fixed < len(model.fixed)
    assert np.array_equal(want["vertices"].view(U32), transform_points_f64(model.vertices, vol.getGlobalTransform()).view(U32))
    out = str(tmp_path / "out.bin")
    subprocess.run([harness, "volume", path, out] + args(*ARGS) + ["1.0", "1", repr(float(decimate))], check=True, timeout=120)
    raw = open(out, "rb").read()
    (xyz, polys, step, blob), at = read_mesh(raw, 0)
    assert at == len(raw)
    assert np.array_equal(xyz, want["vertices"].view(U32)), "the C++ class' vertices differ from the Python path's"
    assert np.array_equal(polys, want["polygons"]) and np.array_equal(polys, before["polygons"]), "the polygons changed"
    bgr = np.frombuffer(blob, np.uint8).reshape(-1, step)[:, 16:19]
    assert np.array_equal(bgr[:, ::-1], want["rgb"]) and np.array_equal(want["rgb"], before["rgb"]), "the colours changed"


def test_gpu_backed_pass_equals_the_host_pass_byte_for_byte(harness, tmp_path):
    """smoothMesh and smoothMeshGpu on copies of one coloured PolygonMesh, whatever smoothMeshAuto would choose: only the
    x, y, z fields of the blob change."""
    verts, faces, lam, mu, it, kb = sc.cases()["random"]
    want = sc.model("random")
    rgb = np.random.default_rng(3).integers(0, 256, (len(verts), 3)).astype(np.uint8)
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, verts, faces, rgb)
    subprocess.run([harness, "mesh", src, out] + args(lam, mu, it, kb), check=True, timeout=120)
    raw = open(out, "rb").read()
    host, at = read_mesh(raw, 0)
    gpu_mesh, at = read_mesh(raw, at)
    assert at == len(raw)
    assert host[2] == gpu_mesh[2] and host[3] == gpu_mesh[3], "the point cloud blobs differ"
    assert np.array_equal(host[1], gpu_mesh[1]) and np.array_equal(host[1], faces), "the polygons changed"
    assert np.array_equal(host[0], want.vertices.view(U32))
    bgr = np.frombuffer(host[3], np.uint8).reshape(-1, host[2])[:, 16:19]
    assert np.array_equal(bgr[:, ::-1], rgb), "the colours did not survive"


@pytest.fixture(scope="module")
def sequence(gpu):
    if not os.path.exists(su.OUR_INTEGRATE):
        from cpu_tsdf_amd import build as b
        b.build_programs()
    d = su.digit_free_dir("smooth")
    su.make_sequence(os.path.join(d, "in"), n_frames=4, width=W, height=H)
    yield d
    shutil.rmtree(d, ignore_errors=True)


def run_integrate(d, tag, extra, env=None):
    full = dict(os.environ)
    full.update(env or {})
    cmd = ["--in", os.path.join(d, "in")] + COMMON + ["--color", "--out", os.path.join(d, tag)] + extra
    out = subprocess.run([su.OUR_INTEGRATE] + [str(a) for a in cmd], capture_output=True, text=True, timeout=300, env=full)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    return os.path.join(d, tag, "mesh.ply")


def same_colours(a, b):
    return (a is None and b is None) or np.array_equal(a, b)


def test_integrate_program_with_smooth_writes_the_model_of_its_flattened_mesh(sequence):
    d = sequence
    plain = run_integrate(d, "plain", ["--flatten"])
    again = run_integrate(d, "again", ["--flatten"])
    assert open(plain, "rb").read() == open(again, "rb").read()  # without the option: the bytes it always wrote
    v, c, f = su.read_ply(plain)
    assert len(f) > 200
    want = sc.Model(v, f, 0.5, -0.53, 3, 1)
    assert 0 < want.n_fixed < len(v)
    auto_pass = run_integrate(d, "auto", ["--flatten", "--smooth", 3])
    host_pass = run_integrate(d, "host", ["--flatten", "--smooth", 3], env={"TSDF_HIP_HOST_MESH_POST": "1"})
    assert open(auto_pass, "rb").read() == open(host_pass, "rb").read(), "smoothMeshAuto and the host pass wrote different files"
    v2, c2, f2 = su.read_ply(auto_pass)
    assert np.array_equal(v2.view(U32), want.vertices.view(U32))
    assert np.array_equal(f2, f) and same_colours(c2, c)
    # other factors; and still a soup: flattened first, at the default distance
    other = run_integrate(d, "other", ["--smooth", 2, "--smooth-lambda", 0.6, "--smooth-mu", -0.4])
    v3, c3, f3 = su.read_ply(other)
    assert np.array_equal(f3, f) and np.array_equal(v3.view(U32), sc.Model(v, f, 0.6, -0.4, 2, 1).vertices.view(U32))
    # arguments the program must refuse
    for extra in (["--smooth", 3, "--smooth-lambda", 0.0], ["--smooth", 1001], ["--smooth", 3, "--smooth-mu", 0.5]):
        rc, log = su.run(su.OUR_INTEGRATE, ["--in", os.path.join(d, "in")] + COMMON + ["--flatten", "--out", os.path.join(d, "bad")] + extra)
        assert rc == 1 and "--smooth" in log, (extra, log[-500:])


def test_tsdf2mesh_with_smooth(sequence):
    d = sequence
    rc, log = su.run(su.OUR_INTEGRATE, ["--in", os.path.join(d, "in")] + COMMON + ["--color", "--save-tsdf", "--out", os.path.join(d, "vol")])
    assert rc == 0, log[-2000:]
    vol = os.path.join(d, "vol", "volume.tsdf")
    outs = {}
    for tag, extra, env in (("plain", [], {}), ("again", [], {}), ("smooth", ["--smooth", 3], {}), ("host", ["--smooth", 3], {"TSDF_HIP_HOST_MESH_POST": "1"})):
        outs[tag] = os.path.join(d, f"t_{tag}.ply")
        full = dict(os.environ)
        full.update(env)
        out = subprocess.run([su.OUR_TSDF2MESH, vol, outs[tag]] + [str(a) for a in extra], capture_output=True, text=True, timeout=300, env=full)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert open(outs["plain"], "rb").read() == open(outs["again"], "rb").read()
    assert open(outs["smooth"], "rb").read() == open(outs["host"], "rb").read()
    v, c, f = su.read_ply(outs["plain"])
    assert len(f) > 200 and c is None
    flat = flatten_mesh(v, f)  # the soup is flattened first, at the default distance (tests/test_flatten_gpu.py pins this pass)
    want = sc.Model(flat["vertices"], flat["polygons"], 0.5, -0.53, 3, 1)
    v2, c2, f2 = su.read_ply(outs["smooth"])
    assert c2 is None and np.array_equal(f2, flat["polygons"])
    assert np.array_equal(v2.view(U32), want.vertices.view(U32))
    rc, log = su.run(su.OUR_TSDF2MESH, [vol, os.path.join(d, "t_bad.ply"), "--smooth", -1])
    assert rc == 1 and "--smooth" in log
