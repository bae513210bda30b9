"""GPU tier: meshNormals above the C ABI.  `tsdf2mesh in.vol out.ply --normals`, alone and after --decimate and --smooth, must
write the same file whichever pass runs, and its nx ny nz must be the model (tests/normals_cases.py) on the file's own
vertices and faces; the two passes of csrc/prog/mesh_post.h must write the same blob; and cpu_tsdf::MarchingCubesTSDFOctree
with setNormals, through tests/harness/meshnormals.cpp on a volume the Python binding saved, must return the Python path's
mesh with those normals appended."""
import os
import struct
import subprocess

import numpy as np
import pytest

from cpu_tsdf_amd import synth
from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree
from tests import normals_cases as nc
from tests import sequence_util as su
from tests.common import frames, make_volume
from tests.test_normals_gpu import VOXEL, H, W
from tests.test_normals_oracle import build_harness, write_mesh

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
RES = 64  # (the .vol format needs a cubic power-of-two grid)


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshnormals"))


@pytest.fixture(scope="module")
def saved_volume(gpu, tmp_path_factory):
    vol, scene = make_volume(RES, W, H, color=True)
    vol.reset()
    for _, tr, dep, col in frames(scene, 6, 8):
        vol.integrateCloud(dep, col, tr)
    vol.setGlobalTransform(synth.turntable_pose(2, 8, RES * VOXEL))
    path = str(tmp_path_factory.mktemp("normalsvol") / "fused.vol")
    vol.save(path)
    yield vol, path
    vol.close()


def read_mesh(raw, at):
    """one mesh of the harness: (fields {name: offset}, blob rows (n, point_step) uint8, polygons (k, 3)), next offset"""
    step, blob_bytes, n_poly, n_fields = struct.unpack_from("<4q", raw, at)
    at += 32
    fields = {}
    for _ in range(n_fields):
        name = raw[at:at + 16].split(b"\0")[0].decode()
        fields[name], = struct.unpack_from("<q", raw, at + 16)
        at += 24
    rows = np.frombuffer(raw, np.uint8, blob_bytes, at).reshape(-1, step) if blob_bytes else np.empty((0, step), np.uint8)
    at += blob_bytes
    polys = []
    for _ in range(n_poly):
        k, = struct.unpack_from("<q", raw, at)
        polys.append(struct.unpack_from(f"<{k}I", raw, at + 8))
        at += 8 + 4 * k
    return (fields, rows, np.asarray(polys, np.int64).reshape(-1, 3)), at


def words(rows, offset, count=3):
    return rows[:, offset:offset + 4 * count].copy().view(U32).reshape(-1, count)


def read_ply(path):
    """a binary PLY of the programs: (vertices, normals or None, faces)"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().splitlines()
    assert "binary_little_endian" in header[1]
    nv = int([ln for ln in header if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in header if ln.startswith("element face")][0].split()[-1])
    props = [ln.split()[-1] for ln in header if ln.startswith("property float") or ln.startswith("property uchar")]
    assert props in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"]), props
    vdt = [(p, "<f4") for p in props]
    v = np.frombuffer(data, vdt, nv, end)
    fc = np.frombuffer(data, [("n", "u1"), ("i", "<i4", 3)], nf, end + nv * np.dtype(vdt).itemsize)
    assert end + v.nbytes + fc.nbytes == len(data) and (fc["n"] == 3).all()
    normals = np.stack([v["nx"], v["ny"], v["nz"]], 1) if "nx" in props else None
    return np.stack([v["x"], v["y"], v["z"]], 1), normals, fc["i"].copy()


def is_soup(verts, faces):
    return len(verts) == 3 * len(faces) and np.array_equal(np.asarray(faces).ravel(), np.arange(len(verts)))


@pytest.mark.parametrize("extra", [[], ["--decimate", repr(2 * VOXEL), "--smooth", "3"]], ids=["soup", "decimate_smooth"])
def test_tsdf2mesh_with_normals(saved_volume, tmp_path, extra):
    _, vol = saved_volume
    if not os.path.exists(su.OUR_TSDF2MESH):
        from cpu_tsdf_amd import build as b
        b.build_programs()
    outs = {}
    for tag, more, env in (("plain", [], {}), ("auto", ["--normals"], {}), ("host", ["--normals"], {"TSDF_HIP_HOST_MESH_POST": "1"})):
        outs[tag] = str(tmp_path / f"{tag}.ply")
        full = dict(os.environ)
        full.update(env)
        out = subprocess.run([su.OUR_TSDF2MESH, vol, outs[tag]] + extra + more, capture_output=True, text=True, timeout=300, env=full)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert open(outs["auto"], "rb").read() == open(outs["host"], "rb").read(), "meshNormalsAuto and the host pass wrote different files"
    v0, n0, f0 = read_ply(outs["plain"])
    v, n, f = read_ply(outs["auto"])
    assert n0 is None and n is not None and len(f) > 200
    assert np.array_equal(v.view(U32), v0.view(U32)) and np.array_equal(f, f0), "--normals changed the mesh itself"
    assert is_soup(v, f) == (not extra)
    want = nc.Model(v, None if is_soup(v, f) else f)
    assert np.array_equal(n.view(U32), want.normals.view(U32)), "nx ny nz differ from the model on the file's own mesh"
    assert want.n_zero < len(v) // 10


def test_gpu_backed_pass_equals_the_host_pass_byte_for_byte(harness, tmp_path):
    """meshNormals and meshNormalsGpu on copies of one PolygonMesh, whatever meshNormalsAuto would choose: an indexed mesh with
    colours, and a soup"""
    rgb = np.random.default_rng(3).integers(0, 256, (2000, 3)).astype(np.uint8)
    for name, colours in (("random", rgb), ("random_soup_257", None), ("icosphere_5", None)):
        verts, faces, _ = nc.arrays(name)
        want = nc.model(name)
        src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
        write_mesh(src, verts, faces, rgb=colours)
        subprocess.run([harness, "mesh", src, out], check=True, timeout=120)
        raw = open(out, "rb").read()
        host, at = read_mesh(raw, 0)
        gpu_mesh, at = read_mesh(raw, at)
        assert at == len(raw)
        assert host[0] == gpu_mesh[0] and host[1].tobytes() == gpu_mesh[1].tobytes(), "the point cloud blobs differ"
        assert np.array_equal(host[2], gpu_mesh[2])
        fields, rows, polys = host
        step = 32 if colours is not None else 16
        assert list(fields)[-3:] == ["normal_x", "normal_y", "normal_z"] and [fields[k] for k in list(fields)[-3:]] == [step, step + 4, step + 8]
        assert rows.shape[1] == step + 12
        assert np.array_equal(words(rows, fields["normal_x"]), want.normals.view(U32))
        assert np.array_equal(words(rows, 0), verts.view(U32)), "the positions changed"
        assert np.array_equal(polys, np.arange(len(verts)).reshape(-1, 3) if faces is None else faces), "the polygons changed"
        if colours is not None:
            assert np.array_equal(rows[:, 16:19][:, ::-1], colours), "the colours did not survive"


def reconstruct(vol, decimate, smooth, normals, transform=True):
    g = vol.getGlobalTransform()
    if not transform:
        vol.setGlobalTransform(np.eye(4))
    mc = MarchingCubesTSDFOctree()
    mc.setInputTSDF(vol)
    mc.setMinWeight(1.0)
    mc.setColorByRGB(True)
    if decimate:
        mc.setDecimate(decimate)
    if smooth:
        mc.setSmooth(smooth)
    mc.setNormals(normals)
    try:
        return mc.reconstruct()
    finally:
        vol.setGlobalTransform(g)


@pytest.mark.parametrize("decimate,smooth", [(0.0, 0), (2 * VOXEL, 3)], ids=["soup", "decimate_smooth"])
def test_cpp_class_with_set_normals_equals_the_python_path_and_the_model(harness, saved_volume, tmp_path, decimate, smooth):
    vol, path = saved_volume
    g = vol.getGlobalTransform()
    assert not np.array_equal(g, np.eye(4))
    want = reconstruct(vol, decimate, smooth, True)
    before = reconstruct(vol, decimate, smooth, False, transform=False)  # the mesh in the volume frame
    soup = is_soup(before["vertices"], before["polygons"])
    assert soup == (not decimate) and len(before["polygons"]) > 200
    model = nc.Model(before["vertices"], None if soup else before["polygons"])
    # the normals are those of the mesh in the volume frame, turned by the global transform's rotation like the vertices
    r, n64 = g[:3, :3].astype(np.float64), model.normals.astype(np.float64)
    turned = (n64[:, 0:1] * r[:, 0] + (n64[:, 1:2] * r[:, 1] + n64[:, 2:3] * r[:, 2])).astype(F32)
    assert np.array_equal(want["normals"].view(U32), turned.view(U32))
    at_home = reconstruct(vol, decimate, smooth, True, transform=False)
    assert np.array_equal(at_home["normals"].view(U32), model.normals.view(U32))  # identity: word for word
    out = str(tmp_path / "out.bin")
    subprocess.run([harness, "volume", path, out, "1.0", "1", "0", repr(float(decimate)), str(smooth)], check=True, timeout=120)
    raw = open(out, "rb").read()
    (fields, rows, polys), at = read_mesh(raw, 0)
    assert at == len(raw)
    assert list(fields) == ["x", "y", "z", "rgb", "normal_x", "normal_y", "normal_z"] and rows.shape[1] == 44
    assert [fields[k] for k in ("normal_x", "normal_y", "normal_z")] == [32, 36, 40]
    assert np.array_equal(words(rows, 0), want["vertices"].view(U32)), "the C++ class' vertices differ from the Python path's"
    assert np.array_equal(polys, want["polygons"])
    assert np.array_equal(rows[:, 16:19][:, ::-1], want["rgb"]), "the colours changed"
    assert np.array_equal(words(rows, 32), want["normals"].view(U32)), "the C++ class' normals differ from the Python path's"
