"""CPU tier: the numpy model of the meshNormals tests (tests/normals_cases.py) against the host pass that defines the result --
cpu_tsdf::mesh_post::normalArrays, run through tests/harness/meshnormals.cpp, which touches no device.  Normals (as words),
flags and counts must be equal on every case the GPU tests use: this pins the model here, without a GPU.  Then what the
cases are meant to show, the two discriminators, the orientation on a marched sphere (the oracle's marching cubes, on the CPU
alone) and the PLY writer."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import normals_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
E_INVALID = 1


def build_harness(dirpath):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(dirpath / "meshnormals")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tests", "harness", "meshnormals.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip",
                           "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def write_mesh(path, verts, faces, n_faces=None, rgb=None):
    """faces None: a soup (faces == NULL) of n_faces faces (default: a third of the vertices)"""
    if n_faces is None:
        n_faces = len(verts) // 3 if faces is None else len(faces)
    with open(path, "wb") as f:
        f.write(struct.pack("<4q", len(verts), n_faces, 1 if faces is None else 0, 0 if rgb is None else 1))
        f.write(np.ascontiguousarray(verts, F32).tobytes())
        if rgb is not None:
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
        if faces is not None:
            f.write(np.ascontiguousarray(faces, U32).tobytes())


def host_pass(harness, tmp_path, verts, faces, n_faces=None):
    """-> (rc, dict) or (rc, the refusal's text, was the output left untouched)"""
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, verts, faces, n_faces)
    subprocess.run([harness, "arrays", src, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    rc, = struct.unpack_from("<q", raw, 0)
    if rc:
        return rc, raw[8:-1].decode(), raw[-1] == 1
    n, skipped, zero = struct.unpack_from("<3q", raw, 8)
    normals = np.frombuffer(raw, U32, 3 * n, 32).reshape(n, 3)
    flags = np.frombuffer(raw, np.uint8, n, 32 + normals.nbytes)
    assert 32 + normals.nbytes + n == len(raw)
    return 0, {"normals": normals, "flags": flags, "stats": [n, skipped, zero]}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshnormals"))


def assert_equals_model(got, want):
    assert np.array_equal(got["flags"], want.flags), "flags differ from the model's"
    bad = np.flatnonzero((got["normals"].view(U32) != want.normals.view(U32)).any(1))
    assert len(bad) == 0, f"{len(bad)} of {len(want.normals)} normals differ from the model's, first {bad[:8].tolist()}"


@pytest.mark.parametrize("name", sorted(nc.cases()))
def test_host_pass_equals_the_numpy_model(harness, tmp_path, name):
    want = nc.model(name)
    rc, got = host_pass(harness, tmp_path, *nc.arrays(name))
    assert rc == 0, got
    assert_equals_model(got, want)
    assert got["stats"] == want.stats


def test_refusals_of_the_host_pass(harness, tmp_path):
    v, f = nc.sc.grid_patch()
    bad = f.copy()
    bad[7, 2] = len(v)
    rc, why, untouched = host_pass(harness, tmp_path, v, bad)
    assert rc == E_INVALID and untouched and ">= n_verts" in why
    soup = nc.random_soup()[0]
    rc, why, untouched = host_pass(harness, tmp_path, soup[:-1], None, 256)  # 770 vertices: not a multiple of 3
    assert rc == E_INVALID and untouched and "multiple of 3" in why
    rc, why, untouched = host_pass(harness, tmp_path, soup, None, 256)  # 257 triangles, 256 faces
    assert rc == E_INVALID and untouched and "n_verts / 3" in why
    rc, why, untouched = host_pass(harness, tmp_path, np.empty((0, 3), F32), np.zeros((1, 3), U32))
    assert rc == E_INVALID and untouched and ">= n_verts" in why
    # an empty mesh is accepted, indexed or soup
    for faces in (nc.NO_FACES, None):
        rc, got = host_pass(harness, tmp_path, np.empty((0, 3), F32), faces)
        assert rc == 0 and got["normals"].shape == (0, 3) and got["stats"] == [0, 0, 0]


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_the_cases_say_what_they_are_meant_to():
    """What the GPU tests rely on, derived from the model alone."""
    # the tetrahedron: every vertex in three faces; its faces wind clockwise seen from outside, so the normals point INWARDS
    m = nc.model("tetrahedron")
    v = nc.cases()["tetrahedron"][0].astype(np.float64)
    assert (m.valence == 3).all() and not m.flags.any() and ((m.normals.astype(np.float64) * unit(v - v.mean(0))).sum(1) < -0.9).all()
    assert np.allclose(np.linalg.norm(m.normals.astype(np.float64), axis=1), 1.0, atol=1e-6)
    m = nc.model("grid_5x5")
    assert len(m.normals) == 25 and not m.flags.any() and (m.normals[:, 2] < -0.7).all() and m.valence.max() == 6 and m.valence.min() == 1
    # the fans: one lane walks 300 / 600 entries
    m = nc.model("fan_300")
    assert m.valence[0] == 300 and (m.valence[1:] == 2).all() and not m.flags.any()
    m = nc.model("double_fan_300")
    assert m.valence[0] == m.valence[1] == 300 and (m.valence[2:] == 4).all() and not m.flags.any()
    # block edges: 255 / 256 / 257 vertices and 255 / 256 / 257 faces
    assert [len(nc.cases()[f"strip_{n}"][0]) for n in (255, 256, 257)] == [255, 256, 257]
    assert [len(nc.cases()[f"strip_{n}"][1]) for n in (257, 258, 259)] == [255, 256, 257]
    for n in (255, 256, 257, 258, 259):
        assert not nc.model(f"strip_{n}").flags.any()
    # vertices in no face: first, in the middle, last -- flags 1 | 2
    m = nc.model("unreferenced")
    assert np.flatnonzero(m.flags).tolist() == [0, 5, 11] and (m.flags[[0, 5, 11]] == 3).all() and len(m.flags) == 12
    assert not m.normals[[0, 5, 11]].any() and m.stats == [12, 0, 3]
    assert (nc.model("no_faces").flags == 3).all() and (nc.model("soup_no_faces").flags == 3).all()
    # odd faces: (9, 9, 10) and (11, 11, 11) give the exact zero vector; 9, 10 and 11 are named, by nothing else: flag 2, not 1
    m = nc.model("odd_faces")
    f = nc.cases()["odd_faces"][1].tolist()
    assert [9, 9, 10] in f and [11, 11, 11] in f and f[0] == f[1] == [0, 1, 2] and [4, 5, 6] in f and [4, 5, 7] in f and [5, 4, 8] in f
    assert m.flags[[9, 10, 11]].tolist() == [2, 2, 2] and m.valence[9] == 2 and m.valence[11] == 3
    assert not m.face_vectors[[5, 6]].any()
    # a face given twice: the sums of its vertices are twice the face vector, the normals those of one copy
    assert np.array_equal(m.sums[[0, 1, 2]], 2 * np.tile(m.face_vectors[0], (3, 1))) and not m.flags[[0, 1, 2]].any()
    once = nc.Model(nc.cases()["odd_faces"][0], [[0, 1, 2]])
    assert np.array_equal(m.normals[[0, 1, 2]].view(U32), once.normals[[0, 1, 2]].view(U32))
    assert m.valence[4] == m.valence[5] == 3 and not m.flags[[4, 5]].any()  # three faces on the edge 4-5
    # the same triangle in both windings: exactly zero, flag 2
    m = nc.model("opposite")
    assert (m.flags == 2).all() and not m.sums.any() and not np.signbit(m.sums).any() and m.face_vectors[0].any()
    assert np.array_equal(m.face_vectors[0], -m.face_vectors[1]) and m.stats == [3, 0, 3]
    # coincident corners: different vertices, one position, inexact products -- and still exactly zero
    m = nc.model("coincident")
    v, f = nc.cases()["coincident"]
    assert (f[:, 1] != f[:, 2]).all() and np.array_equal(v[f[:, 1]], v[f[:, 2]]) and (v[f[:, 0]] != v[f[:, 1]]).any(1).all()
    mag = np.abs(v[v != 0])
    assert mag.min() < 1e-5 and mag.max() > 1e5
    assert not m.face_vectors.any() and (m.flags == 2).all() and m.n_skipped == 0
    # the add order: ascending the big faces cancel what the small ones added
    m = nc.model("add_order")
    assert m.face_vectors[:, 2].tolist() == [1.0, 1.0, 2.0 ** 60, -(2.0 ** 60)] and not m.face_vectors[:, :2].any()
    assert m.flags[0] == 2 and not m.normals[0].any() and m.valence[0] == 4
    # not finite: the faces are skipped, the neighbours keep what their other faces add and say so
    m = nc.model("non_finite")
    v = nc.cases()["non_finite"][0]
    assert np.isnan(v[5, 1]) and np.isinf(v[15, 2]) and v.view(U32)[6, 2] == 0x80000000
    assert np.flatnonzero(m.skipped_faces).tolist() == [3, 4, 5, 13, 14, 15] and m.n_skipped == 6
    assert m.flags[5] == 6 and m.flags[15] == 6 and not m.normals[[5, 15]].any()  # only skipped faces: 2 | 4
    for i in (3, 4, 6, 7, 13, 14, 16, 17):
        assert m.flags[i] == 4 and m.normals[i].any() and np.isfinite(m.normals[i]).all()
    assert not m.flags[[0, 1, 2, 8, 12, 18, 23]].any()
    # the random mesh: irregular valence; the soup: one degenerate and one skipped face among 257
    m = nc.model("random")
    assert len(m.normals) == 2000 and m.valence.max() >= 3 * max(1, m.valence.min()) and m.valence.max() > 12
    m = nc.model("random_soup_257")
    assert len(m.normals) == 771 and nc.cases()["random_soup_257"][1] is None and m.stats == [771, 1, 6]
    assert (m.flags[300:303] == 2).all() and (m.flags[600:603] == 6).all() and np.count_nonzero(m.flags) == 6
    assert np.array_equal(m.normals[0::3].view(U32), m.normals[1::3].view(U32)) and np.array_equal(m.normals[0::3].view(U32), m.normals[2::3].view(U32))
    # above the 64 KiB pinned-copy threshold
    v, f = nc.cases()["icosphere_5"]
    assert v.nbytes >= 64 << 10 and f.nbytes >= 64 << 10
    m = nc.model("icosphere_5")
    assert not m.flags.any() and ((m.normals.astype(np.float64) * unit(v.astype(np.float64) - 0.25)).sum(1) > 0.999).all()


def test_the_discriminators_tell_implementations_apart():
    """A pass that adds a vertex's faces in descending index, and one whose compiler contracts a * b - c * d into an FMA, give
    results different from the rule's -- on the cases made for that."""
    v, f = nc.cases()["add_order"]
    up, down = nc.model("add_order"), nc.Model(v, f, descending=True)
    assert up.flags[0] == 2 and down.flags[0] == 0 and down.sums[0].tolist() == [0.0, 0.0, 2.0] and down.normals[0].tolist() == [0.0, 0.0, 1.0]
    v, f = nc.cases()["coincident"]
    plain, fused = nc.model("coincident"), nc.Model(v, f, contracted=True)
    nonzero = fused.face_vectors.any(1)
    print(f"contracted: {int(nonzero.sum())} of {len(f)} coincident faces have a nonzero face vector")
    assert not plain.face_vectors.any() and nonzero.sum() > len(f) // 2
    assert (fused.flags != plain.flags).any() and (fused.normals.view(U32) != plain.normals.view(U32)).any()


# ---- orientation -------------------------------------------------------------------------------------------------------------
def test_normals_of_a_marched_sphere_point_out_of_the_surface():
    """Rule 5 on the CPU alone: the oracle's marching cubes on a sphere (d < 0 inside), vertices of identical words welded,
    the model on that mesh: every normal is within 8.1 degrees of the radial direction, outwards -- towards increasing d."""
    from oracle.oracle import OracleVolume
    from tests.common import make_volume
    vol, _ = make_volume(nc.SPHERE_RES)
    d, w, centre = nc.sphere_field(vol._p)
    ov = OracleVolume(vol._p, adopt=(d, w, None))
    soup, _, _ = ov.march(1.0)
    words, index = np.unique(np.ascontiguousarray(soup).view(U32), axis=0, return_inverse=True)
    verts, faces = words.view(F32), index.reshape(-1, 3)
    m = nc.Model(verts, faces)
    dots = (m.normals.astype(np.float64) * unit(verts.astype(np.float64) - centre)).sum(1)
    print(f"{len(faces)} triangles, {len(verts)} vertices, {m.n_zero} zero normals, minimum dot {dots.min():.4f}")
    assert len(faces) > 3000 and len(verts) > 1500
    assert not m.flags.any()
    assert dots.min() >= 0.99
    # flat normals of the soup itself point the same way
    flat = nc.Model(soup, None)
    assert ((flat.normals.astype(np.float64) * unit(soup.astype(np.float64) - centre)).sum(1)[flat.flags == 0] > 0.9).all()


# ---- the PLY writer ------------------------------------------------------------------------------------------------------------
def ply_bytes(verts, faces, binary, rgb=None, normals=None):
    """what save_ply writes: the header, then per vertex x y z [r g b] [nx ny nz] -- ascii with 5 significant digits -- and the
    faces"""
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment PCL generated", "element vertex %d" % len(verts),
            "property float x", "property float y", "property float z"]
    if rgb is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    out = ("\n".join(head) + "\n").encode()
    for i in range(len(verts)):
        if binary:
            out += np.asarray(verts[i], F32).tobytes()
            if rgb is not None:
                out += bytes(rgb[i].tolist())
            if normals is not None:
                out += np.asarray(normals[i], F32).tobytes()
        else:
            row = ["%.5g" % x for x in verts[i].tolist()]
            if rgb is not None:
                row += ["%d" % c for c in rgb[i].tolist()]
            if normals is not None:
                row += ["%.5g" % x for x in normals[i].tolist()]
            out += (" ".join(row) + "\n").encode()
    for f in np.asarray(faces).tolist():
        out += (b"\x03" + np.asarray(f, np.int32).tobytes()) if binary else ("3 %d %d %d\n" % tuple(f)).encode()
    return out


@pytest.mark.parametrize("colour", [False, True], ids=["xyz", "xyzrgb"])
def test_ply_writer_writes_the_normal_fields_and_nothing_else_changes(harness, tmp_path, colour):
    v, f = nc.cases()["grid_5x5"]
    rgb = np.random.default_rng(3).integers(0, 256, (len(v), 3)).astype(np.uint8) if colour else None
    src = str(tmp_path / "mesh.bin")
    write_mesh(src, v, f, rgb=rgb)
    want = nc.model("grid_5x5").normals
    for normals in (0, 1, 2):  # none; computed once; computed twice: the fields are rewritten, not appended again
        prefix = str(tmp_path / f"out{normals}")
        subprocess.run([harness, "ply", src, prefix, str(normals)], check=True, timeout=120)
        for binary in (False, True):
            got = open(prefix + (".binary.ply" if binary else ".ascii.ply"), "rb").read()
            assert got == ply_bytes(v, f, binary, rgb, want if normals else None), (normals, binary)
    # a soup goes the same way, with flat normals
    v, _ = nc.random_soup()
    write_mesh(src, v, None)
    prefix = str(tmp_path / "soup")
    subprocess.run([harness, "ply", src, prefix, "1"], check=True, timeout=120)
    faces = np.arange(len(v)).reshape(-1, 3)
    assert open(prefix + ".binary.ply", "rb").read() == ply_bytes(v, faces, True, None, nc.model("random_soup_257").normals)


def test_a_polygon_that_is_not_a_triangle_refuses_the_mesh(tmp_path):
    """meshNormals on a PolygonMesh with a quad: E_INVALID, the mesh untouched."""
    from cpu_tsdf_amd import build as b
    src = tmp_path / "quad.cpp"
    src.write_text("""
#include <pcl/PolygonMesh.h>
#include "mesh_post.h"
int main() {
  pcl::PolygonMesh mesh;
  const std::vector<float> xyz = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0};
  const uint32_t tri[3] = {0, 1, 2};
  cpu_tsdf::mesh_post::storeDecimated(xyz, {}, 4, tri, 1, mesh);
  mesh.polygons[0].vertices.push_back(3);
  const pcl::PolygonMesh before = mesh;
  std::string why;
  if (cpu_tsdf::mesh_post::meshNormals(mesh, &why) != TSDF_HIP_E_INVALID) return 1;
  if (why.find("not a triangle") == std::string::npos) return 2;
  if (mesh.cloud.data != before.cloud.data || mesh.cloud.fields.size() != 3 || mesh.cloud.point_step != before.cloud.point_step) return 3;
  mesh.polygons[0].vertices.pop_back();
  if (cpu_tsdf::mesh_post::meshNormals(mesh, &why) != 0) return 4;
  if (mesh.cloud.fields.size() != 6 || mesh.cloud.fields[3].name != "normal_x" || mesh.cloud.fields[5].name != "normal_z") return 5;
  if (mesh.cloud.point_step != before.cloud.point_step + 12 || mesh.cloud.fields[3].offset != before.cloud.point_step) return 6;
  float n[3];
  memcpy(n, mesh.cloud.data.data() + mesh.cloud.fields[3].offset, 12);
  return n[0] == 0.f && n[1] == 0.f && n[2] == 1.f ? 0 : 7;
}
""")
    exe = str(tmp_path / "quad")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, str(src), "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    subprocess.run([exe], check=True, timeout=60)
