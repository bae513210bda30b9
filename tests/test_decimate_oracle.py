"""CPU tier: the numpy model of the decimateMesh tests (tests/decimate_cases.py: the SEQUENTIAL pass restated) against the
host pass it restates -- cpu_tsdf::mesh_post::decimateArrays, run through tests/harness/meshdec.cpp, which touches no device.
remap, output vertices (bit for bit), colours, member counts and faces must be equal on every case the GPU tests use: this
pins the model here, without a GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import decimate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def build_harness(dirpath):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(dirpath / "meshdec")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tests", "harness", "meshdec.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip",
                           "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def write_mesh(path, verts, faces, rgb):
    with open(path, "wb") as f:
        f.write(struct.pack("<3q", len(verts), -1 if faces is None else len(faces), 0 if rgb is None else 1))
        f.write(np.ascontiguousarray(verts, F32).tobytes())
        if rgb is not None:
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
        if faces is not None:
            f.write(np.ascontiguousarray(faces, np.uint32).tobytes())


def host_pass(harness, tmp_path, verts, faces, rgb, cell):
    """-> (rc, dict or the refusal's text)"""
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, verts, faces, rgb)
    subprocess.run([harness, "arrays", src, out, repr(float(F32(cell)))], check=True, timeout=120)
    raw = open(out, "rb").read()
    rc, = struct.unpack_from("<q", raw, 0)
    if rc:
        return rc, raw[8:].decode()
    n, m, k, has_rgb, dup = struct.unpack_from("<5q", raw, 8)
    at = 48
    got = {"duplicates": dup}
    for name, dtype, count, shape in (("remap", np.uint32, n, (n,)), ("vertices", np.uint32, 3 * m, (m, 3)), ("rgb", np.uint8, 3 * m * has_rgb, (m, 3)),
                                      ("counts", np.uint32, m, (m,)), ("polygons", np.uint32, 3 * k, (k, 3))):
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        got[name] = a.reshape(shape) if count or name != "rgb" else None
    assert at == len(raw)
    return 0, got


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshdec"))


@pytest.mark.parametrize("name", sorted(dc.cases()))
def test_host_pass_equals_the_numpy_model(harness, tmp_path, name):
    verts, faces, rgb, cell, with_faces = dc.cases()[name]
    want = dc.model(name)
    if not with_faces:
        faces = np.empty((0, 3), np.uint32)
    rc, got = host_pass(harness, tmp_path, verts, faces, rgb, cell)
    assert rc == 0, got
    assert np.array_equal(got["remap"], want.remap), "remap differs from the model's"
    assert np.array_equal(got["vertices"], want.vertices.view(np.uint32)), "output vertices differ from the model's"
    assert np.array_equal(got["counts"], want.counts)
    if rgb is None:
        assert got["rgb"] is None
    else:
        assert np.array_equal(got["rgb"], want.rgb), "colours differ from the model's"
    if with_faces:
        assert np.array_equal(got["polygons"], want.polygons.astype(np.uint32)), "faces differ from the model's"
        assert got["duplicates"] == int(want.duplicate.sum())
    else:
        assert len(got["polygons"]) == 0


def test_extent_refusal(harness, tmp_path):
    """One vertex at cell index 2^20 refuses the call; -2^20 and 2^20 - 1 (the case extent_edges) are accepted."""
    with pytest.raises(dc.ExtentError):
        dc.Dec(dc.extent_refused(), None, None, 1.0)
    rc, why = host_pass(harness, tmp_path, dc.extent_refused(), np.empty((0, 3), np.uint32), None, 1.0)
    assert rc == 1 and "1048576" in why  # E_INVALID, and the text names the extent
    cell = dc.model("extent_edges").cell
    assert cell.min() == -(1 << 20) and cell.max() == (1 << 20) - 1


def test_bad_arguments_of_the_host_pass(harness, tmp_path):
    v = dc.extent_edges()
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert host_pass(harness, tmp_path, v, None, None, cell)[0] == 1, cell
    assert host_pass(harness, tmp_path, v, np.asarray([[0, 1, 5]], np.uint32), None, 1.0)[0] == 1  # a face names vertex 5 of 5
    rc, got = host_pass(harness, tmp_path, np.empty((0, 3), F32), None, None, 1.0)
    assert rc == 0 and len(got["remap"]) == 0 and len(got["vertices"]) == 0 and len(got["polygons"]) == 0


def test_the_cases_say_what_they_are_meant_to():
    """What the GPU tests rely on, derived from the model alone."""
    # 5 to 10 vertices per cell
    o = dc.model("random_cloud")
    assert 5 <= np.median(o.counts) <= 10 and len(o.counts) == 512 + 4
    assert len(dc.model("exact_duplicates").counts) == 800 + 4 and (dc.model("exact_duplicates").counts[:10] == 5).all()
    # cell borders: see the comments in cell_borders()
    o = dc.model("cell_borders")
    assert o.remap.tolist() == [0, 1, 0, 2, 3, 4, 5, 5, 5, 5, 6, 7, 6, 8, 9, 9]
    assert o.cell[0, 0] == -2 and o.cell[1, 0] == -1 and (o.cell[5] == -1).all() and (o.cell[8] == 0).all()
    assert (o.cell[10] == 3).all() and o.cell[11].tolist() == [2, 3, 3] and (o.cell[14] == -3).all()
    assert o.vertices.view(np.uint32)[8, 0] == 0x80000000  # the lone -0.0 kept its sign: no arithmetic touched it
    assert o.vertices.view(np.uint32)[5, 0] != 0x80000000 and o.vertices[5, 0] > 0  # +0, -0, 0.0125, 0.125 averaged
    assert int(dc.model("big_bucket").counts.max()) == 3000
    # the add order shows in the float: the ascending copy rounds up, the descending one down
    o = dc.model("add_order")
    v = dc.add_order()
    by_row = {name: int(o.remap[np.flatnonzero((v[:, 1] == F32(y)) & (v[:, 2] == F32(0.5)))[0]]) for name, y in dc.ORDER_ROWS.items()}
    assert o.counts[by_row["ascending"]] == o.counts[by_row["descending"]] == 8
    up, down = o.vertices[by_row["ascending"], 0], o.vertices[by_row["descending"], 0]
    assert down == F32(0.5) and up == np.nextafter(F32(0.5), F32(1)), (up, down)
    # and a pairwise (tree) sum of the descending copy does NOT give what the sequential adds give
    x = dc.order_series()[::-1].astype(np.float64)
    tree = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))
    assert F32(tree / 8.0) != down
    # NaN / Inf: clusters of their own, bits kept
    o = dc.model("nan_mesh")
    for at in dc.NAN_AT:
        assert o.counts[o.remap[at]] == 1
    bits = o.vertices.view(np.uint32)
    assert bits[o.remap[100], 1] == dc.NAN_BITS[0] and bits[o.remap[101], 0] == dc.NAN_BITS[1] and np.isinf(o.vertices[o.remap[102], 2])
    assert o.keep[303] and o.duplicate[301] and not o.duplicate[300] and o.degenerate[302]
    # many duplicates on the snapped mesh
    o = dc.model("snapped_indexed")
    assert int(o.duplicate.sum()) >= 20 and np.array_equal(dc.model("snapped_soup").keep, o.keep)
    # opposite orientation: the lower index survives with its own orientation
    o = dc.model("opposite_faces")
    assert o.keep.tolist() == [True, False, False, True, False] and o.polygons.tolist() == [[0, 1, 2], [3, 0, 1]]
    assert dc.model("colour_rounding").rgb.tolist() == [[11, 1, 255], [2, 255, 0], [255, 0, 8], [9, 8, 7]]
