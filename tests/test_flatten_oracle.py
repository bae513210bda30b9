"""CPU tier: the numpy oracle of the flattenVertices tests (tests/flatten_cases.py: the SEQUENTIAL loop restated) against the
host pass it restates -- cpu_tsdf::mesh_post::flattenVertices, run through tests/harness/meshflat.cpp in --host-only mode,
which touches no device.  Output vertices (bit for bit) and polygons must be equal on every case the GPU tests use: this
pins the oracle here, without a GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import flatten_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness(dirpath):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(dirpath / "meshflat")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tests", "harness", "meshflat.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip",
                           "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def write_mesh(path, verts, faces):
    with open(path, "wb") as f:
        f.write(struct.pack("<2q", len(verts), len(faces)))
        f.write(np.ascontiguousarray(verts, np.float32).tobytes())
        f.write(np.ascontiguousarray(faces, np.uint32).tobytes())


def read_mesh(raw, at):
    """(xyz bits (m, 3) uint32, polygons (k, 3) int64, point_step, blob), next offset."""
    step, blob_bytes, n_poly = struct.unpack_from("<3q", raw, at)
    at += 24
    blob = raw[at:at + blob_bytes]
    at += blob_bytes
    xyz = np.frombuffer(blob, np.uint8).reshape(-1, step)[:, :12].copy().view(np.uint32).reshape(-1, 3) if blob_bytes else np.empty((0, 3), np.uint32)
    polys = []
    for _ in range(n_poly):
        k, = struct.unpack_from("<q", raw, at)
        polys.append(struct.unpack_from(f"<{k}I", raw, at + 8))
        at += 8 + 4 * k
    return (xyz, np.asarray(polys, np.int64).reshape(-1, 3), step, blob), at


def faces_of(verts, faces, with_faces):
    if faces is not None:
        return faces
    return np.arange(len(verts), dtype=np.uint32).reshape(-1, 3) if with_faces else np.empty((0, 3), np.uint32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshflat"))


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_host_pass_equals_the_numpy_oracle(harness, tmp_path, name):
    verts, faces, md, with_faces = fc.cases()[name]
    want = fc.oracle(name)
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, verts, faces_of(verts, faces, with_faces))
    subprocess.run([harness, src, out, repr(float(md)), "--host-only"], check=True, timeout=120)
    raw = open(out, "rb").read()
    (xyz, polys, _, _), at = read_mesh(raw, 0)
    assert at == len(raw)
    assert np.array_equal(xyz, want.vertices.view(np.uint32)), "output vertices differ from the oracle's"
    if with_faces:
        assert np.array_equal(polys, want.polygons), "polygons differ from the oracle's"
    else:
        assert len(polys) == 0


def test_the_cases_say_what_they_are_meant_to():
    """What the GPU tests rely on, derived from the oracle alone."""
    o = fc.oracle("dense_cloud")
    # the last-writer rule is observable: a merged vertex whose remap is not that of its lowest seed neighbour
    is_seed = np.zeros(len(o.remap), bool)
    is_seed[o.seeds] = True
    differ = 0
    for j in np.flatnonzero(~is_seed)[:400]:
        nb = o.neighbours(j)
        s = np.sort(nb[is_seed[nb]])
        assert len(s) and o.remap[j] == o.remap[s[-1]]
        differ += int(o.remap[j] != o.remap[s[0]])
    assert differ > 0
    o = fc.oracle("chain_index")
    assert o.seeds.tolist() == list(range(0, 500, 2))
    assert fc.oracle("chain_reversed").seeds.tolist() == list(range(0, 500, 2))  # in ITS index order: the other end's vertices
    assert not np.array_equal(np.sort(fc.chain("reversed")[fc.oracle("chain_reversed").seeds.astype(int), 0]),
                              np.sort(fc.chain("index")[o.seeds.astype(int), 0]))
    assert len(fc.oracle("exact_duplicates").seeds) == 800
    assert fc.oracle("strict_pairs").remap.tolist() == [0, 1, 2, 2]
    assert fc.oracle("strict_pairs_2").remap.tolist() == [0, 1, 2, 2]
