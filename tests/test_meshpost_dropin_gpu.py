"""GPU tier: the `integrate` program's --cleanup through tests/harness/meshpost.cpp -- cpu_tsdf::mesh_post::cleanupMesh (the
host pass, which defines the result) and cleanupMeshGpu (the face set from tsdf_hip_mesh_cleanup, the host's own tail) on
copies of one indexed mesh with shared vertices.  The two results must be byte-equal: the point cloud blob and every
polygon.  The mesh is the random cloud of tests/test_meshpost_gpu.py, which pins the face set to the numpy oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_meshpost_gpu import FD, centroids, indexed_random_mesh, oracle_keep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(tmp_path_factory.mktemp("meshpost") / "meshpost")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tests", "harness", "meshpost.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip",
                           "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def read_mesh(raw, at):
    step, blob_bytes, n_poly = struct.unpack_from("<3q", raw, at)
    at += 24
    blob = raw[at:at + blob_bytes]
    at += blob_bytes
    polys = []
    for _ in range(n_poly):
        k, = struct.unpack_from("<q", raw, at)
        polys.append(struct.unpack_from(f"<{k}I", raw, at + 8))
        at += 8 + 4 * k
    return (step, blob, polys), at


def test_gpu_backed_cleanup_equals_the_host_pass_byte_for_byte(harness, tmp_path):
    pool, faces = indexed_random_mesh()
    keep = oracle_keep(centroids(pool, faces), FD, 5)
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<2q", len(pool), len(faces)))
        f.write(pool.astype(np.float32).tobytes())
        f.write(faces.astype(np.uint32).tobytes())
    subprocess.run([harness, src, out, repr(FD), "5"], check=True, timeout=300)
    raw = open(out, "rb").read()
    host, at = read_mesh(raw, 0)
    gpu_mesh, at = read_mesh(raw, at)
    assert at == len(raw)
    assert len(host[2]) == int(keep.sum()) and 0 < len(host[2]) < len(faces)
    assert host[0] == gpu_mesh[0] and host[1] == gpu_mesh[1], "the point cloud blobs differ"
    assert host[2] == gpu_mesh[2], "the polygons differ"
    # unused vertices went: the blob holds exactly the vertices the surviving faces name
    assert len(host[1]) == host[0] * len(np.unique(faces[keep]))
