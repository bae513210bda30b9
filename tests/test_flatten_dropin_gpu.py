"""GPU tier: the `integrate` program's --flatten through tests/harness/meshflat.cpp -- cpu_tsdf::mesh_post::flattenVertices
(the host pass, which defines the result) and flattenVerticesGpu (seeds and faces from tsdf_hip_mesh_flatten, the vertex blob
built by the host's own tail) on copies of one indexed mesh with shared vertices.  The two results must be byte-equal: the
point cloud blob and every polygon.  The mesh is the snapped one of tests/flatten_cases.py, which tests/test_flatten_gpu.py
pins to the numpy oracle."""
import subprocess

import numpy as np
import pytest

from tests import flatten_cases as fc
from tests.test_flatten_oracle import build_harness, read_mesh, write_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshflat"))


def test_gpu_backed_flatten_equals_the_host_pass_byte_for_byte(harness, tmp_path):
    pool, faces = fc.snapped_mesh()
    want = fc.oracle("snapped_indexed")
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, pool, faces)
    subprocess.run([harness, src, out, repr(float(fc.SNAP_MD))], check=True, timeout=300)
    raw = open(out, "rb").read()
    host, at = read_mesh(raw, 0)
    gpu_mesh, at = read_mesh(raw, at)
    assert at == len(raw)
    assert len(host[1]) == len(want.polygons) and 0 < len(host[1]) < len(faces)
    assert len(host[0]) == len(want.seeds) and 2 <= len(host[0]) < len(pool)
    assert host[2] == gpu_mesh[2] and host[3] == gpu_mesh[3], "the point cloud blobs differ"
    assert np.array_equal(host[1], gpu_mesh[1]), "the polygons differ"
