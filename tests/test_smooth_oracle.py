"""CPU tier: the numpy model of the smoothMesh tests (tests/smooth_cases.py) against the host pass that defines the result --
cpu_tsdf::mesh_post::smoothArrays, run through tests/harness/meshsmooth.cpp, which touches no device.  Output vertices (as
words), fixed bits and degrees must be equal on every case the GPU tests use: this pins the model here, without a GPU.  And two
properties of the rule itself, on the model alone: Taubin's mu step removes noise without shrinking a sphere, the plain
Laplacian shrinks it."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import smooth_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
E_INVALID = 1


def build_harness(dirpath):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(dirpath / "meshsmooth")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + b.host_include_flags() +
                          ["-I" + b.PROG, os.path.join(ROOT, "tests", "harness", "meshsmooth.cpp"), "-L" + b.LIBDIR, "-lcpu_tsdf_hip",
                           "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def write_mesh(path, verts, faces, rgb=None):
    with open(path, "wb") as f:
        f.write(struct.pack("<3q", len(verts), -1 if faces is None else len(faces), 0 if rgb is None else 1))
        f.write(np.ascontiguousarray(verts, F32).tobytes())
        if rgb is not None:
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
        if faces is not None:
            f.write(np.ascontiguousarray(faces, U32).tobytes())


def args(lam, mu, iterations, keep_boundary):
    return [repr(float(F32(lam))), repr(float(F32(mu))), str(int(iterations)), str(int(keep_boundary))]


def host_pass(harness, tmp_path, verts, faces, lam, mu, iterations, keep_boundary):
    """-> (rc, dict) or (rc, the refusal's text, was the output left untouched)"""
    src, out = str(tmp_path / "mesh.bin"), str(tmp_path / "out.bin")
    write_mesh(src, verts, faces)
    subprocess.run([harness, "arrays", src, out] + args(lam, mu, iterations, keep_boundary), check=True, timeout=120)
    raw = open(out, "rb").read()
    rc, = struct.unpack_from("<q", raw, 0)
    if rc:
        return rc, raw[8:-1].decode(), raw[-1] == 1
    n, edges = struct.unpack_from("<2q", raw, 8)
    at = 24
    got = {"edges": edges}
    for name, dtype, count, shape in (("vertices", U32, 3 * n, (n, 3)), ("fixed", np.uint8, n, (n,)), ("degree", U32, n, (n,))):
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        got[name] = a.reshape(shape)
    assert at == len(raw)
    return 0, got


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("meshsmooth"))


@pytest.mark.parametrize("name", sorted(sc.cases()))
def test_host_pass_equals_the_numpy_model(harness, tmp_path, name):
    want = sc.model(name)
    rc, got = host_pass(harness, tmp_path, *sc.cases()[name])
    assert rc == 0, got
    assert np.array_equal(got["degree"], want.degree), "degrees differ from the model's"
    assert np.array_equal(got["fixed"], want.fixed), "fixed bits differ from the model's"
    bad = np.flatnonzero((got["vertices"] != want.vertices.view(U32)).any(1))
    assert len(bad) == 0, f"{len(bad)} of {len(want.vertices)} output vertices differ from the model's, first {bad[:8].tolist()}"
    assert got["edges"] == want.n_edges


def test_refusals_of_the_host_pass(harness, tmp_path):
    v, f = sc.grid_patch()
    ok = dict(lam=0.5, mu=-0.53, iterations=2, keep_boundary=1)
    refused = [dict(lam=x) for x in (0.0, -0.5, 1.5, float("nan"), float("inf"))]
    refused += [dict(mu=x) for x in (0.1, -1.5, float("nan"), float("-inf"))]
    refused += [dict(iterations=x) for x in (-1, 1001)]
    for bad in refused:
        rc, why, untouched = host_pass(harness, tmp_path, v, f, **dict(ok, **bad))
        assert rc == E_INVALID and untouched and next(iter(bad)).replace("lam", "lambda") in why, (bad, why)
    rc, why, untouched = host_pass(harness, tmp_path, v, None, **ok)  # a soup: faces == NULL
    assert rc == E_INVALID and untouched and "flatten or decimate first" in why
    f = f.copy()
    f[7, 2] = len(v)
    rc, why, untouched = host_pass(harness, tmp_path, v, f, **ok)
    assert rc == E_INVALID and untouched and ">= n_verts" in why
    # the ends of the ranges are accepted, and an empty mesh is
    v, f = sc.grid_patch()
    assert host_pass(harness, tmp_path, v, f, 1.0, -1.0, 1000, 0)[0] == 0
    rc, got = host_pass(harness, tmp_path, np.empty((0, 3), F32), sc.NO_FACES, **ok)
    assert rc == 0 and got["vertices"].shape == (0, 3) and got["edges"] == 0


def test_the_cases_say_what_they_are_meant_to():
    """What the GPU tests rely on, derived from the model alone."""
    m = sc.model("tetrahedron")
    assert (m.degree == 3).all() and not m.fixed.any() and m.n_edges == 6 and m.steps == 8
    # the patch: boundary ring fixed only with keep_boundary; the interior moves either way
    free, kept = sc.model("grid_keep0"), sc.model("grid_keep1")
    ring = np.asarray([i in (0, 4) or j in (0, 4) for i in range(5) for j in range(5)])
    assert not free.fixed.any() and np.array_equal(kept.fixed, ring * 4)
    v = sc.grid_patch()[0]
    assert np.array_equal(kept.vertices.view(U32)[ring], v.view(U32)[ring]) and (kept.vertices[~ring] != v[~ring]).any(1).all()
    assert (free.vertices != v).any(1).all()
    # the fans: a hub of degree 300; the disc's rim is boundary, the double fan has none, and the hubs move
    m = sc.model("fan_300")
    assert m.degree[0] == 300 and m.fixed[0] == 0 and (m.fixed[1:] == 4).all() and (m.vertices[0] != sc.fan()[0][0]).all()
    m = sc.model("double_fan_300")
    assert m.degree[0] == m.degree[1] == 300 and not m.fixed.any() and (m.vertices[:2] != sc.fan(300, 2)[0][:2]).all()
    assert sc.model("strip_1").fixed.tolist() == [2] and len(sc.cases()["strip_1"][1]) == 0
    for n in (255, 256, 257):
        assert len(sc.model(f"strip_{n}").vertices) == n and not sc.model(f"strip_{n}").fixed.any()
    # vertices in no face: first, in the middle, last
    m = sc.model("unreferenced")
    assert np.flatnonzero(m.fixed).tolist() == [0, 5, 11] and (m.fixed[[0, 5, 11]] == 2).all() and int(sc.cases()["unreferenced"][1].max()) == 10
    # multiplicities: a face twice and three faces on an edge are not boundary; (9, 9, 10) names 9-10 twice; (11, 11, 11) nothing
    m = sc.model("odd_faces_keep1")
    assert m.fixed[[0, 1, 2]].tolist() == [0, 0, 0] and m.fixed[[9, 10]].tolist() == [0, 0] and m.fixed[11] == 2 and m.degree[11] == 0
    assert (m.fixed[[4, 5, 6, 7, 8]] == 4).all() and m.degree[4] == m.degree[5] == 4 and m.degree[9] == m.degree[10] == 1
    assert sc.model("odd_faces_keep0").fixed.tolist() == [0] * 11 + [2, 0, 0]
    # not finite: the vertex and its neighbours are fixed with their words; neighbours of neighbours move
    m = sc.model("non_finite")
    v = sc.non_finite()[0]
    assert np.flatnonzero(m.fixed).tolist() == [3, 4, 5, 6, 7, 13, 14, 15, 16, 17] and (m.fixed[m.fixed != 0] == 1).all()
    assert m.vertices.view(U32)[5, 1] == sc.NAN_BITS and np.isinf(m.vertices[15, 2]) and m.vertices.view(U32)[6, 2] == 0x80000000
    assert (m.vertices[[2, 8, 12, 18]] != v[[2, 8, 12, 18]]).any(1).all()
    # step counts that end in either buffer
    assert [sc.model(k).steps for k in ("grid_steps_1_nomu", "grid_steps_1_mu", "grid_steps_2_nomu", "grid_steps_3_mu", "grid_steps_0_mu")] == [1, 2, 2, 6, 0]
    assert np.array_equal(sc.model("grid_steps_0_mu").vertices.view(U32), sc.grid_patch(6, seed=8)[0].view(U32))
    # the random mesh: irregular degrees, many non-manifold edges
    m = sc.model("random")
    assert len(m.vertices) == 2000 and m.degree.max() > 2 * m.degree.min() > 0 and np.isfinite(m.vertices).all()


def test_the_add_order_case_tells_the_orders_apart():
    """A model that sums the neighbours in DESCENDING index must give another result.  On the random mesh it cannot: its
    coordinates span 1e-3 .. 1e3, so a double sum of them needs 24 + 20 bits and every partial sum is exact, in any order
    (measured: 0 of 2000 vertices differ, also with coordinates over 1e-8 .. 1e8, where the sums differ in their last bits and
    the difference is rounded away in the cast to float).  The order shows where a sum cancels: `add_order` has a vertex whose
    neighbours hold 1, 1, 2^60 and -2^60 in ascending index."""
    c = sc.cases()["add_order"]
    up, down = sc.model("add_order"), sc.Model(*c, descending=True)
    assert up.vertices[0, 0] != down.vertices[0, 0]
    assert up.fixed[0] == 0 and up.degree[0] == 4
    r = sc.cases()["random"]
    assert np.array_equal(sc.Model(*r, descending=True).vertices.view(U32), sc.model("random").vertices.view(U32))


def test_taubin_removes_noise_without_shrinking_and_laplacian_shrinks():
    v, f = sc.icosphere(4)
    assert v.shape == (2562, 3) and f.shape == (5120, 3)
    rng = np.random.default_rng(5)
    x = (v * (0.5 * (1.0 + rng.normal(0, 0.01, len(v))))[:, None] + 1.0).astype(F32)

    def radius(p):
        return np.linalg.norm(p.astype(np.float64) - 1.0, axis=1) / 0.5

    before = radius(x)
    taubin = radius(sc.Model(x, f, 0.5, -0.53, 10, 1).vertices)
    laplace = radius(sc.Model(x, f, 0.5, 0.0, 10, 1).vertices)
    print(f"std of the normalised radius: input {before.std():.5f}, Taubin {taubin.std():.5f}; mean: Taubin {taubin.mean():.4f}, "
          f"Laplacian {laplace.mean():.4f}")
    assert taubin.std() <= 0.5 * before.std()
    assert abs(taubin.mean() - 1.0) <= 0.005
    assert laplace.mean() < 0.99
