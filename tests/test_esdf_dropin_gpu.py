"""GPU tier: computeDistanceField above the C ABI.  The C++ drop-in's computeDistanceField / getDistanceField / getDistance,
through tests/harness/esdf.cpp, fuse the same frames into their own 32^3 volume and must return the Python binding's d2 and
dist byte for byte; getDistance must return getDistanceField's value at the voxel that contains the point; before reset(),
and before the first computeDistanceField, the members return false.  `tsdf2mesh A.vol out.ply --esdf out.npy` must write a
.npy that numpy.load reads, with the bits of the Python call."""
import os
import struct
import subprocess

import numpy as np
import pytest

from cpu_tsdf_amd.volume import TSDFVolumeOctree
from tests import esdf_cases as ec
from tests import sequence_util as su
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, NPTS = 32, 100


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(tmp_path_factory.mktemp("esdf") / "esdf")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [os.path.join(ROOT, "tests", "harness", "esdf.cpp"), "-L" + b.LIBDIR,
                                                                            "-lcpu_tsdf_hip", "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def fused():
    vol, sc = make_volume(RES, 160, 120, color=False)
    vol.reset()
    fr = [(tr, dep) for i, tr, dep, col in frames(sc, 4, 8)]
    for tr, dep in fr:
        vol.integrateCloud(dep, None, tr)
    return vol, sc, fr


@pytest.fixture(scope="module")
def run(harness, tmp_path_factory):
    vol, sc, fr = fused()
    planes = vol.download()
    rng = np.random.RandomState(11)
    pts = rng.uniform(-0.55 * sc.size, 0.55 * sc.size, (NPTS, 3)).astype(np.float32)
    res = dict(py=[], cpp=[], pts=pts, vol_index=[vol.getVoxelIndex(*pt) for pt in pts], half=sc.size / 2)
    for r in (0, 2):
        n = vol.computeDistanceField(r)
        want = ec.model(vol._p, planes[0], planes[1], None, r)
        assert n == want[2] and n > 200
        res["py"].append((n,) + vol.getDistanceField())
        assert np.array_equal(res["py"][-1][1], want[0]) and res["py"][-1][2].tobytes() == want[1].tobytes(), "the Python binding differs from the model"
    vol.close()
    tmp = tmp_path_factory.mktemp("esdf_io")
    inp, out = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<5q", RES, sc.width, sc.height, len(fr), NPTS))
        f.write(struct.pack("<5d", sc.size, sc.fx, sc.fy, sc.cx, sc.cy))
        for tr, dep in fr:
            f.write(np.ascontiguousarray(tr, np.float64).tobytes())
            f.write(np.ascontiguousarray(dep, np.float32).tobytes())
        f.write(pts.tobytes())
    subprocess.run([harness, inp, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    nv = RES ** 3
    per = 16 + 8 * nv + 12 * NPTS
    assert len(raw) == 8 + 2 * per
    res["refused"] = struct.unpack_from("<q", raw, 0)[0]
    for k in range(2):
        off = 8 + k * per
        ok, sites = struct.unpack_from("<qQ", raw, off)
        res["cpp"].append((ok, sites, np.frombuffer(raw, np.uint32, nv, off + 16).reshape(RES, RES, RES),
                           np.frombuffer(raw, np.float32, nv, off + 16 + 4 * nv).reshape(RES, RES, RES),
                           np.frombuffer(raw, np.int64, NPTS, off + 16 + 8 * nv), np.frombuffer(raw, np.float32, NPTS, off + 16 + 8 * nv + 8 * NPTS)))
    return res


@pytest.mark.parametrize("k", [0, 1], ids=["unlimited", "r_max_2"])
def test_cpp_members_return_the_python_bindings_bytes(run, k):
    (n, d2, dist), (ok, sites, c_d2, c_dist, found, val) = run["py"][k], run["cpp"][k]
    assert ok == 1 and sites == n
    assert c_d2.tobytes() == d2.tobytes(), "d2 differs from the Python binding"
    assert c_dist.tobytes() == dist.tobytes(), "dist differs from the Python binding"
    if k == 1:
        assert (d2 == ec.FAR).any() and (d2 != ec.FAR).any() and d2[d2 != ec.FAR].max() == 4


@pytest.mark.parametrize("k", [0, 1], ids=["unlimited", "r_max_2"])
def test_get_distance_matches_the_field_at_the_points_voxel(run, k):
    _, _, _, c_dist, found, val = run["cpp"][k]
    inside = 0
    for pt, (ok, (i, j, kz)), f, v in zip(run["pts"], run["vol_index"], found, val):
        ok = ok and bool(np.all(np.abs(pt) <= np.float32(run["half"])))
        assert f == (1 if ok else 0), pt
        if ok:
            inside += 1
            assert np.float32(v).tobytes() == c_dist[kz, j, i].tobytes(), pt
        else:
            assert v == 7
    assert 30 < inside < NPTS


def test_members_before_reset_return_false(run):
    assert run["refused"] == 1


def test_tsdf2mesh_writes_the_field_as_npy(gpu, tmp_path):
    if not os.path.exists(su.OUR_TSDF2MESH):
        from cpu_tsdf_amd import build as b
        b.build_programs()
    vol, _, _ = fused()
    a_vol = str(tmp_path / "a.vol")
    vol.save(a_vol)
    vol.close()
    a = TSDFVolumeOctree()
    a.load(a_vol)
    want = {}
    for r in (0, 2):
        assert a.computeDistanceField(r) > 200
        want[r] = a.getDistanceField()[1]
    a.close()
    assert want[0].tobytes() != want[2].tobytes()
    ply, plain = str(tmp_path / "out.ply"), str(tmp_path / "plain.ply")
    rc, log = su.run(su.OUR_TSDF2MESH, [a_vol, plain])
    assert rc == 0, log[-2000:]
    for r, extra in ((0, []), (2, ["--esdf-radius", "2"])):
        npy = str(tmp_path / f"field_{r}.npy")
        rc, log = su.run(su.OUR_TSDF2MESH, [a_vol, ply, "--esdf", npy] + extra)
        assert rc == 0, log[-2000:]
        got = np.load(npy)
        assert got.shape == (RES, RES, RES) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        assert got.tobytes() == want[r].tobytes(), f"--esdf (radius {r}) differs from the Python call"
        assert open(npy, "rb").read(8) == b"\x93NUMPY\x01\x00"
        assert open(ply, "rb").read() == open(plain, "rb").read()  # the mesh is what it was
    rc, log = su.run(su.OUR_TSDF2MESH, [a_vol, ply, "--esdf", str(tmp_path / "no_such_dir" / "x.npy")])
    assert rc == 1
