"""GPU tier: castRays above the C ABI.  cpu_tsdf::TSDFVolumeOctree::castRays of the C++ drop-in, through
tests/harness/castrays.cpp, fuses three organised host clouds (pcl::PointCloud<pcl::PointXYZRGBA>) into its own 32^3 volume,
casts 500 rays read from a file -- with and without per-ray ranges -- and must return the points, colours and status bytes the
Python binding returns, byte for byte.  Before reset() the member returns false."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import castrays_cases as cc
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, NR = 32, 500


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(tmp_path_factory.mktemp("castrays") / "castrays")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [os.path.join(ROOT, "tests", "harness", "castrays.cpp"),
                                                                            "-L" + b.LIBDIR, "-lcpu_tsdf_hip", "-ltsdf_hip",
                                                                            "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


@pytest.fixture(scope="module", params=[False, True], ids=["sensor-range", "per-ray-range"])
def run(request, harness, tmp_path_factory):
    with_range = request.param
    vol, sc = make_volume(RES, color=True)
    vol.reset()
    fr = list(frames(sc, 3, 8))
    for i, tr, dep, col in fr:
        vol.integrateCloud(dep, col, tr)
    rng = np.random.RandomState(21)
    o1, u1 = cc.family_outside_in(rng, sc.size, NR - 100)
    o2, u2 = cc.family_inside_out(rng, sc.size, 100)
    org, u = np.ascontiguousarray(np.concatenate([o1, o2])), np.ascontiguousarray(np.concatenate([u1, u2]))
    org[7, 1] = np.nan                                        # one refused ray
    t_range = np.stack([rng.uniform(0.0, 0.1, NR), rng.uniform(0.2, 0.75, NR)], 1).astype(np.float32)
    py = vol.castRays(org, u, t_range if with_range else None, want_rgb=True)
    vol.close()
    tmp = tmp_path_factory.mktemp("castrays_io")
    inp, out = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<6q", RES, sc.width, sc.height, len(fr), NR, 1 if with_range else 0))
        f.write(struct.pack("<5d", sc.size, sc.fx, sc.fy, sc.cx, sc.cy))
        for i, tr, dep, col in fr:
            f.write(np.ascontiguousarray(tr, np.float64).tobytes())
            f.write(np.ascontiguousarray(dep, np.float32).tobytes())
            f.write(np.ascontiguousarray(col, np.uint8).tobytes())
        f.write(org.tobytes() + u.tobytes() + t_range.tobytes())
    subprocess.run([harness, inp, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    assert len(raw) == 8 * 5 + NR * (24 + 3 + 1)
    refused, ok, width, height, dense = struct.unpack_from("<5q", raw, 0)
    pts = np.frombuffer(raw, np.float32, 6 * NR, 40).reshape(NR, 6)
    rgb = np.frombuffer(raw, np.uint8, 3 * NR, 40 + 24 * NR).reshape(NR, 3)
    st = np.frombuffer(raw, np.uint8, NR, 40 + 27 * NR)
    return dict(refused=refused, ok=ok, shape=(width, height, dense), cpp=(pts, rgb, st), py=py)


def test_cpp_member_returns_the_python_bindings_bytes(run):
    out, st, rgb = run["py"]
    pts, crgb, cst = run["cpp"]
    assert run["ok"] == 1 and run["shape"] == (NR, 1, 0)
    assert 200 < (st == 1).sum() < NR and st[7] == 2 and (st == 0).sum() > 20
    assert pts.tobytes() == np.ascontiguousarray(out[:, :6]).tobytes(), "points / normals differ from the Python binding"
    assert cst.tobytes() == st.tobytes(), "status differs from the Python binding"
    assert crgb.tobytes() == rgb.tobytes(), "colours differ from the Python binding"
    assert len(np.unique(crgb[st == 1], axis=0)) > 10


def test_cast_rays_before_reset_returns_false(run):
    assert run["refused"] == 1
