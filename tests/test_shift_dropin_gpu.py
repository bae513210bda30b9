"""GPU tier: cpu_tsdf::TSDFVolumeOctree::shiftVolume of the C++ drop-in through tests/harness/shift.cpp: the harness fuses
the same frames into its own 64^3 volume, shifts it by (5, -3, 2) and must return the Python binding's voxels byte for byte,
moved = s * size / res in doubles exactly and the global transform G * Translation(moved) exactly; before reset() the member
returns false and leaves *moved alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import shift_cases as sc_
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = (5, -3, 2)
# a quarter turn about z and dyadic offsets: every product and sum of G * Translation(moved) is exact in doubles, so the
# comparison does not depend on the order a matrix product is summed in
G = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(tmp_path_factory.mktemp("shift") / "shift")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [os.path.join(ROOT, "tests", "harness", "shift.cpp"), "-L" + b.LIBDIR,
                                                                            "-lcpu_tsdf_hip", "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def run(harness, tmp_path_factory):
    vol, sc = make_volume(64)
    vol.reset()
    vol.setGlobalTransform(G)
    fr = [(tr, dep) for i, tr, dep, col in frames(sc, 4, 8)]
    for tr, dep in fr:
        vol.integrateCloud(dep, None, tr)
    before = vol.download()
    moved = vol.shiftVolume(*SHIFT)
    after, gt = vol.download(), vol.getGlobalTransform()
    size = float(vol._p.size[0])
    vol.close()
    tmp = tmp_path_factory.mktemp("shift_io")
    src, out = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<7q", 64, sc.width, sc.height, len(fr), *SHIFT))
        f.write(struct.pack("<5d", sc.size, sc.fx, sc.fy, sc.cx, sc.cy))
        f.write(np.ascontiguousarray(G, np.float64).tobytes())
        for tr, dep in fr:
            f.write(np.ascontiguousarray(tr, np.float64).tobytes())
            f.write(np.ascontiguousarray(dep, np.float32).tobytes())
    subprocess.run([harness, src, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    nv = 64 ** 3
    assert len(raw) == 16 + 24 + 128 + 8 * nv
    ok, refused = struct.unpack_from("<2q", raw, 0)
    return dict(ok=ok, refused=refused, moved=np.frombuffer(raw, np.float64, 3, 16), gt=np.frombuffer(raw, np.float64, 16, 40).reshape(4, 4),
                d=np.frombuffer(raw, np.float32, nv, 168).reshape(64, 64, 64), w=np.frombuffer(raw, np.float32, nv, 168 + 4 * nv).reshape(64, 64, 64),
                py_before=before, py_after=after, py_moved=moved, py_gt=gt, size=size)


def test_cpp_member_returns_the_python_bindings_bytes(run):
    r = run
    assert r["ok"] == 1
    assert (r["py_before"][1] > 0).sum() > 1000
    want = sc_.shifted_volume(r["py_before"][0], r["py_before"][1], None, SHIFT)
    assert r["py_after"][0].tobytes() == want[0].tobytes() and r["py_after"][1].tobytes() == want[1].tobytes()
    assert r["d"].tobytes() == r["py_after"][0].tobytes(), "d differs from the Python binding"
    assert r["w"].tobytes() == r["py_after"][1].tobytes(), "w differs from the Python binding"
    moved = np.array([s * r["size"] / 64 for s in SHIFT], np.float64)  # s * size / res in doubles
    assert r["moved"].tobytes() == moved.tobytes() and r["py_moved"].tobytes() == moved.tobytes()
    t = np.eye(4)
    t[:3, 3] = moved
    assert r["gt"].tobytes() == (G @ t).tobytes() and r["py_gt"].tobytes() == (G @ t).tobytes()


def test_shift_volume_before_reset_returns_false(run):
    assert run["refused"] == 1
