"""GPU tier: cpu_tsdf::TSDFVolumeOctree::alignCloud / getAlignmentSystem of the C++ drop-in through tests/harness/align.cpp,
on the scene of tests/test_align_gpu.py::test_it_aligns: the harness fuses the same frames into its own volume and must
return the Python binding's out[29] and refined pose byte for byte (both front ends forward to the same C entry points; the
template additionally strips points without a finite z); both members refuse on a non-cubic setGridSize."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import align_cases as ac
from tests.common import make_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERATIONS = 8


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(tmp_path_factory.mktemp("align") / "align")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [os.path.join(ROOT, "tests", "harness", "align.cpp"), "-L" + b.LIBDIR,
                                                                            "-lcpu_tsdf_hip", "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def test_cpp_members_return_the_python_bindings_bytes(harness, tmp_path):
    vol, sc = make_volume(64)
    vol.reset()
    poses = ac.align_poses(sc)
    depths = [sc.depth(tr) for tr in poses]
    for tr, dep in zip(poses, depths):
        vol.integrateCloud(dep, None, tr)
    cloud, T_star, starts = ac.align_case(vol, sc)
    guess = starts["large"]
    want_sys = vol.alignmentSystem(cloud, guess)
    want_T, it, _ = vol.alignCloud(cloud, guess, max_iterations=ITERATIONS, min_step=0.0)
    assert it == ITERATIONS and want_sys[28] > 1000
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<6q", 64, sc.width, sc.height, len(poses), len(cloud), ITERATIONS))
        f.write(struct.pack("<5d", sc.size, sc.fx, sc.fy, sc.cx, sc.cy))
        for tr, dep in zip(poses, depths):
            f.write(np.ascontiguousarray(tr, np.float64).tobytes())
            f.write(np.ascontiguousarray(dep, np.float32).tobytes())
        f.write(np.ascontiguousarray(cloud, np.float32).tobytes())
        f.write(np.ascontiguousarray(guess, np.float64).tobytes())
    subprocess.run([harness, src, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    assert len(raw) == 29 * 8 + 8 + 16 * 8 + 8
    got_sys = np.frombuffer(raw, np.float64, 29)
    ok, = struct.unpack_from("<q", raw, 29 * 8)
    got_T = np.frombuffer(raw, np.float64, 16, 29 * 8 + 8).reshape(4, 4)
    refused, = struct.unpack_from("<q", raw, 29 * 8 + 8 + 16 * 8)
    assert got_sys.tobytes() == want_sys.tobytes(), "getAlignmentSystem differs from the Python binding"
    assert ok == 1 and got_T.tobytes() == np.ascontiguousarray(want_T).tobytes(), "alignCloud differs from the Python binding"
    assert refused == 1, "a non-cubic setGridSize was not refused"
    vol.close()
