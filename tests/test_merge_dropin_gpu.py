"""GPU tier: mergeVolume above the C ABI.  cpu_tsdf::TSDFVolumeOctree::mergeVolume of the C++ drop-in, through
tests/harness/merge.cpp, fuses the same frames into its own two 32^3 volumes and must return the Python binding's voxels byte
for byte -- once with the explicit transform, once through the two global transforms; before reset() of either volume the
member returns false.  `tsdf2mesh A.vol out.ply --merge B.vol` must write the mesh that load + mergeVolume + reconstruct give
in Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree, TSDFVolumeOctree
from tests import merge_cases as mc
from tests import sequence_util as su
from tests.common import frames, make_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 32
# quarter turns and dyadic offsets: every product, sum and inverse of these matrices is exact in doubles, so the comparison
# does not depend on how either side sums a matrix product or inverts a transform
G_DST = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 0.0, 1.0]])
D_FROM_S = np.array([[0.0, 0.0, 1.0, 2.0 ** -6], [0.0, 1.0, 0.0, -2.0 ** -7], [-1.0, 0.0, 0.0, 2.0 ** -6], [0.0, 0.0, 0.0, 1.0]])  # about y; 4, -2, 4 voxels
G_SRC = G_DST @ D_FROM_S


@pytest.fixture(scope="module")
def harness(gpu, tmp_path_factory):
    from cpu_tsdf_amd import build as b
    if not os.path.exists(b.SHELL_LIB):
        b.build_shell()
    exe = str(tmp_path_factory.mktemp("merge") / "merge")
    subprocess.check_call(["g++"] + b.HOST_FLAGS + b.host_include_flags() + [os.path.join(ROOT, "tests", "harness", "merge.cpp"), "-L" + b.LIBDIR,
                                                                            "-lcpu_tsdf_hip", "-ltsdf_hip", "-Wl,-rpath," + b.LIBDIR, "-o", exe])
    return exe


def fused_pair(color=False):
    """dst: frames 0-3; src: frames 4-7, its volume frame at D_FROM_S in dst's.  Returns (dst, src, sc, frames of dst, of src)."""
    assert np.array_equal(np.linalg.inv(G_DST) @ G_SRC, D_FROM_S)
    dst, sc = make_volume(RES, 160, 120, color=color)
    src, _ = make_volume(RES, 160, 120, color=color)
    inv = np.linalg.inv(D_FROM_S)
    fr = list(frames(sc, 8, 8))
    fa = [(tr, dep, col) for i, tr, dep, col in fr[:4]]
    fb = [(inv @ tr, dep, col) for i, tr, dep, col in fr[4:]]
    for vol, g, fs in ((dst, G_DST, fa), (src, G_SRC, fb)):
        vol.reset()
        vol.setGlobalTransform(g)
        for tr, dep, col in fs:
            vol.integrateCloud(dep, col if color else None, tr)
    return dst, src, sc, fa, fb


@pytest.fixture(scope="module")
def run(harness, tmp_path_factory):
    dst, src, sc, fa, fb = fused_pair()
    before_d, before_s = dst.download(), src.download()
    want = mc.merge_model(dst._p, before_d, src._p, before_s, D_FROM_S)
    n_explicit = dst.mergeVolume(src, D_FROM_S, count=True)
    py_explicit = dst.download()
    dst.upload(before_d[0], before_d[1])
    n_global = dst.mergeVolume(src, count=True)
    py_global = dst.download()
    dst.close()
    src.close()
    tmp = tmp_path_factory.mktemp("merge_io")
    inp, out = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<5q", RES, sc.width, sc.height, len(fa), len(fb)))
        f.write(struct.pack("<5d", sc.size, sc.fx, sc.fy, sc.cx, sc.cy))
        for m in (G_DST, G_SRC, D_FROM_S):
            f.write(np.ascontiguousarray(m, np.float64).tobytes())
        for tr, dep, col in fa + fb:
            f.write(np.ascontiguousarray(tr, np.float64).tobytes())
            f.write(np.ascontiguousarray(dep, np.float32).tobytes())
    subprocess.run([harness, inp, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    nv = RES ** 3
    assert len(raw) == 8 + 2 * (16 + 8 * nv)
    res = dict(refused=struct.unpack_from("<q", raw, 0)[0], want=want, py=[(n_explicit, py_explicit), (n_global, py_global)], cpp=[])
    for k in range(2):
        off = 8 + k * (16 + 8 * nv)
        ok, merged = struct.unpack_from("<qQ", raw, off)
        res["cpp"].append((ok, merged, np.frombuffer(raw, np.float32, nv, off + 16).reshape(RES, RES, RES),
                           np.frombuffer(raw, np.float32, nv, off + 16 + 4 * nv).reshape(RES, RES, RES)))
    return res


@pytest.mark.parametrize("k", [0, 1], ids=["explicit_transform", "global_transforms"])
def test_cpp_member_returns_the_python_bindings_bytes(run, k):
    want, (n, py), (ok, merged, d, w) = run["want"], run["py"][k], run["cpp"][k]
    assert n == int(want[3].sum()) and n > 5000
    assert py[0].tobytes() == want[0].tobytes() and py[1].tobytes() == want[1].tobytes(), "the Python binding differs from the model"
    assert ok == 1 and merged == n
    assert d.tobytes() == py[0].tobytes(), "d differs from the Python binding"
    assert w.tobytes() == py[1].tobytes(), "w differs from the Python binding"


def test_merge_volume_before_reset_returns_false(run):
    assert run["refused"] == 1


def test_tsdf2mesh_with_merge_writes_the_python_mesh(gpu, tmp_path):
    if not os.path.exists(su.OUR_TSDF2MESH):
        from cpu_tsdf_amd import build as b
        b.build_programs()
    dst, src, *_ = fused_pair()
    a_vol, b_vol, m_vol = (str(tmp_path / n) for n in ("a.vol", "b.vol", "merged.vol"))
    dst.save(a_vol)
    src.save(b_vol)
    dst.close()
    src.close()
    a, b = TSDFVolumeOctree(), TSDFVolumeOctree()
    a.load(a_vol)
    b.load(b_vol)
    assert np.array_equal(a.getGlobalTransform(), G_DST) and np.array_equal(b.getGlobalTransform(), G_SRC)
    assert a.mergeVolume(b, count=True) > 5000
    a.save(m_vol)
    mcu = MarchingCubesTSDFOctree()  # the program's settings: the class defaults, min weight 2.5, no colour
    mcu.setInputTSDF(a)
    mcu.setMinWeight(2.5)
    mesh = mcu.reconstruct()
    a.close()
    b.close()
    out, ref, plain = (str(tmp_path / n) for n in ("out.ply", "ref.ply", "plain.ply"))
    for args in ([a_vol, out, "--merge", b_vol], [m_vol, ref], [a_vol, plain]):
        rc, log = su.run(su.OUR_TSDF2MESH, args)
        assert rc == 0, log[-2000:]
    v, c, f = su.read_ply(out)
    assert len(f) > 1000 and c is None
    assert np.array_equal(v.view(np.uint32), np.asarray(mesh["vertices"], np.float32).view(np.uint32))
    assert np.array_equal(f, mesh["polygons"])
    assert open(out, "rb").read() == open(ref, "rb").read(), "--merge differs from meshing the merged volume the Python binding saved"
    assert len(su.read_ply(plain)[2]) < len(f)  # (without --merge: A's own surface only)
    rc, log = su.run(su.OUR_TSDF2MESH, [a_vol, out, "--merge", str(tmp_path / "missing.vol")])
    assert rc == 1
