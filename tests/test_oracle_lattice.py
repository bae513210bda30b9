"""CPU tier: the oracle against the compiled reference on the degenerate voxel values of tests/lattice_cases.py -- exact
zeros of either sign, denormals, +-1 and its neighbours, NaN, +-Inf, weights at the thresholds -- so that the GPU tier
(tests/test_lattice_gpu.py) may take the oracle as the reference's stand-in on them.  Every family at 16^3, with and
without colour, goes into the reference through a .vol file (written by the product's writer, read by the reference's own
load()) and into the oracle directly.  Bar: bit equality.

The last test needs no reference: the conditions that keep the GPU comparisons from passing on nothing, at 32^3."""
import numpy as np
import pytest

from cpu_tsdf_amd import synth
from cpu_tsdf_amd.volume import transform_cloud_with_normals
from tests import lattice_cases as L
from tests.common import assert_same_f32, write_vol_from_arrays

RES, SIZE, W, H = 16, 0.0625, 80, 60
COMPARISONS = {}


def break_uniform_octants(d, w, rgb):
    """The .vol writer stores an octant of eight bit-identical voxels as ONE coarse leaf, as the reference's own adaptive
    octree would; the reference then answers getFxn from that leaf's centre, which is its octree's behaviour and not what
    the dense comparison is about.  So the first voxel of every such octant gets another weight from the list."""
    n = 0
    for z in range(0, d.shape[0], 2):
        for y in range(0, d.shape[1], 2):
            for x in range(0, d.shape[2], 2):
                sl = (slice(z, z + 2), slice(y, y + 2), slice(x, x + 2))
                if (len(np.unique(d[sl].view(np.uint32))) == 1 and len(np.unique(w[sl])) == 1
                        and (rgb is None or len(np.unique(rgb[sl].reshape(8, 3), axis=0)) == 1)):
                    w[z, y, x] = 99 if w[z, y, x] == 100 else 100
                    n += 1
    return n


def _ref():
    from oracle import refbind
    if not refbind.available():
        pytest.skip("oracle/_ref not built (needs /root/reference: make -C oracle ref)")
    return refbind


@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("family", L.FAMILIES)
def test_oracle_equals_compiled_reference_on_lattice_values(tmp_path, family, color):
    refbind = _ref()
    p = L.params((RES,) * 3, SIZE, family, color)
    model, (d, w, rgb) = L.model_of(p, family)
    ov = model.ov
    if break_uniform_octants(d, w, rgb):
        model.upload(w=w)
    path = str(tmp_path / "lattice.vol")
    write_vol_from_arrays(path, p, d, w, rgb, chunk=8)
    ref = refbind.RefVolume(RES, SIZE, W, H, p.fx, p.fy, p.cx, p.cy, 0.0, 3 * SIZE, trunc=L.TRUNC[family], max_weight=L.MAX_WEIGHT,
                            color=color)
    ref.load(path)
    n = 0
    rd, rw, rrgb, _, _ = ref.dump_dense()
    L.assert_same_bits(rd, ov.d, "d as the reference loaded it")
    L.assert_same_bits(rw, ov.w, "w as the reference loaded it")
    n += 2
    if color:
        assert np.array_equal(rrgb, ov.rgb)
        n += 1
    for w_min, mode in L.W_MINS:
        mode = mode if (color or mode != 1) else 0
        v_ref, c_ref, _, _ = ref.march(w_min, mode)
        v, c, _ = ov.march(w_min, mode)
        assert len(v) == len(v_ref), (w_min, len(v), len(v_ref))
        assert_same_f32(v, v_ref, f"mesh at w_min {w_min}")
        if mode:
            assert np.array_equal(c, c_ref), f"mesh colours at w_min {w_min}"
        n += 1
    for k, tr in enumerate(L.poses(SIZE)):
        for ds in (1, 2):
            got, _ = ref.render_view(tr, ds)
            want = transform_cloud_with_normals(ov.raycast(tr, ds), synth.eigen_affine_inverse(tr))
            assert_same_f32(want[..., :6], got[..., :6], f"renderView pose {k} ds {ds}")
            n += 1
    pts = L.sample_points(ov)
    ok, val, grad, hess = ov.sample(pts)
    rok, rval, rgrad, rhess = ref.sample(pts)
    assert set(np.unique(rok)) <= {0, 7}
    assert np.array_equal(ok, rok == 7) and 0.3 * len(pts) < ok.sum() < 0.9 * len(pts)
    assert_same_f32(val[ok], rval[ok], "getFxn")
    assert_same_f32(grad[ok], rgrad[ok], "getGradient")
    assert_same_f32(hess[ok], rhess[ok], "getHessian")
    n += 4
    sc = synth.scene_a(RES, W, H)
    for i in range(2):
        tr = synth.turntable_pose(i, 8, sc.size)
        dep, col = sc.depth(tr), sc.bgra(i)
        ref.integrate(dep, col, tr)
        seen = model.integrate(dep, col, tr)
        assert seen > 1000
        rd, rw, rrgb, _, _ = ref.dump_dense()
        assert_same_f32(rd, ov.d, f"d after frame {i}")
        assert_same_f32(rw, ov.w, f"w after frame {i}")
        n += 2
        if color:
            assert np.array_equal(rrgb, ov.rgb), f"rgb after frame {i}"
            n += 1
    assert (ov.w == L.MAX_WEIGHT).any() and (w == 99).any()   # counts 99 and 100 crossed the saturation
    ref.close()
    COMPARISONS[(family, color)] = n
    print(f"{family} {'colour' if color else 'plain'}: {n} comparisons with the compiled reference, {sum(COMPARISONS.values())} so far")


def test_the_values_are_the_bit_patterns_they_claim():
    bits = {float(v) if np.isfinite(v) else str(v): int(b) for v, b in zip(L.VALUES, L.VALUES.view(np.uint32))}
    assert L.TINIEST.view(np.uint32) == 1 and L.TINY.view(np.uint32) == 0x000116c2 and L.ONE_DOWN.view(np.uint32) == 0x3f7fffff
    assert bits[1.0] == 0x3f800000 and bits[-1.0] == 0xbf800000
    assert sorted(L.VALUES[L.VALUES == 0].view(np.uint32).tolist()) == [0, 0x80000000]
    assert len(set(L.VALUES.view(np.uint32).tolist())) == len(L.VALUES) == 17
    d = L.with_quiet_nans(np.zeros((32, 32, 32), np.float32))
    assert np.isnan(d).sum() == 2 and sorted(d.view(np.uint32)[np.isnan(d)].tolist()) == [0x7fc00001, 0xffc00000]
    assert np.float32(L.TINY * np.float32(0.03)) < 0 or np.float32(-L.TINY * np.float32(0.03)) < 0   # survives the truncation scale
    assert np.float32(-L.TINIEST * np.float32(0.03)) == 0 and np.signbit(np.float32(-L.TINIEST * np.float32(0.03)))


@pytest.mark.parametrize("family", L.FAMILIES)
def test_conditions_of_the_gpu_comparisons(family):
    """At 32^3, from the oracle alone: the floors of tests/lattice_cases.FLOORS for the random families in both weight
    draws; for the sheets and shells a mesh, 1000 hits from the front, and -- the point of the denormal shell at truncation
    0.03 -- a mesh that differs from the one the same shell gives with normal-range values."""
    for f32w in (False, True):
        p = L.params((32,) * 3, 0.125, family, True)
        model, _ = L.model_of(p, family, f32w)
        t = L.tally(model, post=True)
        print(family, "F32W weights" if f32w else "PACKED weights", t)
        if family.startswith("random"):
            if family == "random_finite":   # no NaN or Inf among the voxels: those two floors belong to the other draw
                t = {k: v for k, v in t.items() if k not in ("nan_t_rays", "sample_nan_ok")}
            L.check_floors(t)
        else:
            assert t["triangles_w0"] > 0 and t["triangles_w2.5"] > 0
            assert t["hits_per_pose"][L.FRONT] >= 1000, t["hits_per_pose"]
    if family == "denormal_shell":
        cells = model.ov.march(0.0, 0)[2]
        model.upload(d=L.normal_shell((32,) * 3))
        normal = model.ov.march(0.0, 0)[2]
        assert len(normal) > 0 and not np.array_equal(cells, normal)
