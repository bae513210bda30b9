"""GPU tier: the evidence that rounds 2-4 ran by hand (profiles/*.log, tests/evidence/*.py), driver-run.

(b) fixed-seed slices of the two random hunts -- the product against the culled oracle (1-3 slab handles, both layouts,
    half the cases with the principal point pushed off centre so that the reference's frustum cull decides voxels) and the
    C++ drop-in against the COMPILED reference through the shared C driver;
(c) an API-SEQUENCE fuzz for the implied distances of DESIGN.md 3.1c: random interleavings of every entry point that writes
    voxel planes or hands them out -- integrateCloud (host and device frames, counting or not), the two-frame sweep, upload,
    set_planes_device, device_planes (raw pointers), save -> load, a plain-kernel launch, reset -- with the planes compared
    with the oracle after EVERY step and tsdf_hip_last_read_detail checked against a model of the host's record: the
    shortcut is on exactly while every writer since the reset was a flag-keeping PACKED launch, and off from the first one
    that was not until the next reset.  A writer that forgets to end the shortcut fails here on the very next step;
(d) the instance-sensitive modules once more with the ALLIN instance switched off and 16 rows per block (the environment
    knobs the product reads at first use): the general instance and another block shape carry the same results."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cpu_tsdf_amd import capi, synth
from oracle.oracle import OracleVolume
from tests.common import assert_same_f32, make_volume
from tests.sequence_model import Record, compare
from tests.test_fused2_gpu import device_frame
from tests.test_implied_d_gpu import holes, open_scene, read_detail

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_script(args, timeout=900, env_extra=None):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    p = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def test_product_vs_oracle_hunt_slice(gpu):
    rc, out, err = run_script(["tests/evidence/fuzz_product_vs_oracle.py", "--cases", "40", "--seed", "501", "--ref-cull", "0.5"])
    assert rc == 0, (out[-3000:], err[-2000:])
    assert "40 cases, seed 501: 0 with differences" in out, out[-1500:]
    assert out.count(" ok") >= 40 and "refcull" in out


def test_dropin_vs_compiled_reference_hunt_slice(gpu):
    rc, out, err = run_script(["tests/evidence/fuzz_dropin_vs_reference.py", "--cases", "20", "--seed", "502", "--ref-cull", "0.5"])
    assert rc == 0, (out[-3000:], err[-2000:])
    assert "20 cases, seed 502: 0 with differences" in out, out[-1500:]


@pytest.mark.parametrize("seed", range(12))
def test_api_sequences_keep_the_implied_distance_record_right(gpu, seed, tmp_path):
    rng = np.random.RandomState(7000 + seed)
    color = bool(rng.randint(2))
    wmax = float(rng.choice([100.0, 4.0, 2.5, 255.0]))              # 2.5: a non-integer limit -- the shortcut never applies
    trunc = [(0.03, 0.03), (0.03, 0.03), (0.05, 0.02), (0.01, 0.03)][rng.randint(4)]   # 0.01 / 0.03: the hinge identity fails
    layout = capi.LAYOUT_F32W if rng.rand() < 0.15 else capi.LAYOUT_AUTO
    res = int(rng.choice([32, 64]))   # (powers of two: the .vol format of the save -> load step needs an octree)
    vol, sc = make_volume(res, color=color, max_weight=wmax, trunc=trunc)
    vol.setLayout(layout)
    sc = open_scene(sc)
    vol.reset()
    packed = vol.getLayout() == capi.LAYOUT_PACKED
    p = np.float32(trunc[0]) / np.float32(trunc[1])
    kmax = int(np.ceil(wmax))
    fixed = wmax == np.floor(wmax) and all(np.float32(np.float32(p * np.float32(min(k, wmax))) + p) / np.float32(min(k, wmax) + 1) == p
                                           for k in range(kmax + 1))
    rec = Record(packed, fixed, kmax)
    ov = OracleVolume(vol._p)
    lib = capi.load()
    n_frames = 40
    frame_no = [0]
    keep = []

    def next_frame():
        i = frame_no[0]
        frame_no[0] += 1
        tr = synth.turntable_pose(i % n_frames, n_frames, sc.size, tilt=0.2 * np.sin(i))
        return i, tr, holes(sc.depth(tr, noise_seed=900 + i), i), sc.bgra(i)

    took_shortcut = refused = 0
    for step in range(20):
        op = rng.choice(["integrate", "integrate", "integrate", "device", "pair", "upload", "set_planes", "device_planes",
                         "save_load", "plain", "reset", "mesh"])
        what = f"seed {seed} step {step} {op}"
        if op in ("integrate", "device"):
            i, tr, dep, col = next_frame()
            want = ov.integrate(dep, col if color else None, synth.cam_from_vol_f32(tr))
            count = bool(rng.randint(2))
            if op == "integrate":
                n = vol.integrateCloud(dep, col if color else None, tr, count=count, pipelined=bool(rng.randint(2)) and not count)
            else:
                t = device_frame(dep, col if color else None)
                keep.append(t)
                n = vol.integrateCloudDevice(t[0].data_ptr(), t[1].data_ptr() if color else 0, tr, count=count)
            if count:
                assert n == want, what
            vol.synchronize()
            allowed = rec.fast_launch()
            skipped, on = read_detail(vol)
            assert on == int(allowed), (what, on, allowed, rec.__dict__)
            if count:
                assert (skipped > 0) == allowed or (allowed and want == 0), (what, skipped)
            took_shortcut += int(allowed)
            refused += int(not allowed)
        elif op == "pair":
            pair, want = [], []
            for _ in range(2):
                i, tr, dep, col = next_frame()
                t = device_frame(dep, col if color else None)
                keep.append(t)
                pair.append((t[0].data_ptr(), t[1].data_ptr() if color else 0, tr))
                want.append(ov.integrate(dep, col if color else None, synth.cam_from_vol_f32(tr)))
            fused, counts = vol.integrateCloudDevice2(pair[0], pair[1], count=True)
            assert counts == want, what
            if fused:   # one sweep: keeps the flags and the record, reads every distance itself
                rec.fast_launch()
                assert read_detail(vol) == (0, 0), what
            else:       # two ordinary launches
                rec.fast_launch()
                allowed = rec.fast_launch()
                assert read_detail(vol)[1] == int(allowed), what
        elif op == "upload":
            d, w, rgb = vol.download()
            free = np.argwhere((w > 0) & (d == d.max()))
            if len(free):  # a free-space voxel moved off the hinge value where no flag is set: only reading it can tell
                z, y, x = free[rng.randint(len(free))]
                d[z, y, x] = ov.d[z, y, x] = np.float32(0.25)
            vol.upload(d=d, w=w, rgb=rgb)
            rec.foreign_write()
        elif op == "set_planes":
            z0, nz = int(rng.randint(res - 4)), int(rng.randint(1, 4))
            dev = torch.device("cuda", 0)
            dt = torch.empty((nz, res, res), dtype=torch.float32, device=dev)
            wt = torch.empty_like(dt)
            ct = torch.empty((nz, res, res), dtype=torch.int32, device=dev) if color else None
            args = (C.c_void_p(dt.data_ptr()), C.c_void_p(wt.data_ptr()), C.c_void_p(ct.data_ptr()) if color else None)
            capi.check(lib.tsdf_hip_get_planes_device(vol._need(), z0, nz, *args), "get_planes_device")
            vol.synchronize()
            sel = (wt > 0) & (dt == float(p))
            if bool(sel.any()):
                idx = torch.nonzero(sel)[0]
                dt[idx[0], idx[1], idx[2]] = -0.5
                ov.d[z0 + int(idx[0]), int(idx[1]), int(idx[2])] = np.float32(-0.5)
            torch.cuda.synchronize()
            capi.check(lib.tsdf_hip_set_planes_device(vol._need(), z0, nz, *args), "set_planes_device")
            rec.foreign_write()
        elif op == "device_planes":
            vol.device_planes()   # raw pointers handed out: the caller may write through them
            rec.foreign_write()
        elif op == "save_load":
            path = str(tmp_path / f"s{seed}_{step}.vol")
            vol.save(path)
            vol.load(path)
            rec.reset()
            rec.foreign_write()   # a loaded volume holds whatever the file held
        elif op == "plain":
            i, tr, dep, col = next_frame()
            ov.integrate(dep, col if color else None, synth.cam_from_vol_f32(tr))
            try:
                capi.set_tuning("plain_kernel", 1)
                vol.integrateCloud(dep, col if color else None, tr)
                vol.synchronize()
            finally:
                capi.set_tuning("plain_kernel", 0)
            if packed:   # the knob only reaches float-weight volumes (launch_integrate): a PACKED one takes the usual kernel
                assert read_detail(vol)[1] == int(rec.fast_launch()), what
            else:
                rec.foreign_write()   # the plain kernels keep no flags
                assert read_detail(vol)[1] == 0, what
        elif op == "reset":
            vol.reset()
            ov = OracleVolume(vol._p)
            rec.reset()
        elif op == "mesh":   # the flags' other reader
            from cpu_tsdf_amd.volume import MarchingCubesTSDFOctree
            mc = MarchingCubesTSDFOctree()
            mc.setInputTSDF(vol)
            mc.setMinWeight(1.0)
            mc.setColorByRGB(color)
            m = mc.reconstruct(want_cells=True)
            verts, rgb, cells = ov.march(1.0, 1 if color else 0)
            assert np.array_equal(m["cells"], cells), what
            assert_same_f32(m["vertices"], verts, f"mesh {what}")
        compare(vol, ov, what)
    vol.close()
    # every sequence exercises at least one side of the switch; over the twelve seeds both sides occur many times (checked by
    # the asserts above whenever they do)
    assert took_shortcut + refused > 0


def test_instance_sensitive_modules_under_the_general_instance_knobs(gpu):
    """The product reads TSDF_HIP_* at first use; the suite's own invariance tests go through the test library's set_tuning.
    Here the modules whose results depend most on WHICH kernel instance runs are run once more in a process whose environment
    switches the ALLIN instance off and halves the block height."""
    rc, out, err = run_script(["-m", "pytest", "tests/test_integrate_gpu.py", "tests/test_implied_d_gpu.py", "tests/test_dropin_gpu.py",
                               "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                               "--deselect", "tests/test_integrate_gpu.py::test_every_reachable_k_integrate_instance_equals_the_oracle"],
                              timeout=1200, env_extra={"TSDF_HIP_ALLIN": "0", "TSDF_HIP_ROWS_PER_BLOCK": "16"})
    tail = out[-1500:]
    assert rc == 0, (tail, err[-1500:])
    assert " passed" in tail and "failed" not in tail
