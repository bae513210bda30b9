"""GPU tier: bench.py's N>1 code path, as far as one GPU allows (VERDICT r01 "Next round" #5).

(1) world size 1 on the `nccl` backend (= RCCL): communicator init, device-tensor broadcast (overlapped, two-slot
    receive buffer), all-reduce and all-gather really execute on RCCL, through the same step function the driver's
    `--gpus 8` run uses.
(2) two ranks on the one GPU over `gloo` (RCCL refuses two ranks per device): strong scaling of one grid over two
    Z-slabs, rank 1 receiving every frame by broadcast; its observed-voxel total must equal the one-rank run's.
Numbers from these runs mean nothing; the JSON contract and the counts do."""
import json
import os
import socket
import tempfile
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --full: these tests read the roofline byte counts, observed voxels, host-path rate and broadcast time, which a plain run skips
COMMON = ["--res", "256", "--steps", "4", "--warmup", "2", "--full", "--extras", "0", "--cpu-baseline", "0"]
PLAIN = ["--res", "256", "--steps", "4", "--warmup", "2"]


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def run(cmd, env_extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def check_contract(j, n_gpus):
    assert j["n_gpus"] == n_gpus and j["steps"] == 4 and j["warmup"] == 2 and j["unit"] == "Mvoxels/s"
    assert j["scaling"] == "strong" and j["higher_is_better"] is True and j["vs_baseline"] is None
    assert j["config"]["grid"] == [256, 256, 256] and j["value"] > 0
    r = j["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] <= 1 and r["achieved"] == pytest.approx(r["frac"] * r["peak"])


def test_bench_world1_on_rccl(gpu):
    single = run([sys.executable, "bench.py"] + COMMON, {})
    check_contract(single, 1)
    assert "multi_gpu" not in single
    j = run([sys.executable, "bench.py"] + COMMON, {"TSDF_BENCH_FORCE_DIST": "1", "MASTER_PORT": free_port()})
    check_contract(j, 1)
    assert j["multi_gpu"]["backend"] == "nccl" and j["multi_gpu"]["overlap"] is True
    assert len(j["multi_gpu"]["per_rank_kernel_ms"]) == 1 and j["multi_gpu"]["frame_broadcast_ms_isolated"] > 0
    assert j["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]


@pytest.mark.parametrize("overlap", [1, 0])
def test_bench_two_ranks_one_gpu_over_gloo(gpu, overlap):
    single = run([sys.executable, "bench.py"] + COMMON, {})
    j = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
             "--master-port", free_port(), "bench.py", "--gpus", "2", "--overlap", str(overlap)] + COMMON,
            {"TSDF_BENCH_ONE_DEVICE": "1", "TSDF_BENCH_BACKEND": "gloo"})
    check_contract(j, 2)
    assert j["multi_gpu"]["planes_per_gpu"] == 128 and len(j["multi_gpu"]["per_rank_kernel_ms"]) == 2
    # the diagnostics of the first run on a real node: load balance, peer access, RCCL, HBM preflight
    mg = j["multi_gpu"]
    assert len(mg["observed_voxels_per_rank"]) == 2 and sum(mg["observed_voxels_per_rank"]) == j["config"]["observed_voxels_per_frame"]
    assert mg["peer_access"][0][0] is True and mg["visible_devices"] >= 1 and mg["rccl_version"]
    assert 0 < mg["slab_hbm_gib_per_rank"] < mg["free_hbm_gib_before_create_rank0"] and mg["kernel_ms_spread"] >= 1.0
    # every voxel is observed by exactly one slab: the two ranks' counts add up to the single-handle count
    assert j["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]


def test_bench_plain_command_line_launches_its_own_ranks(gpu):
    """`python bench.py --gpus 2` with no launcher (VERDICT r02 missing #4): bench.py re-executes itself under
    torch.distributed.run, one rank per GPU, and prints ONE line with n_gpus == 2."""
    single = run([sys.executable, "bench.py"] + COMMON, {})
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", TSDF_BENCH_ONE_DEVICE="1", TSDF_BENCH_BACKEND="gloo")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + COMMON, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    check_contract(j, 2)
    assert j["multi_gpu"]["world_size"] == 2 and j["multi_gpu"]["backend"] == "gloo"
    assert len(j["multi_gpu"]["per_rank_kernel_ms"]) == 2 and j["multi_gpu"]["frame_broadcast_ms_isolated"] > 0
    assert j["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]


@pytest.mark.parametrize("n", [2, 3])
def test_bench_inprocess_host(gpu, n):
    """--host inprocess: the tsdf_hip_create_multi path the C++ drop-in uses, N slabs on the one GPU."""
    single = run([sys.executable, "bench.py"] + COMMON, {})
    j = run([sys.executable, "bench.py", "--gpus", str(n), "--host", "inprocess"] + COMMON, {"TSDF_BENCH_ONE_DEVICE": "1"})
    assert j["n_gpus"] == n and j["steps"] == 4 and j["unit"] == "Mvoxels/s" and j["value"] > 0
    assert j["config"]["parallelism"] == f"zslab{n}-inprocess" and j["config"]["grid"] == [256, 256, 256]
    mg = j["multi_gpu"]
    assert len(mg["per_slab_kernel_ms"]) == n and all(ms > 0 for ms in mg["per_slab_kernel_ms"])
    assert mg["slabs"][0]["z_begin"] == 0 and mg["slabs"][-1]["z_end"] == 256
    assert 0 < j["roofline"]["frac"] <= 1
    assert j["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]


def test_bench_single_gpu_line_carries_the_host_path_rate(gpu):
    j = run([sys.executable, "bench.py"] + COMMON, {})
    hp = j["host_path"]
    assert hp["frames_per_s_sync_calls"] > 0 and hp["frames_per_s_async_ring"] > 0 and "error" not in hp


def test_bench_dry_run_ranks_reports_the_host_cost_of_a_step(gpu):
    """`python bench.py --dry-run-ranks 4` (VERDICT r03 next #6a): the full four-rank control flow on one GPU over gloo,
    launched by bench.py itself; the line says it is a dry run and carries rank 0's host-side microseconds per step."""
    single = run([sys.executable, "bench.py"] + COMMON, {})
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "TSDF_BENCH_ONE_DEVICE", "TSDF_BENCH_BACKEND")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "bench.py", "--dry-run-ranks", "4"] + COMMON, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    check_contract(j, 4)
    assert "dry_run" in j and j["multi_gpu"]["backend"] == "gloo" and j["multi_gpu"]["planes_per_gpu"] == 64
    assert j["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]
    hu = j["host_us_per_step"]
    assert hu["integrate_calls"] > 0 and hu["event_records"] > 0 and hu["broadcast_calls"] > 0 and hu["total"] < 1e5
    assert single["host_us_per_step"]["broadcast_calls"] is None and 0 < single["host_us_per_step"]["total"] < 2000


def test_bench_pairing_one_rank_and_two_ranks(gpu):
    """`bench.py --pairing 1`: the timed frames go two per call (tsdf_hip_integrate_device2) and, with
    ranks, two per collective; the JSON contract holds, every pair was swept once on the turntable, and the observed-voxel
    counts (counted frame by frame, outside the timed region) equal the unpaired run's."""
    single = run([sys.executable, "bench.py"] + COMMON, {})
    j = run([sys.executable, "bench.py", "--pairing", "1"] + COMMON, {})
    check_contract(j, 1)
    assert j["pairing"]["pairs_launched"] == 2 and j["pairing"]["pairs_swept_once_by_every_slab"] == 2
    assert j["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]
    j2 = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", free_port(), "bench.py", "--gpus", "2", "--pairing", "1"] + COMMON,
             {"TSDF_BENCH_ONE_DEVICE": "1", "TSDF_BENCH_BACKEND": "gloo"})
    check_contract(j2, 2)
    assert j2["pairing"]["pairs_launched"] == 2
    assert j2["config"]["observed_voxels_per_frame"] == single["config"]["observed_voxels_per_frame"]


def test_bench_plain_line_and_dumped_outputs(gpu):
    """A plain run (no --full) prints the headline fields and nothing that needs a run of its own; --dump-outputs writes
    the grid the timed steps left, as float32 arrays, identical with and without --full (the dump precedes every further
    integration) and from run to run."""
    with tempfile.TemporaryDirectory() as td:
        a, b = os.path.join(td, "a"), os.path.join(td, "b")
        j = run([sys.executable, "bench.py"] + PLAIN + ["--dump-outputs", a], {})
        assert j["steps"] == 4 and j["warmup"] == 2 and j["unit"] == "Mvoxels/s" and j["higher_is_better"] is True
        assert j["dtype"] == "f32" and j["value"] > 0 and j["ms_per_step"] > 0 and j["roofline"]["kernel_ms"] > 0
        for leg in ("extras", "host_path", "cpu_baseline"):
            assert leg not in j
        assert j["config"]["observed_voxels_per_frame"] is None and "frac" not in j["roofline"]
        full = run([sys.executable, "bench.py"] + COMMON + ["--dump-outputs", b], {})
        assert full["roofline"]["frac"] > 0
        names = sorted(os.listdir(a))
        assert names == sorted(os.listdir(b)) == ["sample_voxel_zyx.npy", "tsdf_distance.npy", "tsdf_rgb.npy", "tsdf_weight.npy"]
        assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20
        for n in names:
            x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
            assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), y.view(np.uint32)), n
        w = np.load(os.path.join(a, "tsdf_weight.npy"))
        assert (w > 0).any()
