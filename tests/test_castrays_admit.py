"""CPU tier: the admission rule of castRays.  ray_admit (cpu_tsdf_amd/csrc/tsdf_ray_admit.h) is the function the kernels of
tsdf_castrays.hip call per ray; tests/harness/castrays_admit.cpp compiles it with g++ alone and runs it over the table of
tests/castrays_cases.py: NaN and +-inf in each of the 8 inputs, tmax = inf, ranges just below and just above the 2^24 bound
for two leaf sizes, tmax < tmin, tmax == tmin, a far ray.  Verdicts and caps must equal the rule of include/tsdf_hip.h
computed in numpy float64 -- which is what lets tests/test_castrays_gpu.py hand the kernel such rays at all."""
import os
import subprocess

import numpy as np
import pytest

from tests import castrays_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("castrays_admit")
    exe, table = str(tmp / "castrays_admit"), str(tmp / "table.txt")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "cpu_tsdf_amd", "csrc"),
                           os.path.join(ROOT, "tests", "harness", "castrays_admit.cpp"), "-o", exe])
    rows = cc.admit_table()
    with open(table, "w") as f:
        for o, u, tmin, tmax, leaf in rows:
            v = np.array(list(o) + list(u) + [tmin, tmax, leaf], np.float32)
            f.write(" ".join(f"{int(b):08x}" for b in v.view(np.uint32)) + "\n")
    out = subprocess.check_output([exe, table], text=True, timeout=60).split("\n")
    got = [tuple(int(x) for x in ln.split()) for ln in out if ln.strip()]
    assert len(got) == len(rows)
    return rows, got


def test_verdicts_and_caps_equal_the_rule(verdicts):
    rows, got = verdicts
    for row, (ok, cap) in zip(rows, got):
        want_ok, want_cap = cc.admit_rule(*row)
        assert (bool(ok), cap) == (want_ok, want_cap), (row, ok, cap, want_ok, want_cap)


def test_the_table_covers_what_it_claims(verdicts):
    rows, got = verdicts
    by = {}
    for (o, u, tmin, tmax, leaf), (ok, cap) in zip(rows, got):
        vals = np.array(list(o) + list(u) + [tmin, tmax], np.float32)
        if not np.isfinite(vals).all():
            assert (ok, cap) == (0, 0)
            by.setdefault("nonfinite", set()).add((int(np.flatnonzero(~np.isfinite(vals))[0]), str(vals[~np.isfinite(vals)][0])))
        elif tmax < tmin or tmax == tmin:
            assert (ok, cap) == (1, 16)
            by.setdefault("empty", set()).add(tmax == tmin)
        elif tmin == 1e6:
            assert ok == 1 and cap == 16 + 2 * int(np.ceil(1.0 / (np.float64(np.float32(leaf)) / 4)))
            by.setdefault("far", set()).add(leaf)
        else:
            by.setdefault("admitted" if ok else "too_long", set()).add((leaf, tmin, tmax))
            assert cap <= cc.CAP_MAX and (cap >= 16 if ok else cap == 0)
    assert len(by["nonfinite"]) == 8 * 3                      # every input, NaN / inf / -inf (tmax = inf among them)
    assert by["empty"] == {True, False} and len(by["far"]) == 2
    for leaf in (1.0 / 256, 3.3 / 64):                        # both sides of the bound, for both leaf sizes and both tmin
        assert sum(1 for r in by["admitted"] if r[0] == leaf) >= 4 and sum(1 for r in by["too_long"] if r[0] == leaf) >= 4
    caps = [cap for (_, cap) in got]
    assert max(caps) > cc.CAP_MAX - 40000 and max(caps) <= cc.CAP_MAX   # the largest admitted cap sits right under the bound
