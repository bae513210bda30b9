"""GPU tier: the counting instances' counters, value for value.

A counting launch adds four sums (k_integrate2: five) to striped slots of the handle's counter array and the host adds the
stripes up again (tsdf_integrate_collect / tsdf_integrate_collect2): a slot layout that differs between the two sides
miscounts silently, and bench.py quotes bytes from these counters.  For every kernel family of tests/counter_cases.py, at
64 and at 40 rows per block, each launch's returned observation count, tsdf_hip_last_count_detail and
tsdf_hip_last_read_detail must equal tests/golden/integrate_counters.json integer for integer (the counters are sums of
integers: atomic order cannot move them).  That file was recorded from the commit named inside it, before the slot layout
got its names; so that it cannot pin a wrong number, the observation counts must also be the culled CPU oracle's."""
import functools
import json
import os

import pytest

from cpu_tsdf_amd import synth
from oracle.oracle import OracleVolume
from tests import counter_cases as cc
from tests.common import make_volume

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "integrate_counters.json")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def oracle_counts(name):
    """Observed voxels of the case's frames in order (rows per block do not enter); computed once per case."""
    color = cc.CASES[name][0]
    vol, _ = make_volume(cc.RES, cc.W, cc.H, color=color)  # (for its parameters only)
    try:
        ov = OracleVolume(vol._p)
        return tuple(ov.integrate_culled(dep, col if color else None, tr, synth.cam_from_vol_f32(tr)) for tr, dep, col in cc.sequence(name))
    finally:
        vol.close()


@functools.lru_cache(maxsize=None)
def launches(name, rows):
    """(records, blocks) of a case at `rows` rows per block: run once, shared by the two tests below."""
    return cc.run(name, rows)  # (restores every knob itself)


def test_the_golden_file_covers_every_case():
    g = golden()
    assert len(g["parent"]) == 40 and set(g["cases"]) == {f"{name} / {rows}" for name in cc.CASES for rows in cc.ROWS_PER_BLOCK}


@pytest.mark.parametrize("rows", cc.ROWS_PER_BLOCK)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_counters_equal_the_recorded_ones_and_the_oracle(gpu, name, rows):
    got, _ = launches(name, rows)
    for rec in got:
        print(name, rows, rec)
    want_n = oracle_counts(name)
    flat = [n for rec in got for n in (rec["n"] if isinstance(rec["n"], list) else [rec["n"]])]
    assert flat == list(want_n), (name, rows, flat, want_n)
    assert got == golden()["cases"][f"{name} / {rows}"], (name, rows)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_rows_per_block_reaches_the_launch(gpu, name):
    """The 64 rows of the grid are one block of a column at 64 rows per block and two at 40 (40 + 24): a launch over the whole
    grid has twice the blocks.  The LIVE launch covers the frame's index box only, whose rows are not worked out here: it
    has no fewer blocks."""
    b64, b40 = launches(name, 64)[1], launches(name, 40)[1]
    print(name, b64, b40)
    assert len(b64) == len(b40) and min(b64) > 0
    if cc.CASES[name][4]:
        assert all(n40 >= n64 for n64, n40 in zip(b64, b40)), (name, b64, b40)
    else:
        assert b40 == [2 * n for n in b64], (name, b64, b40)
