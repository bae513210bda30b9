"""The host model of reintegrateCloud (tsdf_hip_reintegrate; the definition: include/tsdf_hip.h) and what its
tests share.  The definition is a composition, and so is the model: tests/deintegrate_cases.remove_frame under the old
pose, then OracleVolume.integrate under the new pose with the new pose's reference planes.  No projection code is restated.

Plain module, no fixtures: CPU and GPU tests import it."""
import numpy as np

from cpu_tsdf_amd import synth
from tests import deintegrate_cases as dc


def correction(S):
    """The pose correction of the tests, 4 x 4: T . R_y(1.5 deg) . R_z(0.8 deg) with T a translation by
    (0.04, -0.013, 0.021) . S, S the scene size -- about 1.3 voxels of a 32^3 grid.  The corrected pose of a frame is
    correction(S) @ old."""
    a, b = np.deg2rad(1.5), np.deg2rad(0.8)
    ry = np.eye(4)
    ry[0, 0], ry[0, 2], ry[2, 0], ry[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    rz = np.eye(4)
    rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = np.cos(b), -np.sin(b), np.sin(b), np.cos(b)
    t = np.eye(4)
    t[:3, 3] = (0.04 * S, -0.013 * S, 0.021 * S)
    return t @ ry @ rz


def reintegrate_frame(ov, depth, bgra, old, new, cull=True, z_begin=0, z_end=0):
    """reintegrateCloud on an OracleVolume: (selected_old, lowered, cleared, observed_new, both).  A pose that is None
    selects nothing (what the product does with a pose that is not finite)."""
    col = bgra if ov.rgb is not None else None
    st, sel_old = (0, 0, 0), None
    if old is not None:
        sel_old = dc.observation(ov.p, depth, col, old, cull, z_begin, z_end)[0]
        st = dc.remove_frame(ov, depth, col, old, cull, z_begin, z_end)
    n, both = 0, 0
    if new is not None:
        planes = ov.reference_cull_planes(new) if cull else None
        n = ov.integrate(depth, col, synth.cam_from_vol_f32(new), z_begin, z_end, planes=planes)
        if sel_old is not None:
            both = int((sel_old & dc.observation(ov.p, depth, col, new, cull, z_begin, z_end)[0]).sum())
    return st + (n, both)


class ReposeModel(dc.RemovalModel):
    """tests/sequence_model.Model plus the removal and the re-pose."""

    def reintegrate(self, depth, bgra, old, new):
        """`old`, `new`: the poses as handed to the product (Model.pose applied by the caller)."""
        return reintegrate_frame(self.ov, depth, bgra, old, new, cull=self.cull)


def repose_sets(params, depth, bgra, old, new, w_before):
    """Of one re-pose: (both, only_old, only_new, cleared by the removal and observed again) voxel counts.  w_before: the
    weights before the call."""
    so = dc.observation(params, depth, bgra, old)[0]
    sn = dc.observation(params, depth, bgra, new)[0]
    return int((so & sn).sum()), int((so & ~sn).sum()), int((~so & sn).sum()), int((so & (w_before == 1) & sn).sum())


def quiet_cells(off):
    """[z][y][x] mask of the voxels in 64 x 4 x 1 flag cells of a 64^3 grid that hold no voxel of `off`."""
    return ~np.repeat(off.reshape(64, 16, 4 * 64).any(axis=2), 4, axis=1)[:, :, None] & np.ones(off.shape, bool)


def flag_facts(model_ov, params, depth, bgra, old, new, p):
    """The 64^3 flag case before a re-pose: (in-band additions in cells that no earlier launch and not the removal half
    can have flagged, resting voxels selected by both poses at exactly p on both sides)."""
    pb = np.float32(p).view(np.uint32)
    so, do, _ = dc.observation(params, depth, bgra, old)
    sn, dn, _ = dc.observation(params, depth, bgra, new)
    quiet = quiet_cells((model_ov.w > 0) & (model_ov.d != p))
    rem_band = so & (model_ov.w != 0) & (do.view(np.uint32) != pb)
    add_band = sn & (dn.view(np.uint32) != pb)
    only_add = quiet & quiet_cells(rem_band)   # ... and that the removal half does not flag either
    resting = so & sn & (model_ov.d == p) & (do == p) & (dn == p)
    return int((add_band & only_add).sum()), int(resting.sum())
