"""The pose family of tests/test_oracle_poses.py and tests/test_integrate_poses_gpu.py: cameras that are rolled about the
optical axis, look along the volume's y axis, or are exactly axis-aligned.

Every other pose builder of the suite keeps `down = (0, 1, 0)`, which makes cam_from_vol[0][1] an exact zero (and, at
tilt 0, all of row 1 and column 1 equal to (0, 1, 0)): the integrate kernels' hand-written copies of
pcl::transformPoint then add exact zeros where a wrong index, a wrong summation order or a swapped pair half would show.
Here image u depends on volume y, image v on volume x and z, and three poses are signed permutation matrices (entries 0
and +-1, -0.0 products, whole voxel columns sharing one pixel column).  test_oracle_poses.py asserts this structure.

Plain module, no fixtures: CPU and GPU tests import it."""
import math
from collections import OrderedDict

import numpy as np

from cpu_tsdf_amd import synth

RADIUS_FACTOR = 2.6   # with a sensor range of RANGE_FACTOR * S every corner voxel of a 32^3 .. 96^3 Scene-A grid is inside
RANGE_FACTOR = 4.0    # the image minus the border the ALLIN proof wants, for every pose below (asserted on the CPU tier)
DEFAULT_DOWN = (0.0, 1.0, 0.0)


def specs(S, radius_factor=RADIUS_FACTOR):
    """name -> (eye, target, down), in family order."""
    r = radius_factor * S
    c = 0.577
    o = (0.0, 0.0, 0.0)
    return OrderedDict([
        ("roll30", ((r * math.sin(0.7), -0.2 * S, -r * math.cos(0.7)), o, (0.5, 0.8660254, 0.0))),
        ("roll90", ((r * math.sin(2.1), 0.15 * S, -r * math.cos(2.1)), o, (1.0, 0.0, 0.0))),
        ("roll180", ((r * math.sin(3.9), -0.1 * S, -r * math.cos(3.9)), o, (0.0, -1.0, 0.0))),
        ("roll-135", ((r * math.sin(5.0), 0.3 * S, -r * math.cos(5.0)), o, (-0.7, -0.7, 0.1))),
        ("topdown", ((0.1 * S, -r, 0.05 * S), o, (0.0, 0.0, 1.0))),
        ("frombelow_rolled", ((0.0, r, 0.0), (0.02 * S, 0.0, 0.01 * S), (0.6, 0.0, 0.8))),
        ("axis_z", ((0.0, 0.0, -r), o, DEFAULT_DOWN)),
        ("axis_x_roll90", ((r, 0.0, 0.0), o, (0.0, 0.0, 1.0))),
        ("axis_y", ((0.0, -r, 0.0), o, (1.0, 0.0, 0.0))),
        ("diag", ((r * c, -r * c, -r * c), o, (0.3, 0.9, -0.3))),
    ])


def poses(S, radius_factor=RADIUS_FACTOR):
    """Ordered dict name -> 4x4 camera -> volume pose."""
    return OrderedDict((name, synth.look_at_pose(eye, target, down)) for name, (eye, target, down) in specs(S, radius_factor).items())


def downs():
    """The family's `down` vectors, in family order."""
    return [down for _, _, down in specs(1.0).values()]


def frame(sc, i, tr):
    """Depth and colour of frame i seen from `tr`: noisy, with a comb of NaN pixels that moves from frame to frame."""
    dep = sc.depth(tr, noise_seed=40 + i)
    dep[(i * 5) % 30::31, ::3] = np.nan
    return dep, sc.bgra(i)


def roll_about_optical_axis(deg):
    """4x4 to post-multiply a camera -> volume pose with: the camera turned by `deg` about its own z axis."""
    a = math.radians(deg)
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    return m


def corners_all_inside(tr, centres, fx, fy, cx, cy, width, height, zmin, zmax):
    """The host's ALLIN proof obligation restated (the eight corner voxels in the sensor range with 1e-3 m to spare and
    in the image minus a border): `centres` = the three centre tables (x, y, z), the float cam_from_vol evaluated in
    double."""
    T = synth.cam_from_vol_f32(tr).astype(np.float64).reshape(3, 4)
    zlo = max(zmin, 0.0)
    for k in range(8):
        p = np.array([centres[0][-1 if k & 1 else 0], centres[1][-1 if k & 2 else 0], centres[2][-1 if k & 4 else 0], 1.0], np.float64)
        g = T @ p
        u, v = fx * g[0] / g[2] + cx, fy * g[1] / g[2] + cy
        if not (g[2] > zlo + 1e-3 and g[2] < zmax - 1e-3 and 1 < u < width - 2 and 1 < v < height - 2):
            return False
    return True
