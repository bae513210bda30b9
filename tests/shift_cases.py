"""What tsdf_hip_shift must leave behind, in numpy: a roll with fill over [z][y][x] arrays.  The fill values are those of a
fresh reset() (tsdf_hip_reset: d = -1, w = 0, rgb = 0, colour state 0, M = 0, nsample = 0)."""
import numpy as np

FILL_D, FILL_W, FILL_RGB, FILL_STATE = np.float32(-1.0), np.float32(0.0), np.uint8(0), 0


def _span(n, s):
    """Destination range [lo, hi) along an axis of n voxels whose source index i + s lies in the axis."""
    return max(0, -s), min(n, n - s)


def shifted(a, s, fill):
    """out[z, y, x] = a[z + sz, y + sy, x + sx] where that index lies in the grid, `fill` elsewhere; s = (sx, sy, sz).
    Trailing axes (the three bytes of rgb) ride along."""
    a = np.asarray(a)
    out = np.empty_like(a)
    out[...] = fill
    nz, ny, nx = a.shape[:3]
    (x0, x1), (y0, y1), (z0, z1) = _span(nx, s[0]), _span(ny, s[1]), _span(nz, s[2])
    if x0 < x1 and y0 < y1 and z0 < z1:
        out[z0:z1, y0:y1, x0:x1] = a[z0 + s[2]:z1 + s[2], y0 + s[1]:y1 + s[1], x0 + s[0]:x1 + s[0]]
    return out


def reset_count(shape, s):
    """Voxels of a [z][y][x] grid that shifted() fills."""
    nz, ny, nx = shape[:3]
    kept = max(0, nx - abs(s[0])) * max(0, ny - abs(s[1])) * max(0, nz - abs(s[2]))
    return nx * ny * nz - kept


def shifted_volume(d, w, rgb, s):
    """The three arrays download() returns, rolled."""
    return shifted(d, s, FILL_D), shifted(w, s, FILL_W), (shifted(rgb, s, FILL_RGB) if rgb is not None else None)
