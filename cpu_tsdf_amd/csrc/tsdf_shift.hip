// libtsdf_hip.so -- shift the volume's window by whole voxels, in place (tsdf_hip_shift; not in the reference, whose octree
// has a fixed root like this grid).
//
// After tsdf_hip_shift(h, (sx, sy, sz)) voxel (x, y, z) holds what (x + sx, y + sy, z + sz) held, or the reset state where
// that index lies outside the grid.  Every array of a voxel (d, w | count byte, rgb, the float colour state, M / nsample) is
// independent of the others, so ONE kernel template on the element (4-byte word, 1-byte count) runs per array.  There is no
// second copy of the volume: the hazard -- a block overwriting a voxel another block has yet to read -- is kept away by the
// decomposition:
//   sz != 0            destination planes are taken in batches of |sz| consecutive planes, one launch each.  The batch
//                      [z, z + |sz|) reads the planes [z + sz, z + sz + |sz|), which are disjoint from it, and the batches go
//                      in ascending z for sz > 0 (descending for sz < 0): every source plane is read by an EARLIER launch on
//                      the stream than the one that overwrites it.
//   sz == 0, sy != 0   the same with batches of |sy| rows, each launch doing its rows of all planes.
//   sz == sy == 0      a row moves within itself: one workgroup owns a row, loads a chunk of it into registers, barriers and
//                      stores; the chunks go in ascending x for sx > 0 (descending for sx < 0), so a chunk's sources have not
//                      been written by the chunks before it.
// An sx that comes with a y or z shift rides along in those copies.  No launch reads a location another workgroup of the same
// launch writes.  The pitch padding (x >= nx) is written with the reset value, as tsdf_hip_reset leaves it.
//
// The "band seen" flags (one byte per 64 x 4 x 1 cell) move with the data: the new flag of a cell is the OR of the old flags
// of the up to four cells its source voxels lay in (k_shift_band, from a copy of the old flags), so band_exact survives.
// HBM-bound copies: no LDS, no MFMA.
#include <string.h>

#include <algorithm>

#include "tsdf_common.h"

template <typename T>
struct alignas(4 * sizeof(T)) ShiftQuad {
  T v[4];
};

struct ShiftArgs {
  int nx, ny, nzl;  // voxels per row, rows per plane, allocated planes (sources outside [0, nzl) are outside the grid)
  int64_t pitch;
  int sx, sy, sz;
  int z0, z1, y0, y1;  // destination planes / rows of this launch (local plane indices)
};

// four destination voxels x .. x + 3 of a row whose source row is `src` (row_ok: that row exists)
template <typename T>
static __device__ __forceinline__ ShiftQuad<T> shift_load(const T *src, bool row_ok, int x, int sx, int nx, T fill) {
  ShiftQuad<T> q;
  const int xs = x + sx;
  if (row_ok && (sx & 3) == 0 && xs >= 0 && xs + 3 < nx && x + 3 < nx) {
    q = *reinterpret_cast<const ShiftQuad<T> *>(src + xs);  // rows start on a quad boundary (pitch % 4 == 0)
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xj = xs + j;
      q.v[j] = row_ok && x + j < nx && xj >= 0 && xj < nx ? src[xj] : fill;
    }
  }
  return q;
}

// Rows [y0, y1) of planes [z0, z1) <- rows (y + sy) of planes (z + sz), x shifted by sx.  The host picks the batch so that
// the source rows are not among the destination rows of the launch.  blockIdx.y strides over the rows, x over a row's quads.
template <typename T>
static __global__ void __launch_bounds__(256)
k_shift_copy(const ShiftArgs a, T *p, T fill) {
  const int nyb = a.y1 - a.y0;
  const int64_t rows = (int64_t)(a.z1 - a.z0) * nyb;
  const int qpr = (int)(a.pitch >> 2);
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const int zr = (int)(r / nyb);
    const int z = a.z0 + zr, y = a.y0 + (int)(r - (int64_t)zr * nyb);
    const int zs = z + a.sz, ys = y + a.sy;
    const bool row_ok = zs >= 0 && zs < a.nzl && ys >= 0 && ys < a.ny;
    T *dst = p + ((int64_t)z * a.ny + y) * a.pitch;
    const T *src = row_ok ? p + ((int64_t)zs * a.ny + ys) * a.pitch : p;
    for (int q = (int)(blockIdx.x * blockDim.x + threadIdx.x); q < qpr; q += (int)(gridDim.x * blockDim.x))
      *reinterpret_cast<ShiftQuad<T> *>(dst + 4 * q) = shift_load(src, row_ok, 4 * q, a.sx, a.nx, fill);
  }
}

// sz == sy == 0: every row moves within itself.  A workgroup owns a row at a time and walks it in chunks of 256 x
// SHIFT_U quads: load the chunk's sources into registers, barrier, store.  Ascending chunks for sx > 0 read ahead of
// everything written so far, descending chunks for sx < 0 behind it.
#define SHIFT_U 4
template <typename T>
static __global__ void __launch_bounds__(256)
k_shift_inrow(T *p, int64_t rows, int64_t pitch, int nx, int sx, T fill) {
  const int qpr = (int)(pitch >> 2), per = 256 * SHIFT_U, nch = (qpr + per - 1) / per;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    T *row = p + r * pitch;
    for (int i = 0; i < nch; ++i) {
      const int c = sx > 0 ? i : nch - 1 - i;
      ShiftQuad<T> v[SHIFT_U];
#pragma unroll
      for (int u = 0; u < SHIFT_U; ++u) {
        const int q = c * per + u * 256 + (int)threadIdx.x;
        if (q < qpr) v[u] = shift_load(row, true, 4 * q, sx, nx, fill);
      }
      __syncthreads();  // every source of the chunk is in registers before any of its destinations is written
#pragma unroll
      for (int u = 0; u < SHIFT_U; ++u) {
        const int q = c * per + u * 256 + (int)threadIdx.x;
        if (q < qpr) *reinterpret_cast<ShiftQuad<T> *>(row + 4 * q) = v[u];
      }
    }
  }
}

// New flag of cell (cx, cy, z) = OR of the old flags of the cells that held the cell's voxels: plane z + sz, the x range
// [64 cx + sx, 64 cx + 63 + sx] and the y range [4 cy + sy, 4 cy + 3 + sy], each clipped to the grid (0 where nothing is
// left).  A superset of the exact flags: a set flag only makes the readers look.
static __global__ void __launch_bounds__(256)
k_shift_band(const uint8_t *__restrict__ old_f, uint8_t *__restrict__ new_f, int fx, int fy, int nzl, int nx, int ny, int sx, int sy, int sz) {
  const int64_t n = (int64_t)fx * fy * nzl;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int cx = (int)(i % fx);
    const int64_t r = i / fx;
    const int cy = (int)(r % fy), z = (int)(r / fy);
    const int zs = z + sz;
    const int xl = max(64 * cx + sx, 0), xh = min(min(64 * cx + 63, nx - 1) + sx, nx - 1);
    const int yl = max(4 * cy + sy, 0), yh = min(min(4 * cy + 3, ny - 1) + sy, ny - 1);
    uint8_t f = 0;
    if (zs >= 0 && zs < nzl && xl <= xh && yl <= yh)
      for (int gy = yl >> 2; gy <= (yh >> 2); ++gy)
        for (int gx = xl >> 6; gx <= (xh >> 6); ++gx) f |= old_f[((int64_t)zs * fy + gy) * fx + gx];
    new_f[i] = f ? (uint8_t)1 : (uint8_t)0;
  }
}

template <typename T>
static int shift_array(tsdf_hip_volume *v, T *p, T fill, int sx, int sy, int sz, int dz0, int dz1) {
  if (!p || dz0 >= dz1) return TSDF_HIP_OK;
  const int qpr = (int)(v->pitch >> 2);
  if (!sz && !sy) {
    const int64_t rows = (int64_t)(dz1 - dz0) * v->ny;
    const unsigned grid = (unsigned)std::min<int64_t>(rows, 256 * 32);
    hipLaunchKernelGGL(k_shift_inrow<T>, dim3(grid), dim3(256), 0, v->stream, p + (int64_t)dz0 * v->ny * v->pitch, rows, v->pitch, v->nx, sx, fill);
    TSDF_HIP_TRY(hipGetLastError());
    return TSDF_HIP_OK;
  }
  ShiftArgs a;
  a.nx = v->nx, a.ny = v->ny, a.nzl = v->nz_alloc, a.pitch = v->pitch;
  a.sx = sx, a.sy = sy, a.sz = sz;
  const unsigned gx = (unsigned)((qpr + 255) / 256);
  auto launch = [&](int z0, int z1, int y0, int y1) -> int {
    a.z0 = z0, a.z1 = z1, a.y0 = y0, a.y1 = y1;
    const int64_t rows = (int64_t)(z1 - z0) * (y1 - y0);
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, 256 * 32 / gx));
    hipLaunchKernelGGL(k_shift_copy<T>, dim3(gx, gy), dim3(256), 0, v->stream, a, p, fill);
    TSDF_HIP_TRY(hipGetLastError());
    return TSDF_HIP_OK;
  };
  if (sz) {  // batches of |sz| planes, in the direction of the shift
    const int b = std::abs(sz), nb = (dz1 - dz0 + b - 1) / b;
    for (int i = 0; i < nb; ++i) {
      const int z0 = sz > 0 ? dz0 + i * b : std::max(dz0, dz1 - (i + 1) * b);
      const int z1 = sz > 0 ? std::min(dz1, z0 + b) : dz1 - i * b;
      if (const int rc = launch(z0, z1, 0, v->ny)) return rc;
    }
    return TSDF_HIP_OK;
  }
  const int b = std::abs(sy), nb = (v->ny + b - 1) / b;  // batches of |sy| rows of every plane
  for (int i = 0; i < nb; ++i) {
    const int y0 = sy > 0 ? i * b : std::max(0, v->ny - (i + 1) * b);
    const int y1 = sy > 0 ? std::min(v->ny, y0 + b) : v->ny - i * b;
    if (const int rc = launch(dz0, dz1, y0, y1)) return rc;
  }
  return TSDF_HIP_OK;
}

// Every voxel array of the allocated planes [dz0, dz1) (local indices) <- the voxels at (+sx, +sy, +sz); a source outside the
// allocated planes or the grid gives the reset state.  Asynchronous on the handle's stream; the band flags are not touched.
int tsdf_shift_planes(tsdf_hip_volume *v, int sx, int sy, int sz, int dz0, int dz1) {
  const float minus_one = -1.f;
  uint32_t bits;
  memcpy(&bits, &minus_one, 4);
  int rc = shift_array(v, reinterpret_cast<uint32_t *>(v->d), bits, sx, sy, sz, dz0, dz1);
  uint32_t *words[8] = {reinterpret_cast<uint32_t *>(v->w),     v->rgb,
                        reinterpret_cast<uint32_t *>(v->cn[0]), reinterpret_cast<uint32_t *>(v->cn[1]),
                        reinterpret_cast<uint32_t *>(v->cn[2]), reinterpret_cast<uint32_t *>(v->cn[3]),
                        reinterpret_cast<uint32_t *>(v->vm),    reinterpret_cast<uint32_t *>(v->vn)};
  for (int k = 0; k < 8 && !rc; ++k) rc = shift_array(v, words[k], 0u, sx, sy, sz, dz0, dz1);
  if (!rc) rc = shift_array(v, v->k8, (uint8_t)0, sx, sy, sz, dz0, dz1);
  return rc;
}

// The flags of all allocated planes follow the data (only while they describe the planes).
int tsdf_shift_band(tsdf_hip_volume *v, int sx, int sy, int sz) {
  if (!v->band_exact || !v->band) return TSDF_HIP_OK;
  const size_t n = (size_t)v->band_fx * v->band_fy * v->nz_alloc;
  if (const int rc = tsdf_ensure_scratch(v, n)) return rc;
  TSDF_HIP_TRY(hipMemcpyAsync(v->scratch.p, v->band, n, hipMemcpyDeviceToDevice, v->stream));
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 256 * 8));
  hipLaunchKernelGGL(k_shift_band, dim3(grid), dim3(256), 0, v->stream, (const uint8_t *)v->scratch.p, v->band, v->band_fx, v->band_fy,
                     v->nz_alloc, v->nx, v->ny, sx, sy, sz);
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

int tsdf_shift_mark(tsdf_hip_volume *v, int which) {
  if (const int rc = v->shift_ev.ensure(2)) return rc;
  TSDF_HIP_TRY(hipEventRecord(v->shift_ev[which], v->stream));
  v->shift_timed = true;
  return TSDF_HIP_OK;
}

void tsdf_shift_clamp(const tsdf_hip_volume *v, const int32_t shift[3], int s[3]) {
  const int n[3] = {v->nx, v->ny, v->nz};
  for (int a = 0; a < 3; ++a) s[a] = std::max(-n[a], std::min(n[a], (int)shift[a]));
}

void tsdf_shift_count(int nx, int ny, int nz, const int s[3], uint64_t *kept, uint64_t *reset) {
  const uint64_t k = (uint64_t)std::max(0, nx - std::abs(s[0])) * (uint64_t)std::max(0, ny - std::abs(s[1])) *
                     (uint64_t)std::max(0, nz - std::abs(s[2]));
  *kept = k;
  *reset = (uint64_t)nx * ny * nz - k;
}

extern "C" int tsdf_hip_shift(tsdf_handle h, const int32_t shift[3]) {
  if (!h || !shift) return TSDF_HIP_E_INVALID;
  if (!shift[0] && !shift[1] && !shift[2]) return TSDF_HIP_OK;
  if (h->multi) return tsdf_multi_shift(h, shift);
  int s[3];
  tsdf_shift_clamp(h, shift, s);
  if (s[2] && (h->z_first != 0 || h->nz_alloc != h->nz)) {
    tsdf_set_error("tsdf_hip_shift: this handle owns part of the grid (z_begin / z_end); it can shift along x and y only");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  TSDF_ENTER(h);
  int rc = tsdf_shift_mark(h, 0);
  const bool carried = h->band_exact;
  if (!rc) rc = tsdf_shift_planes(h, s[0], s[1], s[2], 0, h->nz_alloc);
  if (!rc) rc = tsdf_shift_band(h, s[0], s[1], s[2]);
  if (!rc) rc = tsdf_shift_mark(h, 1);
  tsdf_occupied_invalidate(h);  // its list names the voxels by their old indices
  tsdf_esdf_invalidate(h);      // and so does the box of a distance field
  if (rc) {
    h->band_exact = false;
    return rc;
  }
  tsdf_shift_count(h->nx, h->ny, h->nz_alloc, s, &h->shift_stats[0], &h->shift_stats[1]);
  h->shift_stats[2] = carried ? 1u : 0u;
  return TSDF_HIP_OK;
}

// microseconds between the handle's two marks; waits for the second
int tsdf_shift_elapsed_us(tsdf_hip_volume *v, uint64_t *us) {
  *us = 0;
  if (!v->shift_timed) return TSDF_HIP_OK;
  TSDF_ON_DEVICE(v->device);
  TSDF_HIP_TRY(hipEventSynchronize(v->shift_ev[1]));
  float ms = 0.f;
  TSDF_HIP_TRY(hipEventElapsedTime(&ms, v->shift_ev[0], v->shift_ev[1]));
  *us = (uint64_t)(ms * 1000.f);
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_shift_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  out[0] = h->shift_stats[0], out[1] = h->shift_stats[1], out[2] = h->shift_stats[2], out[3] = 0;
  if (h->multi) {  // the slowest slab
    for (int k = 0; k < tsdf_hip_slab_count(h); ++k) {
      uint64_t us = 0;
      if (const int rc = tsdf_shift_elapsed_us(tsdf_multi_slab(h, k), &us)) return rc;
      out[3] = std::max(out[3], us);
    }
    return TSDF_HIP_OK;
  }
  return tsdf_shift_elapsed_us(h, &out[3]);
}
