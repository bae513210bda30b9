// The gather kernels' view of a volume, Octree::getContainingVoxel and the per-point arithmetic of getFxn / getGradient /
// getHessian, shared by tsdf_query.hip (k_raycast, k_lookup_rgb, k_sample), tsdf_align.hip (k_align_system) and
// tsdf_merge.hip (k_merge): ONE statement of the reference's operation order, so that what tests/test_query_gpu.py pins to
// the oracle is what every caller computes.
// Compiled with -ffp-contract=off; float/double operation order follows the reference line by line.
#pragma once

#include <limits.h>
#include <math.h>

#include "tsdf_common.h"

struct GridView {
  int nx, ny, nz;        // full resolution
  int z_first, nz_alloc; // allocated plane range
  int lv[3];             // octree levels per axis (log2 res) or -1
  float size[3];
  float nsize[3];        // size the axis' node centres descend from (tsdf_node_size: size_x on an octree grid)
  float half[3];         // size/2 in float (root bounds test, octree.cpp:630)
  int64_t pitch;
  const float *d;
  PlaneView pv;          // weights (and colour) through tsdf_load_w: layout-independent
  const float *ctr[3];   // octree node-centre tables
};

static inline GridView make_view(const tsdf_hip_volume *v) {
  GridView g;
  g.nx = v->nx;
  g.ny = v->ny;
  g.nz = v->nz;
  g.z_first = v->z_first;
  g.nz_alloc = v->nz_alloc;
  for (int a = 0; a < 3; ++a) {
    g.lv[a] = v->levels[a];
    g.size[a] = v->p.size[a];
    g.nsize[a] = tsdf_node_size(v->p, a);
    g.half[a] = v->p.size[a] / 2;
    g.ctr[a] = v->ctr[a];
  }
  g.pitch = v->pitch;
  g.d = v->d;
  g.pv = tsdf_plane_view(v);
  return g;
}

// x86 cvttsd2si semantics (see tsdf_integrate.hip)
static __device__ __forceinline__ int cvtt(double v) {
  return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN;
}

// getVoxelCenter (tsdf_volume_octree.cpp:553-560), one axis: double formula rounded to float.
static __device__ __forceinline__ float voxel_center(const GridView &g, int a, int i) {
  const int res = a == 0 ? g.nx : a == 1 ? g.ny : g.nz;
  const float off = g.size[a] / 2.0;
  return (float)(((size_t)i + 0.5) * g.size[a] / (double)res - off);
}

// getVoxelIndex (tsdf_volume_octree.cpp:562-574), one axis.
static __device__ __forceinline__ int voxel_index(const GridView &g, int a, float x) {
  const int res = a == 0 ? g.nx : a == 1 ? g.ny : g.nz;
  const double off = (double)g.size[a] / 2.0;
  return cvtt(floor(((double)x + off) / (double)g.size[a] * (double)res));
}

// One axis of OctreeNode::getContainingVoxel's descent (octree.cpp:112-121): child bit = (x - ctr) > 0.
static __device__ __forceinline__ int descend_axis(float x, float size, int L) {
  float c = 0.f, s = size;
  int i = 0;
  for (int l = 0; l < L; ++l) {
    const bool b = (x - c) > 0.f;
    const float off = s / 4;
    c = b ? c + off : c - off;
    s = s / 2;
    i = i * 2 + (b ? 1 : 0);
  }
  return i;
}

static __device__ __forceinline__ int axis_index(const GridView &g, int a, float x) {
  if (g.lv[a] >= 0) return descend_axis(x, g.nsize[a], g.lv[a]);
  const int res = a == 0 ? g.nx : a == 1 ? g.ny : g.nz;
  int i = cvtt(floor(((double)x + (double)g.size[a] / 2.0) / (double)g.size[a] * (double)res));
  return i < 0 ? 0 : (i >= res ? res - 1 : i);
}

// Octree::getContainingVoxel (octree.cpp:628-643) on a fully refined tree; false == NULL.
// `local` reports whether the voxel's plane is held by this handle (always true for a whole grid).
static __device__ __forceinline__ bool containing(const GridView &g, float x, float y, float z, int64_t &vi,
                                                  bool &local, int &k) {
  local = true;
  k = -1;
  if (isnan(z) || fabsf(x) > g.half[0] || fabsf(y) > g.half[1] || fabsf(z) > g.half[2]) return false;
  const int i = axis_index(g, 0, x), j = axis_index(g, 1, y);
  k = axis_index(g, 2, z);
  const int kl = k - g.z_first;
  local = kl >= 0 && kl < g.nz_alloc;
  vi = ((int64_t)(local ? kl : 0) * g.ny + j) * g.pitch + i;
  return true;
}

// ---------------------------------------------------------------------------------------------
// getNeighbors :796-828, getFxn :655-672, getGradient :681-700, getHessian :703-726.
// Neighbour order: dx outer, dy, dz inner.  getFxn/getGradient read the octree NODE centre
// (vox->getCenter), getHessian reads getVoxelCenter (`centers[i]`).  Unqualified fabs(float) is
// double fabs(double), so every term is a double product accumulated into a float.
static __device__ __forceinline__ int sgn(float x) { return x > 0 ? 1 : -1; }  // :674-678

// One query point.  Returns what the reference's getNeighbors returns (`good`); xi, yi, zi are then the lower corner of
// the eight neighbours, all of them inside the grid and inside the planes this handle holds.  v, gr (and with HESS the
// three off-diagonal Hessian entries) are NaN where it returns false.
// A Z-slab handle answers only for points whose lower-corner plane it OWNS: halo planes are allocated but only
// as fresh as the caller's last exchange, and exactly one handle of a partition owns any plane (plane zi + 1
// may be the first halo plane: the one-plane exchange marching cubes needs as well).
template <bool HESS>
static __device__ __forceinline__ bool sample_point(const GridView &g, const int own_lo, const int own_hi, const float px,
                                                    const float py, const float pz, float &v, float gr[3], float hs[3],
                                                    int &xi, int &yi, int &zi) {
  bool good = true;
  xi = voxel_index(g, 0, px);
  yi = voxel_index(g, 1, py);
  zi = voxel_index(g, 2, pz);
  if (!(xi >= 0 && yi >= 0 && zi >= 0 && xi < g.nx && yi < g.ny && zi < g.nz)) good = false;
  if (good) {
    if (px < voxel_center(g, 0, xi)) xi -= 1;
    if (py < voxel_center(g, 1, yi)) yi -= 1;
    if (pz < voxel_center(g, 2, zi)) zi -= 1;
    if (xi < 0 || xi >= g.nx - 1 || yi < 0 || yi >= g.ny - 1 || zi < 0 || zi >= g.nz - 1) good = false;
  }
  const int kl = zi - g.z_first;
  if (good && (zi < own_lo || zi >= own_hi || kl < 0 || kl + 1 >= g.nz_alloc)) good = false;
  v = NAN;
  gr[0] = gr[1] = gr[2] = NAN;
  float h01 = NAN, h02 = NAN, h12 = NAN;
  if (good) {
    const float c = g.size[0] / g.nx;
    v = 0;
    gr[0] = gr[1] = gr[2] = 0;
    h01 = h02 = h12 = 0;
    for (int dx = 0; dx <= 1; dx++)
      for (int dy = 0; dy <= 1; dy++)
        for (int dz = 0; dz <= 1; dz++) {
          const int i = xi + dx, j = yi + dy, k = zi + dz;
          const float dv = g.d[((int64_t)(k - g.z_first) * g.ny + j) * g.pitch + i];
          const float nc[3] = {g.ctr[0][i], g.ctr[1][j], g.ctr[2][k]};
          v += (c - fabs((double)(px - nc[0]))) * (c - fabs((double)(py - nc[1]))) *
               (c - fabs((double)(pz - nc[2]))) * dv;
          gr[0] += -sgn(px - nc[0]) * (c - fabs((double)(py - nc[1]))) * (c - fabs((double)(pz - nc[2]))) * dv;
          gr[1] += (c - fabs((double)(px - nc[0]))) * -sgn(py - nc[1]) * (c - fabs((double)(pz - nc[2]))) * dv;
          gr[2] += (c - fabs((double)(px - nc[0]))) * (c - fabs((double)(py - nc[1]))) * -sgn(pz - nc[2]) * dv;
          if (HESS) {
            const float fc[3] = {voxel_center(g, 0, i), voxel_center(g, 1, j), voxel_center(g, 2, k)};
            h01 += sgn(px - fc[0]) * sgn(py - fc[1]) * (c - fabs((double)(pz - fc[2]))) * dv;
            h02 += sgn(px - fc[0]) * (c - fabs((double)(py - fc[1]))) * sgn(pz - fc[2]) * dv;
            h12 += (c - fabs((double)(px - fc[0]))) * sgn(py - fc[1]) * sgn(pz - fc[2]) * dv;
          }
        }
    const float c3 = c * c * c;
    v /= c3;
    gr[0] /= c3;
    gr[1] /= c3;
    gr[2] /= c3;
    h01 /= c3;
    h02 /= c3;
    h12 /= c3;
  }
  if (HESS) {
    hs[0] = h01;
    hs[1] = h02;
    hs[2] = h12;
  }
  return good;
}
