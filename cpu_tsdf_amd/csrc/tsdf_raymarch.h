// Internal: ONE statement of renderView's ray loop (tsdf_volume_octree.cpp:290-421), shared by the pixel rays of
// tsdf_query.hip (k_raycast, renderView) and the rays from memory of tsdf_castrays.hip (k_cast_rays, castRays).  What
// tests/test_query_gpu.py pins to the oracle is what both compute: the two kernels differ in where a ray's direction,
// origin and range come from (a ray source) and in whether an integer trip cap stands in the loop conditions.
// Compiled with -ffp-contract=off; float/double operation order follows the reference line by line.
#pragma once

#include <limits.h>
#include <math.h>

#include "tsdf_common.h"
#include "tsdf_gridview.h"
#include "tsdf_ray_admit.h"

// interpolateTrilinearly (tsdf_volume_octree.cpp:486-541).  *valid is only ever AND-ed, as in the
// reference.  `local` is cleared if a corner plane is not held by this handle.
static __device__ float trilinear(const GridView &g, float x, float y, float z, bool &valid, bool &local) {
  int xi = voxel_index(g, 0, x), yi = voxel_index(g, 1, y), zi = voxel_index(g, 2, z);
  const bool exists = xi >= 0 && yi >= 0 && zi >= 0 && xi < g.nx && yi < g.ny && zi < g.nz;
  if (!exists || xi <= 0 || xi >= g.nx - 1 || yi <= 0 || yi >= g.ny - 1 || zi <= 0 || zi >= g.nz - 1) {
    valid = false;
    return NAN;
  }
  float vx = voxel_center(g, 0, xi), vy = voxel_center(g, 1, yi), vz = voxel_center(g, 2, zi);
  if (x < vx) xi -= 1;
  if (y < vy) yi -= 1;
  if (z < vz) zi -= 1;
  vx = voxel_center(g, 0, xi);
  vy = voxel_center(g, 1, yi);
  vz = voxel_center(g, 2, zi);
  const float a = (x - vx) * g.nx / g.size[0];
  const float b = (y - vy) * g.ny / g.size[1];
  const float c = (z - vz) * g.nz / g.size[2];
  const int kl = zi - g.z_first;
  if (kl < 0 || kl + 1 >= g.nz_alloc) {
    local = false;
    valid = false;
    return NAN;
  }
  const int64_t o = ((int64_t)kl * g.ny + yi) * g.pitch + xi;
  const int64_t sy = g.pitch, sz = (int64_t)g.ny * g.pitch;
  const int64_t ox = o + 1, oy = o + sy, oz = o + sz, oxy = o + sy + 1, oxz = o + sz + 1, oyz = o + sz + sy,
                oxyz = o + sz + sy + 1;
  valid = valid && (tsdf_load_w(g.pv, o) > 0);
  valid = valid && (tsdf_load_w(g.pv, ox) > 0);
  valid = valid && (tsdf_load_w(g.pv, oy) > 0);
  valid = valid && (tsdf_load_w(g.pv, oz) > 0);
  valid = valid && (tsdf_load_w(g.pv, oxy) > 0);
  valid = valid && (tsdf_load_w(g.pv, oxz) > 0);
  valid = valid && (tsdf_load_w(g.pv, oyz) > 0);
  valid = valid && (tsdf_load_w(g.pv, oxyz) > 0);
  return (g.d[o] * (1 - a) * (1 - b) * (1 - c) + g.d[oz] * (1 - a) * (1 - b) * (c) +
          g.d[oy] * (1 - a) * (b) * (1 - c) + g.d[oyz] * (1 - a) * (b) * (c) +
          g.d[ox] * (a) * (1 - b) * (1 - c) + g.d[oxz] * (a) * (1 - b) * (c) + g.d[oxy] * (a) * (b) * (1 - c) +
          g.d[oxyz] * (a) * (b) * (c));
}

// Eigen::Vector3f::normalize() [Eigen-recall 3.3]: z = x*x + (y*y + z*z); if (z > 0) v /= sqrt(z)
static __device__ __forceinline__ void normalize3(float v[3]) {
  const float n2 = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]);
  if (n2 > 0.f) {
    const float n = sqrtf(n2);
    v[0] /= n;
    v[1] /= n;
    v[2] /= n;
  }
}

struct RayArgs {
  float rot[9], org[3];
  double nfx, nfy, ncx, ncy;
  int nw, nh;
  float zmin, zmax, neg;
  float min_step;     // max_dist_neg_ * 3/4.           (:289)
  float refine_step;  // (zsize_/zres_)/2.              (:329)
  float leaf;         // finest leaf size_ (size_x halved L times; getMinSize/getSize, octree.cpp:58-78)
  int to_camera;      // apply the final transformPointCloudWithNormals(trans^-1) (:422) in the kernel
  double inv[12];     // rows of trans.inverse().matrix(), computed by the caller's Eigen
};

// The constants of a view of handle h (host).  E_INVALID when the downsampled image has no pixel; the handle's constants
// (neg, min_step, refine_step, leaf, zmin, zmax) are filled in either way.
static inline int make_ray_args(tsdf_handle h, const float rot[9], const float origin[3], int downsample, RayArgs &a) {
  const tsdf_params &p = h->p;
  a.to_camera = 0;
  for (int i = 0; i < 12; ++i) a.inv[i] = 0;
  for (int i = 0; i < 9; ++i) a.rot[i] = rot[i];
  for (int i = 0; i < 3; ++i) a.org[i] = origin[i];
  a.nw = p.image_width / downsample;
  a.nh = p.image_height / downsample;
  a.nfx = p.fx / downsample;
  a.nfy = p.fy / downsample;
  a.ncx = p.cx / downsample;
  a.ncy = p.cy / downsample;
  a.zmin = p.min_sensor_dist;
  a.zmax = p.max_sensor_dist;
  a.neg = p.max_dist_neg;
  a.min_step = p.max_dist_neg * 3 / 4.;
  a.refine_step = (p.size[2] / p.res[2]) / 2.;
  {
    float s = p.size[0];
    if (h->levels[0] >= 0)
      for (int l = 0; l < h->levels[0]; ++l) s = s / 2;
    else
      s = p.size[0] / p.res[0];
    a.leaf = s;
  }
  return (int64_t)a.nw * a.nh > 0 ? TSDF_HIP_OK : TSDF_HIP_E_INVALID;
}

// Ray hand-off between Z-slab handles (multi-GPU renderView).  A ray's step sequence depends on the last
// voxel it visited, so slabs cannot march it independently; instead the ray's loop state travels.  One
// record per ray, TSDF_HIP_RAY_RECORD_INTS 32-bit words:
//   [0] status: 0 untouched (only in a delta buffer), 1 suspended, 2 finished
//   [1] need_z: global plane of the voxel the main loop needs next (-1: none yet)
//   [2] niter  [3] hit_voxel  [4] t  [5..7] pt  [8] last_d  [9] last_w  [10] step  [11] pixel index
//   [12] finish flag: the main loop is done, word 4 holds t_star, only the normal is left  [13..15] zero
//   [16..23] the 8 output floats (valid when finished)
// k_raycast<true> resumes every suspended ray this handle is responsible for -- need_z inside its OWNED
// planes [z_begin, z_end), or ray index % world == rank while the ray has not needed a voxel yet -- and
// marches it until it finishes or its main loop reaches a voxel of another slab.  The refinement walk
// (:326-356) and the final trilinear samples read up to `halo` planes beyond the owned range; a read
// outside the allocated planes sets `incomplete` (the caller then asks for a larger halo).
struct RaySlab {
  int rank, world, z_begin, z_end;
  int list_count;  // > 0: state/delta are ONE compact list of that many records, ray id in word 11, updated in place
};
#define RAY_REC TSDF_HIP_RAY_RECORD_INTS

// Ray sources: what ray_march reads of its ray -- du (the direction as the loop uses it), org, zmin, zmax -- and the trip
// cap.  A pixel ray (renderView) has none: its loop ends through float progress of t alone, as the reference's does, and
// at_cap folds to false at compile time.  A ray from memory (castRays) carries the cap ray_admit gave it.
struct PixelRay {
  float du[3], org[3];
  float zmin, zmax;
  __device__ __forceinline__ bool at_cap(unsigned) const { return false; }
};
struct MemoryRay {
  float du[3], org[3];
  float zmin, zmax;
  unsigned cap;
  __device__ __forceinline__ bool at_cap(unsigned trips) const { return trips >= cap; }
};

#define RAY_MISS 0
#define RAY_HIT 1      // a crossing was found (the point may still be NaN: a degenerate crossing)
#define RAY_CAPPED 3   // the trip cap ended the ray: written as a miss, t and iterations as they stood
#define RAY_PARKED -1  // RESUMABLE only: not this handle's ray, or suspended for another slab; nothing was written to `o`

// renderView, tsdf_volume_octree.cpp:290-421, one ray.  The while loop runs until every lane of the wavefront has left it
// (the hardware's exec-mask loop is the ballot); a finished lane idles.
// o: the ray's 8 output floats: x,y,z, nx,ny,nz, t (t_star on a hit), iterations; `incomplete` counts rays that touched a
// plane this handle does not hold (only possible for Z-slab handles; may be NULL where the handle holds the whole grid).
// RESUMABLE: see RaySlab above; `o` is unused, the loop state comes from `state` + RAY_REC * slot and results go to the
// ray's record in `delta`; i is the ray's index (ownership before the first voxel).
// `trips` counts main-loop and refinement-walk iterations together and stands in the condition of both loops through
// src.at_cap; `niter` stays the reference's count (main loop only).
template <bool RESUMABLE, typename Src>
static __device__ __forceinline__ int ray_march(const GridView &g, const RayArgs &a, const Src &src, const int64_t i, const int64_t slot,
                                                float *__restrict__ o, unsigned *__restrict__ incomplete,
                                                const int *__restrict__ state, int *__restrict__ delta, const RaySlab &rs) {
  bool found_crossing = false, all_local = true, finish_only = false, capped = false;
  const float *du = src.du;
  float pt[3] = {src.org[0], src.org[1], src.org[2]};
  float dd = 0, ww = 0, last_w = 0, last_d = 0;
  float t = src.zmin;
  float step = a.min_step;
  bool hit_voxel = false;
  int niter = 0;
  unsigned trips = 0;
  if (RESUMABLE) {
    const int *r = state + RAY_REC * slot;
    if (r[0] != 1) return RAY_PARKED;
    const int need_z = r[1];
    const bool mine = need_z < 0 ? (int)(i % rs.world) == rs.rank : (need_z >= rs.z_begin && need_z < rs.z_end);
    if (!mine) return RAY_PARKED;
    niter = r[2];
    hit_voxel = r[3] != 0;
    t = __int_as_float(r[4]);
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] = __int_as_float(r[5 + k]);
    last_d = __int_as_float(r[8]);
    last_w = __int_as_float(r[9]);
    step = __int_as_float(r[10]);
    finish_only = r[12] != 0;  // the main loop is done; only the normal at t_star (= t) is left, see below
    found_crossing = finish_only;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] += t * du[k];
  }
  int suspend_z = -1;
  while (!finish_only && t < src.zmax && !(capped = src.at_cap(trips))) {
    int64_t vi;
    bool local;
    int kz;
    if (containing(g, pt[0], pt[1], pt[2], vi, local, kz)) {
      if (RESUMABLE && (kz < rs.z_begin || kz >= rs.z_end)) {  // another slab's voxel: hand the ray over
        suspend_z = kz;
        break;
      }
      all_local = all_local && local;
      hit_voxel = true;
      dd = local ? g.d[vi] : -1.f;
      ww = local ? tsdf_load_w(g.pv, vi) : 0.f;
      if (((dd < 0 && last_d > 0) || (dd > 0 && last_d < 0)) && last_w && ww) {
        found_crossing = true;
        const float old_t = t - step;
        step = a.refine_step;
        float last_new_d = dd, last_new_w = ww;
        while (t >= old_t && !(capped = src.at_cap(trips))) {
          ++trips;
          t -= step;
#pragma unroll
          for (int k = 0; k < 3; ++k) pt[k] -= step * du[k];
          if (!containing(g, pt[0], pt[1], pt[2], vi, local, kz)) break;
          all_local = all_local && local;
          const float new_d = local ? g.d[vi] : -1.f, new_w = local ? tsdf_load_w(g.pv, vi) : 0.f;
          if ((last_d > 0 && new_d > 0) || (last_d < 0 && new_d < 0)) {
            last_d = new_d;
            last_w = new_w;
            dd = last_new_d;
            ww = last_new_w;
            t += step;
#pragma unroll
            for (int k = 0; k < 3; ++k) pt[k] += step * du[k];
            break;
          }
          last_new_d = dd;  // sic (:352-353)
          last_new_w = ww;
        }
        break;
      }
      last_d = dd;
      last_w = ww;
      const float s1 = a.leaf / 4.f, s2 = fabsf(dd) * a.neg;  // :360 (the double product rounds to this)
      step = s1 < s2 ? s2 : s1;
    } else if (hit_voxel) {
      break;
    }
    t += step;
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] += step * du[k];
    niter++;
    ++trips;
  }
  if (capped) found_crossing = false;  // (never with a PixelRay)
  int *rec = RESUMABLE ? delta + RAY_REC * slot : nullptr;
  if (RESUMABLE) {
    rec[1] = suspend_z;
    rec[2] = niter;
    rec[3] = hit_voxel ? 1 : 0;
    rec[4] = __float_as_int(t);
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[5 + k] = __float_as_int(pt[k]);
    rec[8] = __float_as_int(last_d);
    rec[9] = __float_as_int(last_w);
    rec[10] = __float_as_int(step);
    rec[12] = 0;
    rec[0] = suspend_z >= 0 ? 1 : 2;
    if (suspend_z >= 0) return RAY_PARKED;
    o = reinterpret_cast<float *>(rec + 16);
  }
  o[3] = o[4] = o[5] = 0.f;
  o[6] = t;
  o[7] = (float)niter;
  if (!found_crossing) {
    o[0] = o[1] = o[2] = NAN;
  } else {
    float t_star = t;  // finish_only: the record carries t_star in the t word
    if (!finish_only) {
      bool has_data = true;
      const float tcurr = t, tprev = t - step;
      last_d = trilinear(g, src.org[0] + tprev * du[0], src.org[1] + tprev * du[1], src.org[2] + tprev * du[2], has_data,
                         all_local);
      dd = trilinear(g, src.org[0] + tcurr * du[0], src.org[1] + tcurr * du[1], src.org[2] + tcurr * du[2], has_data,
                     all_local);
      // :389  evaluated in double: unqualified fabs(float) is double fabs(double) under <cmath>
      t_star = (float)((double)t + (double)step * (-1 + fabs((double)(last_d / (last_d - dd)))));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = src.org[k] + t_star * du[k];
    o[6] = t_star;
    int64_t vi;
    bool local;
    int kz;
    if (!containing(g, o[0], o[1], o[2], vi, local, kz)) {
      o[3] = o[4] = o[5] = NAN;
    } else if (RESUMABLE && !finish_only &&
               ((kz - 2 < g.z_first && g.z_first > 0) || (kz + 2 >= g.z_first + g.nz_alloc && g.z_first + g.nz_alloc < g.nz))) {
      // t_star extrapolates from two trilinear samples and can land ANY distance ahead when they are nearly equal,
      // so the six samples of the normal (planes kz-2 .. kz+2) may not be held here.  The ray then travels once
      // more: suspended for the owner of the hit point's plane with the finish flag and t_star in the t word; that
      // rank recomputes o = org + t_star * du (the same arithmetic) and the normal.
      rec[0] = 1;
      rec[1] = kz;
      rec[4] = __float_as_int(t_star);
      rec[12] = 1;
      if (!all_local && incomplete) atomicAdd(incomplete, 1u);
      return RAY_PARKED;
    } else {
      const float s = a.leaf;
      bool valid = true;
      const float d_xm = trilinear(g, o[0] - s, o[1], o[2], valid, all_local);
      const float d_xp = trilinear(g, o[0] + s, o[1], o[2], valid, all_local);
      const float d_ym = trilinear(g, o[0], o[1] - s, o[2], valid, all_local);
      const float d_yp = trilinear(g, o[0], o[1] + s, o[2], valid, all_local);
      const float d_zm = trilinear(g, o[0], o[1], o[2] - s, valid, all_local);
      const float d_zp = trilinear(g, o[0], o[1], o[2] + s, valid, all_local);
      if (!valid) {
        o[3] = o[4] = o[5] = NAN;
      } else {
        float dF[3];
        dF[0] = (d_xp - d_xm) * a.neg / (2 * s);
        dF[1] = (d_yp - d_ym) * a.neg / (2 * s);
        dF[2] = (d_zp - d_zm) * a.neg / (2 * s);
        normalize3(dF);
        o[3] = dF[0];
        o[4] = dF[1];
        o[5] = dF[2];
      }
    }
  }
  // :422 pcl::transformPointCloudWithNormals(*cloud, *cloud, trans.inverse()) [PCL-recall: Transformer<double>,
  // se3 for the point, so3 for the normal, each x*c0 + (y*c1 + (z*c2 (+ c3))) in double, cast to float; the cloud
  // is not dense, so points with a non-finite coordinate are left untouched]
  if (!RESUMABLE && a.to_camera && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2])) {
    const double px = o[0], py = o[1], pz = o[2], nx = o[3], ny = o[4], nz = o[5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      o[r] = (float)(px * a.inv[4 * r] + (py * a.inv[4 * r + 1] + (pz * a.inv[4 * r + 2] + a.inv[4 * r + 3])));
      o[3 + r] = (float)(nx * a.inv[4 * r] + (ny * a.inv[4 * r + 1] + nz * a.inv[4 * r + 2]));
    }
  }
  if (!all_local && incomplete) atomicAdd(incomplete, 1u);
  return capped ? RAY_CAPPED : found_crossing ? RAY_HIT : RAY_MISS;
}

// renderColoredView's per-hit lookup (tsdf_volume_octree.cpp:443-448): octree_->getContainingVoxel(v) then voxel->getRGB.
// false where the reference gets NULL (or the plane is not held / not OWNED by this handle: halo planes may be stale, and
// exactly one handle of a partition owns any plane); c = r | g << 8 | b << 16, 0 when not found or without a colour plane.
static __device__ __forceinline__ bool lookup_rgb_at(const GridView &g, const int own_lo, const int own_hi, float x, float y, float z,
                                                     uint32_t &c) {
  int64_t vi;
  bool local;
  int k;
  const bool hit = containing(g, x, y, z, vi, local, k) && local && k >= own_lo && k < own_hi;
  c = 0u;
  if (hit && g.pv.rgb) c = tsdf_load_rgb(g.pv, vi);
  return hit;
}
