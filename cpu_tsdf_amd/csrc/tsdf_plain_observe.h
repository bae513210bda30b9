// The per-voxel half of updateVoxel that the plain kernels share (tsdf_integrate.hip: k_integrate_plain, k_integrate_rgbn,
// k_integrate_lab; tsdf_deintegrate.hip: k_deintegrate; tsdf_reintegrate.hip: k_reintegrate): the kernel arguments of an
// integrate launch, the exact projection, the reference's frustum cull, "does this voxel reach addObservation, and with
// what" (plain_observe_at; plain_observe for the thread's own voxel) and the observation count (plain_count).  One copy, so that a frame taken out of the volume selects exactly the voxels it was put into.
// Internal; translation units that include it are compiled with -ffp-contract=off like the rest.
#pragma once

#include "tsdf_common.h"
#include "tsdf_div.h"

struct IntegrateArgs {
  float m[12];        // cam_from_vol, row-major 3x4
  float fxf, fyf, cxf, cyf;  // the same, rounded to float (fast projection path); cxf/cyf carry the +band shift
  float hb_u, hb_v;          // certificate threshold: fract(R~) > 2 * band
  float hb_max;              // max(hb_u, hb_v): the ALLIN instance certifies a quad with ONE compare of min(fract) against it
  unsigned kcap, kinc;       // PACKED count after an observation, byte 3 of a word: min(k, kcap) + kinc == min(k + 1, kmax)
  int hinge_fixed;           // PACKED: (p*w + p)/(w + 1) == p for every stored weight w, p = pos_over_neg (host-checked)
  int neg_in_window;         // max_dist_pos/neg inside the scale-free divider's window
  unsigned kmax;             // PACKED layout: saturation count ceil(max_weight)
  int wmax_is_int;           // PACKED layout: max_weight is an integer (then every stored weight is)
  float zmin, zmax;   // min/max_sensor_dist_
  float zlo;          // gz > zlo  <=>  !(gz < zmin) && gz > 0  (see make_args)
  float pos, neg;     // max_dist_pos_/neg_
  float wmax;         // max_weight_
  float pos_over_neg; // max_dist_pos_ / max_dist_neg_ (IEEE fp32, host)
  int W, H;
  int ny;             // rows this launch may touch (counted from the launch's first row)
  int plane_rows;     // rows of a whole plane: the address stride between planes
  int qpr;            // quads per row = ceil(nx/4) (counted from the launch's first quad)
  int z_global0;      // global z of the first integrated plane
  int zl0;            // allocated-plane index of the first integrated plane
  int log2TX, TX, TY; // thread tile: TX quads along x, TY rows along y (TX*TY == 256)
  int rpb;            // row groups (of TY rows) per block
  int expf_fused_r;      // the host libm's expf fuses r = InvLn2N * x - k (tsdf_expf_glibc; probed by tsdf_hip_set_weighting)
  int ref_cull;          // replicate the reference's frustum cull (getFrustumCulledVoxels): six plane tests per voxel centre
  float cull[24];        // its planes l, r, t, b, far, near (tsdf_hip_set_reference_cull), 4 floats each
  int band_fx, band_fy;  // "band seen" flags: cells of 64 x 4 x 1 voxels, [allocated plane][fy][fx] (tsdf_common.h)
  int implied_d;         // PACKED: in a cell whose flag is still 0 a voxel's distance follows from its count (see k_integrate)
  int x_abs0, y_abs0;    // grid x / y of the launch's first voxel / row (the launch may be a sub-box of the slab)
  int zfast;             // the hardware grid is (planes, row groups, x chunks) instead of (x chunks, row groups, planes): see tsdf_block_coords
  int64_t pitch;
};

// reprojectPoint (tsdf_volume_octree.cpp:611-617), EXACT: u = (int)(x*fx/z + cx) evaluated in double,
// truncation toward zero, for a voxel that already passed the range test (g.z > 0, finite).
// u and v divide by the same g.z, so the fp64 reciprocal is refined once (tsdf_div.h).
// v_cvt_i32_f64 saturates where x86's cvttsd2si returns INT_MIN; both land outside [0, W), and NaN
// cannot occur (the host rejects non-finite / absurd poses before launching).
static __device__ __forceinline__ int project_exact(const IntegrateArgs &a, const double *__restrict__ cam,
                                                    float gx, float gy, float gz) {
  // [phase: exact fp64 re-projection (rare: uncertified voxels)]
  const Rcp64 rz = rcp64_prepare((double)gz);
  const int u = (int)(div64((double)gx * cam[0], rz) + cam[2]);  // cam = fx, fy, cx, cy
  const int v = (int)(div64((double)gy * cam[1], rz) + cam[3]);
  const bool in = (unsigned)u < (unsigned)a.W && (unsigned)v < (unsigned)a.H;
  return in ? v * a.W + u : -1;
}

// pcl::FrustumCulling's verdict on a voxel centre (tsdf_volume_octree.cpp:619-652 -> filters/impl/frustum_culling.hpp
// [PCL-recall]): `pt.dot(plane) <= 0` for all six planes, pt = (x, y, z, 1) as Vector4f, the 4-term dot reduced as
// (p0 + p1) + (p2 + p3) [Eigen-recall]; no FMA (this file is built with -ffp-contract=off).  A NaN coordinate fails.
static __device__ __forceinline__ bool reference_cull_keeps(const IntegrateArgs &a, float x, float y, float z) {
  bool keep = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float *pl = a.cull + 4 * k;
    keep = keep && ((x * pl[0] + y * pl[1]) + (z * pl[2] + 1.0f * pl[3]) <= 0.f);
  }
  return keep;
}

// The counting instances' counters: per quantity a stripe of slots in the handle's counter array, a block adding to the slot of its
// number; the host sums each stripe.
enum {  // one frame: k_integrate, k_integrate_p -> tsdf_integrate_collect
  TSDF_CNT_STRIPE = 1024,
  TSDF_CNT_OBSERVED = 0,    // voxels brought to addObservation (all k_integrate_plain counts: TSDF_CNT_STRIPE slots)
  TSDF_CNT_CHANGED = 1024,  // bytes of voxel words whose VALUE changed: what any layout-preserving kernel has to write
  TSDF_CNT_IMPLIED = 2048,  // observed voxels whose distance word was not read
  TSDF_CNT_READ = 3072,     // bytes of the voxel planes the launch requested, observed voxel or not
  TSDF_CNT_SLOTS = 4096
};

struct PlainObs {
  int pix;     // the pixel the voxel projects to
  float z;     // its raw depth (weight_by_depth_ needs it)
  float dn;    // the hinged, normalised distance handed to addObservation
  int64_t vi;  // the voxel's index in the planes
};

// Does the voxel (x, y) of the launch's plane zl reach addObservation?  If so, *o says with what.
template <int ORDER>
static __device__ __forceinline__ bool plain_observe_at(const IntegrateArgs &a, const double *__restrict__ cam,
                                                        const float *__restrict__ ctrx, const float *__restrict__ ctry,
                                                        const float *__restrict__ ctrz, const float *__restrict__ depth,
                                                        const int x, const int y, const int zl, PlainObs *o) {
  if (!(x < (int)a.pitch)) return false;  // the x centre table is NaN beyond nx: those lanes fail the range test
  const float cx = ctrx[x], cy = ctry[y], cz = ctrz[a.z_global0 + zl];
  float g[3];
#pragma unroll
  for (int q = 0; q < 3; ++q)  // pcl::transformPoint (hpp:145) in the summation order of this PCL build
    g[q] = ORDER == TSDF_XFORM_PCL_SSE ? cx * a.m[4 * q] + (cy * a.m[4 * q + 1] + (cz * a.m[4 * q + 2] + a.m[4 * q + 3]))
                                       : ((a.m[4 * q] * cx + a.m[4 * q + 1] * cy) + a.m[4 * q + 2] * cz) + a.m[4 * q + 3];
  const bool in = !(g[2] < a.zmin || g[2] > a.zmax) && g[2] > 0.f &&  // hpp:146, .cpp:616
                  (!a.ref_cull || reference_cull_keeps(a, cx, cy, cz));  // hpp:93-94 (replication mode)
  o->pix = in ? project_exact(a, cam, g[0], g[1], g[2]) : -1;
  if (o->pix < 0) return false;
  o->z = depth[o->pix];
  const float dn = o->z - g[2];  // hpp:159
  if (isnan(o->z) || dn < -a.neg) return false;  // hpp:152, :193-196
  o->dn = dn > a.pos ? a.pos_over_neg : dn / a.neg;  // hpp:189-198
  o->vi = ((int64_t)(a.zl0 + zl) * a.plane_rows + y) * a.pitch + x;
  return true;
}

// ... this thread's voxel, in the grid of the plain family: (x blocks of 256, rows, planes)
template <int ORDER>
static __device__ __forceinline__ bool plain_observe(const IntegrateArgs &a, const double *__restrict__ cam,
                                                     const float *__restrict__ ctrx, const float *__restrict__ ctry,
                                                     const float *__restrict__ ctrz, const float *__restrict__ depth, PlainObs *o) {
  const int x = (int)(blockIdx.x * 256u + threadIdx.x);
  const int y = (int)blockIdx.y, zl = (int)blockIdx.z;
  return plain_observe_at<ORDER>(a, cam, ctrx, ctry, ctrz, depth, x, y, zl, o);
}

// n_obs (NULL: no count): 1024 striped counters of the voxels that reached addObservation, one atomic per wave
static __device__ __forceinline__ void plain_count(bool observed, unsigned long long *__restrict__ n_obs) {
  if (!n_obs) return;
  const unsigned long long m = __ballot(observed);
  if ((threadIdx.x & 63u) == 0u && m)
    atomicAdd(n_obs + TSDF_CNT_OBSERVED + ((blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y) & (TSDF_CNT_STRIPE - 1u)),
              (unsigned long long)__popcll(m));
}

// Host (tsdf_integrate.hip): the arguments of a plain-family launch over the handle's own planes for the pose T -- what
// tsdf_integrate_launch hands launch_plain_family, with the reference cull switched on only where its planes can bite --
// and the number of planes (the grid's z extent).  False: the pose is not finite, nothing is to be launched.
bool tsdf_plain_launch_args(tsdf_handle h, const float T[12], IntegrateArgs *a, unsigned *planes);
// Host (tsdf_integrate.hip): the implied-distance record (rest_state, rest_bits) as a flag-keeping integrate launch with
// these arguments updates it; `flags_kept`: the launch maintains the "band seen" flags.
int tsdf_plain_implied_distances(tsdf_handle h, const IntegrateArgs &a, bool flags_kept);
