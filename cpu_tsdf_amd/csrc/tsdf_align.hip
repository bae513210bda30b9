// libtsdf_hip.so -- alignCloud: register a cloud to the fused signed distance field (NOT in the reference, which has
// getFxn / getGradient for exactly this use but leaves the optimisation to the caller, one point per call).
//
// k_align_system fuses  transform -> getFxnAndGradient -> 6-DoF normal equations  over a device-resident cloud; the
// Gauss-Newton loop around it (tsdf_hip_align) brings 29 doubles back per iteration.  The per-point arithmetic is
// sample_point (tsdf_gridview.h), the code k_sample runs: value and gradient are bit for bit what tsdf_hip_sample
// returns.  New here are a transform, a gate and a sum -- see include/tsdf_hip.h for their definition and DESIGN.md 3.14
// for the derivation of J and the summation order.
//
// Summation order (fixed: two calls return identical bytes; no floating-point atomics anywhere):
//   grid = min(ceil(n / 256), 256) blocks of 256 threads -- a function of n alone; thread t of block b takes points
//   b * 256 + t, + grid * 256, ... in that order into 29 fp64 accumulators; the 64 lanes of a wave are folded by
//   __shfl_down (32, 16, ..., 1); the four wave sums go through LDS and are added in wave order; one 29-double partial
//   per block goes to scratch; k_align_finish (one block, a launch boundary instead of a "last block" hand-off) adds the
//   block partials in block order.
// The gather is 8 distance and 8 weight loads per point, latency-bound like k_sample; no roofline claim is made.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tsdf_common.h"
#include "tsdf_gridview.h"
#include "tsdf_se3.h"

#define ALIGN_TERMS 29
#define ALIGN_BLOCK 256
#define ALIGN_MAX_BLOCKS 256

struct AlignArgs {
  float R[9], t[3];  // vol_from_src cast to float (trans.cast<float>(), hpp:76)
  float min_weight, r_max;
};

static __global__ void __launch_bounds__(ALIGN_BLOCK)
k_align_system(const GridView g, const int own_lo, const int own_hi, const AlignArgs a, const float *__restrict__ xyz,
               const size_t n, double *__restrict__ partial, unsigned char *__restrict__ used, float *__restrict__ xyz_vol) {
  double acc[ALIGN_TERMS];
#pragma unroll
  for (int k = 0; k < ALIGN_TERMS; ++k) acc[k] = 0.0;
  const size_t stride = (size_t)gridDim.x * ALIGN_BLOCK;
  for (size_t idx = (size_t)blockIdx.x * ALIGN_BLOCK + threadIdx.x; idx < n; idx += stride) {
    const float px = xyz[3 * idx], py = xyz[3 * idx + 1], pz = xyz[3 * idx + 2];
    float q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = ((a.R[3 * r] * px + a.R[3 * r + 1] * py) + a.R[3 * r + 2] * pz) + a.t[r];
    float val, gr[3], hs[3];
    int xi, yi, zi;
    bool use = sample_point<false>(g, own_lo, own_hi, q[0], q[1], q[2], val, gr, hs, xi, yi, zi);
    if (use) {  // (xi, yi, zi) .. + 1 are inside the grid and inside the planes this handle holds
      const int64_t o = ((int64_t)(zi - g.z_first) * g.ny + yi) * g.pitch + xi;
      const int64_t sy = g.pitch, sz = (int64_t)g.ny * g.pitch;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int64_t oc = o + ((c & 4) ? 1 : 0) + ((c & 2) ? sy : 0) + ((c & 1) ? sz : 0);
        use = use && (tsdf_load_w(g.pv, oc) > a.min_weight);
      }
      use = use && (fabsf(val) < a.r_max);
    }
    if (used) used[idx] = use ? 1 : 0;
    if (xyz_vol) {
      xyz_vol[3 * idx] = q[0];
      xyz_vol[3 * idx + 1] = q[1];
      xyz_vol[3 * idx + 2] = q[2];
    }
    if (use) {
      const double qx = q[0], qy = q[1], qz = q[2], gx = gr[0], gy = gr[1], gz = gr[2], r = val;
      const double J[6] = {qy * gz - qz * gy, qz * gx - qx * gz, qx * gy - qy * gx, gx, gy, gz};
      int k = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r;
      acc[27] += r * r;
      acc[28] += 1.0;
    }
  }
  // wave: lane L receives lane L + off; after the last step lane 0 holds the wave's sum
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < ALIGN_TERMS; ++k) acc[k] += __shfl_down(acc[k], off, 64);
  }
  __shared__ double wave_sum[ALIGN_BLOCK / 64][ALIGN_TERMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < ALIGN_TERMS; ++k) wave_sum[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < ALIGN_TERMS) {
    double s = wave_sum[0][threadIdx.x];
    for (int w = 1; w < ALIGN_BLOCK / 64; ++w) s += wave_sum[w][threadIdx.x];
    partial[(size_t)blockIdx.x * ALIGN_TERMS + threadIdx.x] = s;
  }
}

// out[k] = the block partials in block order
static __global__ void __launch_bounds__(64) k_align_finish(const double *__restrict__ partial, const int n_blocks, double *__restrict__ out) {
  if (threadIdx.x >= ALIGN_TERMS) return;
  double s = partial[threadIdx.x];
  for (int b = 1; b < n_blocks; ++b) s += partial[(size_t)b * ALIGN_TERMS + threadIdx.x];
  out[threadIdx.x] = s;
}

static bool align_args_ok(const void *xyz, size_t n, const double *T, float min_weight, float r_max) {
  if (!xyz || !n || !T || !(r_max > 0.f) || min_weight != min_weight) return false;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(T[i])) return false;
  return true;
}

static unsigned align_grid(size_t n) { return (unsigned)std::min<size_t>((n + ALIGN_BLOCK - 1) / ALIGN_BLOCK, ALIGN_MAX_BLOCKS); }

// doubles the two kernels need behind whatever else the caller keeps in scratch: block partials, then out
static size_t align_work_bytes() { return (size_t)(ALIGN_MAX_BLOCKS + 1) * ALIGN_TERMS * sizeof(double); }

// Both launches, asynchronous on the handle's stream, between the handle's two events; d_work holds align_work_bytes().
static int align_launch(tsdf_handle h, const float *d_xyz, size_t n, const double T[12], float min_weight, float r_max,
                        double *d_work, unsigned char *d_used, float *d_xyz_vol) {
  AlignArgs a;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a.R[3 * r + c] = (float)T[4 * r + c];
    a.t[r] = (float)T[4 * r + 3];
  }
  a.min_weight = min_weight;
  a.r_max = r_max;
  if (const int rc = h->align_ev.ensure(2)) return rc;
  const unsigned grid = align_grid(n);
  TSDF_HIP_TRY(hipEventRecord(h->align_ev[0], h->stream));
  hipLaunchKernelGGL(k_align_system, dim3(grid), dim3(ALIGN_BLOCK), 0, h->stream, make_view(h), h->z_begin, h->z_end, a, d_xyz, n,
                     d_work, d_used, d_xyz_vol);
  TSDF_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(64), 0, h->stream, (const double *)d_work, (int)grid,
                     d_work + (size_t)ALIGN_MAX_BLOCKS * ALIGN_TERMS);
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(h->align_ev[1], h->stream));
  return TSDF_HIP_OK;
}

// `out` to the host (synchronises the stream) and the device time of the two launches
static int align_collect(tsdf_handle h, const double *d_work, double out[ALIGN_TERMS], uint64_t *usec) {
  const int rc = tsdf_to_host(h, out, d_work + (size_t)ALIGN_MAX_BLOCKS * ALIGN_TERMS, ALIGN_TERMS * sizeof(double));
  if (rc) return rc;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->align_ev[0], h->align_ev[1]) == hipSuccess) *usec += (uint64_t)llround((double)ms * 1000.0);
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_align_system(tsdf_handle h, const float *xyz, size_t n, const double vol_from_src[12], float min_weight,
                                     float r_max, double out[29], uint8_t *used, float *xyz_vol) {
  if (!h || !out || !align_args_ok(xyz, n, vol_from_src, min_weight, r_max)) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_align_system(h, xyz, n, vol_from_src, min_weight, r_max, out, used, xyz_vol);
  TSDF_ENTER(h);
  // scratch layout: work doubles | xyz[3n] | xyz_vol[3n] floats | used[n] bytes
  const size_t wb = align_work_bytes();
  int rc = tsdf_ensure_scratch(h, wb + 6 * n * sizeof(float) + n + 16);
  if (rc) return rc;
  double *d_work = (double *)h->scratch.p;
  float *d_xyz = (float *)((char *)h->scratch.p + wb), *d_q = d_xyz + 3 * n;
  unsigned char *d_used = (unsigned char *)(d_q + 3 * n);
  if ((rc = tsdf_to_device(h, d_xyz, xyz, 3 * n * sizeof(float)))) return rc;
  if ((rc = align_launch(h, d_xyz, n, vol_from_src, min_weight, r_max, d_work, used ? d_used : nullptr, xyz_vol ? d_q : nullptr))) return rc;
  uint64_t usec = 0;
  if ((rc = align_collect(h, d_work, out, &usec))) return rc;
  if (used && (rc = tsdf_to_host(h, used, d_used, n))) return rc;
  if (xyz_vol && (rc = tsdf_to_host(h, xyz_vol, d_q, 3 * n * sizeof(float)))) return rc;
  h->align_stats[0] = n;
  h->align_stats[1] = (uint64_t)out[28];
  h->align_stats[2] = 0;
  h->align_stats[3] = usec;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_align_system_device(tsdf_handle h, const float *d_xyz, size_t n, const double vol_from_src[12],
                                            float min_weight, float r_max, double out[29]) {
  if (!h || !out || !align_args_ok(d_xyz, n, vol_from_src, min_weight, r_max)) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_align_system_device (a device cloud lives on one GPU; use tsdf_hip_align_system)");
  TSDF_ENTER(h);
  int rc = tsdf_ensure_scratch(h, align_work_bytes());
  if (rc) return rc;
  double *d_work = (double *)h->scratch.p;
  if ((rc = align_launch(h, d_xyz, n, vol_from_src, min_weight, r_max, d_work, nullptr, nullptr))) return rc;
  uint64_t usec = 0;
  if ((rc = align_collect(h, d_work, out, &usec))) return rc;
  h->align_stats[0] = n;
  h->align_stats[1] = (uint64_t)out[28];
  h->align_stats[2] = 0;
  h->align_stats[3] = usec;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_align(tsdf_handle h, const float *xyz, size_t n, const double guess[12], float min_weight, float r_max,
                              int max_iterations, double min_step, double refined[12], int32_t *iterations, double *cost_log) {
  if (!h || !refined || !align_args_ok(xyz, n, guess, min_weight, r_max) || max_iterations < 1 || !(min_step >= 0.0))
    return TSDF_HIP_E_INVALID;
  double T[12];
  memcpy(T, guess, sizeof T);
  memcpy(refined, guess, sizeof T);
  if (iterations) *iterations = 0;
  double *d_work = nullptr;
  float *d_xyz = nullptr;
  if (!h->multi) {  // the cloud goes up once; a set uploads per slab and iteration through tsdf_multi_align_system
    TSDF_ENTER(h);
    const size_t wb = align_work_bytes();
    int rc = tsdf_ensure_scratch(h, wb + 3 * n * sizeof(float));
    if (rc) return rc;
    d_work = (double *)h->scratch.p;
    d_xyz = (float *)((char *)h->scratch.p + wb);
    if ((rc = tsdf_to_device(h, d_xyz, xyz, 3 * n * sizeof(float)))) return rc;
  }
  uint64_t usec = 0, n_used = 0;
  int steps = 0, status = TSDF_HIP_OK;
  for (int it = 0; it < max_iterations; ++it) {
    double sys[ALIGN_TERMS];
    int rc;
    if (h->multi) {
      rc = tsdf_multi_align_system(h, xyz, n, T, min_weight, r_max, sys, nullptr, nullptr);
      usec += h->align_stats[3];
    } else {
      TSDF_ON_DEVICE(h->device);
      rc = align_launch(h, d_xyz, n, T, min_weight, r_max, d_work, nullptr, nullptr);
      if (!rc) rc = align_collect(h, d_work, sys, &usec);
    }
    if (rc) return rc;
    n_used = (uint64_t)sys[28];
    if (cost_log) {
      cost_log[2 * it] = sys[27];
      cost_log[2 * it + 1] = sys[28];
    }
    if (!(sys[28] > 0.0)) {
      tsdf_set_error("tsdf_hip_align: no point passed the gate (outside the volume, unobserved voxels, or |value| >= r_max)");
      status = TSDF_HIP_ALIGN_NO_POINTS;
      break;
    }
    double delta[6], E[12], Tn[12];
    if (tsdf_solve_step(sys, delta)) {
      tsdf_set_error("tsdf_hip_align: the normal equations are not positive definite: the used points do not constrain all six freedoms");
      status = TSDF_HIP_ALIGN_RANK_DEFICIENT;
      break;
    }
    tsdf_se3_exp(delta, E);
    tsdf_se3_mul(E, T, Tn);
    memcpy(T, Tn, sizeof T);
    ++steps;
    double s2 = 0.0;
    for (int k = 0; k < 6; ++k) s2 += delta[k] * delta[k];
    if (sqrt(s2) < min_step) break;
  }
  memcpy(refined, T, sizeof T);
  if (iterations) *iterations = steps;
  h->align_stats[0] = n;
  h->align_stats[1] = n_used;
  h->align_stats[2] = (uint64_t)steps;
  h->align_stats[3] = usec;
  return status;
}

extern "C" int tsdf_hip_align_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = h->align_stats[i];
  return TSDF_HIP_OK;
}
