// libtsdf_hip.so -- castRays (not in the reference): arbitrary rays into the fused volume, one lane per ray.
//
// tsdf_hip_cast_rays / _device / _stats (include/tsdf_hip.h states the definition).  A ray's 8 output floats are what
// k_raycast<false> (tsdf_query.hip, renderView) writes for a pixel whose rotated direction equals the ray's: both kernels
// run ray_march (tsdf_raymarch.h), the one statement of the reference's loop (tsdf_volume_octree.cpp:290-421).  What is
// new here: the ray comes from memory (6 floats, + 2 when ranges are passed), ray_admit (tsdf_ray_admit.h) decides whether
// it is marched at all and gives it an integer trip cap, the hit's colour is read in the same pass (lookup_rgb_at, the
// lookup of tsdf_hip_lookup_rgb), and hits / ended rays are counted with one integer atomic per wave.
// The rays are marched in the caller's order, ray i by lane i.  An ordered path -- a Morton key of the ray's entry cell and
// direction octant, a radix sort, the march through the permutation -- was built and measured (DESIGN.md 3.23,
// profiles/castrays_timing.json): on 307 200 rays it did not beat the given order even when that order was a random
// permutation, and cost 0.05-0.07 ms for the keys and the sort, so it was deleted; TSDF_HIP_RAYS_AS_GIVEN is accepted and
// changes nothing.
// Gather/latency-bound like k_raycast; no roofline claim is made.  Compiled with -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include "tsdf_common.h"
#include "tsdf_gridview.h"
#include "tsdf_raymarch.h"

struct CastRays {
  const float *org, *dir, *t_range;  // n x 3, n x 3, n x 2 or NULL
  float zmin, zmax;                  // the range of every ray when t_range == NULL
  unsigned n;
};

static __device__ __forceinline__ void cast_load(const CastRays &r, unsigned i, float o[3], float u[3], float &tmin, float &tmax) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = r.org[3 * (size_t)i + k];
    u[k] = r.dir[3 * (size_t)i + k];
  }
  tmin = r.t_range ? r.t_range[2 * (size_t)i] : r.zmin;
  tmax = r.t_range ? r.t_range[2 * (size_t)i + 1] : r.zmax;
}

// One lane per ray.  status: 0 miss, 1 hit (finite xyz), 2 not admitted, 3 stopped by the trip cap.  count: hits in the low
// word, rays ended with status 2 or 3 in the high word -- one 64-bit integer atomic per wave (ballot + popcount; n < 2^31).
static __global__ void __launch_bounds__(256)
k_cast_rays(const GridView g, const RayArgs a, const CastRays r, float *__restrict__ out, uint8_t *__restrict__ rgb,
            uint8_t *__restrict__ status, unsigned long long *__restrict__ count) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < r.n;
  int st = RAY_MISS;
  if (live) {
    MemoryRay src;
    cast_load(r, i, src.org, src.du, src.zmin, src.zmax);
    float *o = out + 8 * (size_t)i;
    uint32_t c = 0u;
    if (!ray_admit(src.org, src.du, src.zmin, src.zmax, a.leaf, &src.cap)) {
      st = 2;
      o[0] = o[1] = o[2] = NAN;
      o[3] = o[4] = o[5] = 0.f;
      o[6] = src.zmin;
      o[7] = 0.f;
    } else {
      st = ray_march<false>(g, a, src, (int64_t)i, (int64_t)i, o, (unsigned *)nullptr, (const int *)nullptr, (int *)nullptr,
                            RaySlab{0, 1, 0, 0, 0});
      if (st == RAY_HIT) {
        if (isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2])) {
          if (rgb) (void)lookup_rgb_at(g, 0, g.nz, o[0], o[1], o[2], c);
        } else {
          st = RAY_MISS;  // a degenerate crossing (t* not finite): the point is NaN, as renderView leaves it
        }
      }
    }
    if (rgb) {
      rgb[3 * (size_t)i] = (uint8_t)(c & 255u);
      rgb[3 * (size_t)i + 1] = (uint8_t)((c >> 8) & 255u);
      rgb[3 * (size_t)i + 2] = (uint8_t)((c >> 16) & 255u);
    }
    if (status) status[i] = (uint8_t)st;
  }
  const unsigned long long hits = __ballot(live && st == RAY_HIT), ended = __ballot(live && st >= 2);
  if ((threadIdx.x & 63u) == 0u && (hits | ended))
    atomicAdd(count, (unsigned long long)__popcll(hits) | ((unsigned long long)__popcll(ended) << 32));
}

// Everything that refuses a call, before any device is touched.
static int cast_check(tsdf_handle h, const float *org, const float *dir, size_t n, int flags, const float *out, const uint8_t *rgb) {
  if (!h || !org || !dir || !out || !n || n >= (1ull << 31) || (flags & ~TSDF_HIP_RAYS_AS_GIVEN)) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_cast_rays");
  if (h->z_first != 0 || h->nz_alloc != h->nz || h->z_begin != 0 || h->z_end != h->nz) {
    tsdf_set_error("tsdf_hip_cast_rays: this handle holds a Z-slab, not the whole grid (a ray's steps depend on every voxel it visits)");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  if (rgb && h->lab_img) {
    tsdf_set_error("tsdf_hip_cast_rays: the exact colour bytes of a TSDF_COLOR_LAB volume need the host's pow; pass rgb = NULL and use "
                   "tsdf_hip_lookup_rgb on the hit points");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  return TSDF_HIP_OK;
}

// Queue the kernel on the handle's stream; every pointer is device memory.
static int cast_launch(tsdf_handle h, const float *d_org, const float *d_dir, const float *d_range, size_t n, float *d_out, uint8_t *d_rgb,
                       uint8_t *d_status) {
  const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
  RayArgs a;
  (void)make_ray_args(h, eye, zero, 1, a);  // the handle's constants; the image is not used
  const CastRays r{d_org, d_dir, d_range, a.zmin, a.zmax, (unsigned)n};
  h->cast_timed = false;
  if (const int rc = h->cast_ev.ensure(2)) return rc;
  if (const int rc = h->cast_count.reserve(sizeof(unsigned long long), h->stream)) return rc;
  TSDF_HIP_TRY(hipMemsetAsync(h->cast_count.p, 0, sizeof(unsigned long long), h->stream));
  TSDF_HIP_TRY(hipEventRecord(h->cast_ev[0], h->stream));
  hipLaunchKernelGGL(k_cast_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, make_view(h), a, r, d_out, d_rgb, d_status,
                     h->cast_count.as<unsigned long long>());
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(h->cast_ev[1], h->stream));
  h->cast_rays = n;
  h->cast_timed = true;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_cast_rays_device(tsdf_handle h, const float *d_org, const float *d_dir, const float *d_t_range, size_t n, int flags,
                                         float *d_out, uint8_t *d_rgb, uint8_t *d_status) {
  if (const int rc = cast_check(h, d_org, d_dir, n, flags, d_out, d_rgb)) return rc;
  TSDF_ENTER(h);
  return cast_launch(h, d_org, d_dir, d_t_range, n, d_out, d_rgb, d_status);
}

extern "C" int tsdf_hip_cast_rays(tsdf_handle h, const float *org, const float *dir, const float *t_range, size_t n, int flags, float *out,
                                  uint8_t *rgb, uint8_t *status) {
  if (const int rc = cast_check(h, org, dir, n, flags, out, rgb)) return rc;
  TSDF_ENTER(h);
  // scratch layout: org[3n] dir[3n] range[2n] out[8n] floats, rgb[3n] status[n] bytes
  int rc = tsdf_ensure_scratch(h, 16 * n * sizeof(float) + 4 * n);
  if (rc) return rc;
  float *d_org = (float *)h->scratch.p, *d_dir = d_org + 3 * n, *d_range = d_dir + 3 * n, *d_out = d_range + 2 * n;
  uint8_t *d_rgb = (uint8_t *)(d_out + 8 * n), *d_status = d_rgb + 3 * n;
  if ((rc = tsdf_to_device(h, d_org, org, 3 * n * sizeof(float)))) return rc;
  if ((rc = tsdf_to_device(h, d_dir, dir, 3 * n * sizeof(float)))) return rc;
  if (t_range && (rc = tsdf_to_device(h, d_range, t_range, 2 * n * sizeof(float)))) return rc;
  if ((rc = cast_launch(h, d_org, d_dir, t_range ? d_range : nullptr, n, d_out, rgb ? d_rgb : nullptr, status ? d_status : nullptr))) return rc;
  if ((rc = tsdf_to_host(h, out, d_out, 8 * n * sizeof(float)))) return rc;
  if (rgb && (rc = tsdf_to_host(h, rgb, d_rgb, 3 * n))) return rc;
  if (status && (rc = tsdf_to_host(h, status, d_status, n))) return rc;
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_cast_rays_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (h->multi || !h->cast_timed) return TSDF_HIP_OK;
  TSDF_ON_DEVICE(h->device);
  TSDF_HIP_TRY(hipEventSynchronize(h->cast_ev[1]));
  unsigned long long c = 0;
  TSDF_HIP_TRY(hipMemcpy(&c, h->cast_count.p, sizeof c, hipMemcpyDeviceToHost));
  float ms = 0.f;
  TSDF_HIP_TRY(hipEventElapsedTime(&ms, h->cast_ev[0], h->cast_ev[1]));
  out[0] = h->cast_rays;
  out[1] = c & 0xffffffffull;
  out[2] = c >> 32;
  out[3] = (uint64_t)(ms * 1000.f);
  return TSDF_HIP_OK;
}
