// Internal: the admission rule of tsdf_hip_cast_rays (include/tsdf_hip.h, castRays) -- which rays the march kernel takes
// at all, and the integer trip cap that ends a ray whatever its float arithmetic does.  Pure: no grid, no device state; the
// kernels of tsdf_castrays.hip call it per ray, and tests/harness/castrays_admit.cpp compiles it with the host compiler alone.
#pragma once

#include <math.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define TSDF_RAY_CAP_MAX 16777216u  // 2^24 trips: the longest ray the kernel takes

static inline __host__ __device__ bool tsdf_ray_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN, +-inf

// false: the ray is refused (status 2) -- one of its 8 inputs is not finite, or its range would need more than 2^24 trips.
// Otherwise *cap = 16 + 2 * ceil((tmax - tmin) / (leaf / 4)), in double: the main loop advances by at least leaf / 4 per
// iteration (tsdf_volume_octree.cpp:360), so a ray that makes the reference's forward progress spends at most
// ceil(range / (leaf / 4)) main-loop iterations and no more refinement steps than that again; the 16 cover the walk's two
// extra steps and rounding.  tmax <= tmin is admitted with the floor of 16: the loop does not run, as in the reference.
static inline __host__ __device__ bool ray_admit(const float o[3], const float u[3], float tmin, float tmax, float leaf, uint32_t *cap) {
  *cap = 0;
  if (!(tsdf_ray_finite(o[0]) && tsdf_ray_finite(o[1]) && tsdf_ray_finite(o[2]) && tsdf_ray_finite(u[0]) && tsdf_ray_finite(u[1]) &&
        tsdf_ray_finite(u[2]) && tsdf_ray_finite(tmin) && tsdf_ray_finite(tmax)))
    return false;
  const double range = (double)tmax - (double)tmin;
  const double trips = range > 0.0 ? ceil(range / ((double)leaf / 4.0)) : 0.0;
  const double c = 16.0 + 2.0 * trips;
  if (!(c <= (double)TSDF_RAY_CAP_MAX)) return false;  // (also a leaf of 0 or NaN)
  *cap = (uint32_t)c;
  return true;
}
