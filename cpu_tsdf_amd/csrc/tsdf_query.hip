// libtsdf_hip.so -- renderView (one thread per ray) and getFxn/getGradient/getHessian (one thread per
// query point) on the flat SoA grid.
//
// Replaces TSDFVolumeOctree::renderView (src/lib/tsdf_volume_octree.cpp:278-421),
// getTSDFValue/interpolateTrilinearly (:453-541), getFxn/getGradient/getHessian/getNeighbors (:655-828).
// Every root-to-leaf pointer chase of the reference (Octree::getContainingVoxel, src/lib/octree.cpp:
// 112-133,628-643) becomes an index computation that replays the octree's descent comparisons exactly,
// so a ray visits the same voxels and takes the same steps as on the CPU.  Both kernels are
// gather/latency-bound (dependent loads along the ray); no roofline claim is made for them.
// Compiled with -ffp-contract=off; float/double operation order follows the reference line by line.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include <string.h>

#include "tsdf_common.h"
#include "tsdf_gridview.h"
#include "tsdf_raymarch.h"  // trilinear, normalize3, RayArgs, RaySlab, ray_march: shared with tsdf_castrays.hip
#ifdef TSDF_HIP_TEST_HOOKS
#include "tsdf_hip_test.h"
#endif

static __device__ __forceinline__ void ray_direction(const RayArgs &a, int64_t i, float du[3]) {
  const size_t x = (size_t)(i % a.nw), y = (size_t)(i / a.nw);
  du[0] = (float)((x - a.ncx) / a.nfx);
  du[1] = (float)((y - a.ncy) / a.nfy);
  du[2] = 1.f;
  normalize3(du);
  // du = R * du: each coefficient p0 + (p1 + p2) [Eigen-recall 3.3 reduction tree]
  const float p = du[0], q = du[1], r = du[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) du[k] = a.rot[3 * k] * p + (a.rot[3 * k + 1] * q + a.rot[3 * k + 2] * r);
}

// The state every ray starts from (:305-313).
static __global__ void __launch_bounds__(256) k_ray_begin(const RayArgs a, int *__restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.nw * a.nh) return;
  float du[3];
  ray_direction(a, i, du);
  int *r = state + RAY_REC * i;
  const float t = a.zmin;
  r[0] = 1;
  r[1] = -1;
  r[2] = 0;
  r[3] = 0;
  r[4] = __float_as_int(t);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float pt = a.org[k];
    pt += t * du[k];
    r[5 + k] = __float_as_int(pt);
  }
  r[8] = r[9] = 0;  // last_d, last_w = 0.f
  r[10] = __float_as_int(a.min_step);
  r[11] = (int)i;  // the ray's pixel index: lets records travel in compact lists (tsdf_hip_raycast_advance_list)
  for (int k = 12; k < RAY_REC; ++k) r[k] = 0;
}

// renderView, tsdf_volume_octree.cpp:290-421, one ray per thread: the pixel's ray through ray_march (tsdf_raymarch.h).
// out: 8 floats per pixel: x,y,z, nx,ny,nz, t (t_star on a hit), iterations; `incomplete` counts rays
// that touched a plane this handle does not hold (only possible for Z-slab handles).
// RESUMABLE: see RaySlab (tsdf_raymarch.h); `out` is unused, results go to the ray's record in `delta`.
template <bool RESUMABLE>
static __global__ void __launch_bounds__(256)
k_raycast(const GridView g, const RayArgs a, float *__restrict__ out, unsigned *__restrict__ incomplete,
          const int *__restrict__ state, int *__restrict__ delta, const RaySlab rs) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // record (and, unless a list, pixel) index
  int64_t i = slot;
  if (RESUMABLE && rs.list_count > 0) {
    if (slot >= rs.list_count) return;
    i = state[RAY_REC * slot + 11];
  }
  if (i < 0 || i >= (int64_t)a.nw * a.nh) return;
  PixelRay src;
  ray_direction(a, i, src.du);
#pragma unroll
  for (int k = 0; k < 3; ++k) src.org[k] = a.org[k];
  src.zmin = a.zmin;
  src.zmax = a.zmax;
  (void)ray_march<RESUMABLE>(g, a, src, i, slot, RESUMABLE ? nullptr : out + 8 * i, incomplete, state, delta, rs);
}

static int raycast_impl(tsdf_handle h, const float rot[9], const float origin[3], int downsample, const double *inv,
                        float *out) {
  if (!h || !rot || !origin || !out || downsample < 1) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_raycast(h, rot, origin, downsample, inv, out);
  TSDF_ENTER(h);
  RayArgs a;
  if (make_ray_args(h, rot, origin, downsample, a)) return TSDF_HIP_E_INVALID;
  if (inv) {
    a.to_camera = 1;
    for (int i = 0; i < 12; ++i) a.inv[i] = inv[i];
  }
  const int64_t n = (int64_t)a.nw * a.nh;
  int rc = tsdf_ensure_scratch(h, (size_t)n * 8 * sizeof(float) + 16);
  if (rc) return rc;
  float *d_out = (float *)h->scratch.p;
  unsigned *d_inc = (unsigned *)((char *)h->scratch.p + (size_t)n * 8 * sizeof(float));
  TSDF_HIP_TRY(hipMemsetAsync(d_inc, 0, sizeof(unsigned), h->stream));
  const GridView g = make_view(h);
  hipLaunchKernelGGL(k_raycast<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, g, a, d_out, d_inc,
                     (const int *)nullptr, (int *)nullptr, RaySlab{0, 1, 0, 0, 0});
  TSDF_HIP_TRY(hipGetLastError());
  unsigned inc = 0;
  TSDF_HIP_TRY(hipMemcpyAsync(&inc, d_inc, sizeof inc, hipMemcpyDeviceToHost, h->stream));
  if ((rc = tsdf_to_host(h, out, d_out, (size_t)n * 8 * sizeof(float)))) return rc;  // (synchronises the stream)
  if (inc) {
    tsdf_set_error("raycast touched planes outside this handle's Z-slab (+halo)");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_raycast(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                                float *out) {
  return raycast_impl(h, rot, origin, downsample, nullptr, out);
}

extern "C" int tsdf_hip_raycast_camera(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                                       const double cam_from_vol[12], float *out) {
  if (!cam_from_vol) return TSDF_HIP_E_INVALID;
  return raycast_impl(h, rot, origin, downsample, cam_from_vol, out);
}

// Multi-slab renderView: ray records on the DEVICE (see RaySlab).  begin fills the start state of every
// ray; advance zero-fills `d_delta`, resumes the rays this handle is responsible for and writes their new
// records there.  The caller sums the deltas of all ranks (integer all-reduce: every ray is advanced by
// exactly one rank) and overwrites the touched records.
extern "C" int tsdf_hip_raycast_begin(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                                      int32_t *d_state) {
  if (!h || !rot || !origin || !d_state || downsample < 1) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_raycast_begin");
  TSDF_ENTER(h);
  RayArgs a;
  if (make_ray_args(h, rot, origin, downsample, a)) return TSDF_HIP_E_INVALID;
  const int64_t n = (int64_t)a.nw * a.nh;
  hipLaunchKernelGGL(k_ray_begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, a, (int *)d_state);
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_raycast_advance(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                                        int rank, int world, const int32_t *d_state, int32_t *d_delta) {
  if (!h || !rot || !origin || !d_state || !d_delta || downsample < 1 || world < 1 || rank < 0 || rank >= world)
    return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_raycast_advance");
  TSDF_ENTER(h);
  RayArgs a;
  if (make_ray_args(h, rot, origin, downsample, a)) return TSDF_HIP_E_INVALID;
  const int64_t n = (int64_t)a.nw * a.nh;
  int rc = tsdf_ensure_scratch(h, 16);
  if (rc) return rc;
  unsigned *d_inc = (unsigned *)h->scratch.p;
  TSDF_HIP_TRY(hipMemsetAsync(d_inc, 0, sizeof(unsigned), h->stream));
  TSDF_HIP_TRY(hipMemsetAsync(d_delta, 0, (size_t)n * RAY_REC * sizeof(int32_t), h->stream));
  const GridView g = make_view(h);
  hipLaunchKernelGGL(k_raycast<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, g, a,
                     (float *)nullptr, d_inc, (const int *)d_state, (int *)d_delta,
                     RaySlab{rank, world, h->z_begin, h->z_end, 0});
  TSDF_HIP_TRY(hipGetLastError());
  unsigned inc = 0;
  TSDF_HIP_TRY(hipMemcpyAsync(&inc, d_inc, sizeof inc, hipMemcpyDeviceToHost, h->stream));
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  if (inc) {
    tsdf_set_error("ray hand-off: the refinement walk / trilinear samples left this handle's halo planes; "
                   "create the slab with a larger halo (tsdf_hip_render_halo)");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  return TSDF_HIP_OK;
}

// The same on a COMPACT list of `count` records (ray id in word 11), updated in place: the scalable form of the
// hand-off, where a record travels point-to-point to the rank that owns its next voxel instead of every rank
// holding every ray.  Records this handle is not responsible for are left untouched.
extern "C" int tsdf_hip_raycast_advance_list(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                                             int rank, int world, int32_t *d_records, size_t count) {
  if (!h || !rot || !origin || downsample < 1 || world < 1 || rank < 0 || rank >= world || count >= (1ull << 31) ||
      (count && !d_records))
    return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_raycast_advance_list");
  if (!count) return TSDF_HIP_OK;
  TSDF_ENTER(h);
  RayArgs a;
  if (make_ray_args(h, rot, origin, downsample, a)) return TSDF_HIP_E_INVALID;
  int rc = tsdf_ensure_scratch(h, 16);
  if (rc) return rc;
  unsigned *d_inc = (unsigned *)h->scratch.p;
  TSDF_HIP_TRY(hipMemsetAsync(d_inc, 0, sizeof(unsigned), h->stream));
  hipLaunchKernelGGL(k_raycast<true>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, make_view(h), a,
                     (float *)nullptr, d_inc, (const int *)d_records, (int *)d_records,
                     RaySlab{rank, world, h->z_begin, h->z_end, (int)count});
  TSDF_HIP_TRY(hipGetLastError());
  unsigned inc = 0;
  TSDF_HIP_TRY(hipMemcpyAsync(&inc, d_inc, sizeof inc, hipMemcpyDeviceToHost, h->stream));
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  if (inc) {
    tsdf_set_error("ray hand-off: the refinement walk / trilinear samples left this handle's halo planes; "
                   "create the slab with a larger halo (tsdf_hip_render_halo)");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  return TSDF_HIP_OK;
}

// ---------------------------------------------------------------------------------------------
// Compact ray lists for the one-process multi-GPU renderView (tsdf_multi.hip).  Every slab keeps ONLY the records it is
// responsible for; after a round of k_raycast<true> in list mode a record is either finished -- its pixel index and 8
// output floats go to the image on the first slab -- or suspended for the owner of its next plane, and travels there
// point-to-point.  The kernels below are the device side of that routing: nothing image-sized ever crosses a link.
#define RAY_FIN_INTS TSDF_RAY_FIN_INTS
struct RayRoute {
  int n_slab;
  int z_end[TSDF_MAX_SLABS];  // owner of plane z = first slab whose z_end exceeds it
};

// The start records of the rays with pixel index = rank (mod world), as a compact list (:305-313).
static __global__ void __launch_bounds__(256)
k_ray_begin_list(const RayArgs a, int *__restrict__ list, int rank, int world, unsigned count) {
  const unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  const int64_t i = (int64_t)slot * world + rank;
  float du[3];
  ray_direction(a, i, du);
  int *r = list + RAY_REC * (size_t)slot;
  const float t = a.zmin;
  r[0] = 1;
  r[1] = -1;
  r[2] = 0;
  r[3] = 0;
  r[4] = __float_as_int(t);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float pt = a.org[k];
    pt += t * du[k];
    r[5 + k] = __float_as_int(pt);
  }
  r[8] = r[9] = 0;
  r[10] = __float_as_int(a.min_step);
  r[11] = (int)i;
  for (int k = 12; k < RAY_REC; ++k) r[k] = 0;
}

static __device__ __forceinline__ int ray_dest(const RayRoute &rt, const int *r) {
  if (r[0] == 2) return rt.n_slab;  // finished: to the image
  int d = 0;
  while (d < rt.n_slab - 1 && r[1] >= rt.z_end[d]) ++d;
  return d;
}

// counters[0 .. n_slab] = records per destination (n_slab = finished)
static __global__ void __launch_bounds__(256)
k_ray_route_count(const int *__restrict__ list, unsigned count, const RayRoute rt, unsigned *__restrict__ counters) {
  __shared__ unsigned hist[TSDF_MAX_SLABS + 1];
  for (int k = threadIdx.x; k <= rt.n_slab; k += 256) hist[k] = 0;
  __syncthreads();
  const unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot < count) atomicAdd(&hist[ray_dest(rt, list + RAY_REC * (size_t)slot)], 1u);
  __syncthreads();
  for (int k = threadIdx.x; k <= rt.n_slab; k += 256)
    if (hist[k]) atomicAdd(&counters[k], hist[k]);
}

// cursors[d] = first outbox slot of destination d (exclusive prefix over the slabs); the finished rays have their own box
static __global__ void k_ray_route_offsets(const unsigned *__restrict__ counters, unsigned *__restrict__ cursors, int n_slab) {
  if (threadIdx.x || blockIdx.x) return;
  unsigned run = 0;
  for (int k = 0; k < n_slab; ++k) {
    cursors[k] = run;
    run += counters[k];
  }
  cursors[n_slab] = 0;
}

// Records sorted by destination into `outbox` (suspended, whole records) and `finbox` (finished, RAY_FIN_INTS words);
// one atomic per wave and destination.
static __global__ void __launch_bounds__(256)
k_ray_route_scatter(const int *__restrict__ list, unsigned count, const RayRoute rt, unsigned *__restrict__ cursors,
                    int *__restrict__ outbox, int *__restrict__ finbox) {
  const unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = slot < count;
  const int *r = list + RAY_REC * (size_t)(valid ? slot : 0);
  const int dest = valid ? ray_dest(rt, r) : -1;
  const unsigned lane = threadIdx.x & 63u;
  unsigned pos = 0;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int d = __shfl(dest, leader);
    const unsigned long long same = __ballot(valid && dest == d);
    unsigned base = 0;
    if ((int)lane == leader) base = atomicAdd(&cursors[d], (unsigned)__popcll(same));
    base = __shfl(base, leader);
    if (valid && dest == d) pos = base + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  if (!valid) return;
  if (dest == rt.n_slab) {
    int *o = finbox + RAY_FIN_INTS * (size_t)pos;
    o[0] = r[11];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[1 + k] = r[16 + k];
  } else {
    int *o = outbox + RAY_REC * (size_t)pos;
#pragma unroll
    for (int k = 0; k < RAY_REC; ++k) o[k] = r[k];
  }
}

// Finished rays into the image (8 floats per pixel), with renderView's last line (:422) applied as k_raycast does.
struct RayDeliver {
  int to_camera;
  double inv[12];
};
static __global__ void __launch_bounds__(256)
k_ray_deliver(const int *__restrict__ fin, unsigned count, float *__restrict__ out, int64_t n_pix, const RayDeliver dl) {
  const unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  const int *f = fin + RAY_FIN_INTS * (size_t)slot;
  const int64_t pix = f[0];
  if (pix < 0 || pix >= n_pix) return;
  float o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = __int_as_float(f[1 + k]);
  if (dl.to_camera && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2])) {
    const double px = o[0], py = o[1], pz = o[2], nx = o[3], ny = o[4], nz = o[5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      o[r] = (float)(px * dl.inv[4 * r] + (py * dl.inv[4 * r + 1] + (pz * dl.inv[4 * r + 2] + dl.inv[4 * r + 3])));
      o[3 + r] = (float)(nx * dl.inv[4 * r] + (ny * dl.inv[4 * r + 1] + nz * dl.inv[4 * r + 2]));
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) out[8 * pix + k] = o[k];
}

// Host side of the above, all asynchronous on the slab's stream (the caller is on the slab's device).
unsigned tsdf_ray_list_share(int64_t n_rays, int rank, int world) {  // rays with index = rank (mod world)
  return n_rays > rank ? (unsigned)((n_rays - rank + world - 1) / world) : 0u;
}

int tsdf_ray_list_begin(tsdf_handle s, const float rot[9], const float origin[3], int downsample, int rank, int world,
                        int32_t *d_list, unsigned *count) {
  RayArgs a;
  if (make_ray_args(s, rot, origin, downsample, a)) return TSDF_HIP_E_INVALID;
  *count = tsdf_ray_list_share((int64_t)a.nw * a.nh, rank, world);
  if (!*count) return TSDF_HIP_OK;
  hipLaunchKernelGGL(k_ray_begin_list, dim3((*count + 255u) / 256u), dim3(256), 0, s->stream, a, (int *)d_list, rank, world, *count);
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

int tsdf_ray_list_advance(tsdf_handle s, const float rot[9], const float origin[3], int downsample, int rank, int world,
                          int32_t *d_list, unsigned count, unsigned *d_incomplete) {
  if (!count) return TSDF_HIP_OK;
  RayArgs a;
  if (make_ray_args(s, rot, origin, downsample, a)) return TSDF_HIP_E_INVALID;
  hipLaunchKernelGGL(k_raycast<true>, dim3((count + 255u) / 256u), dim3(256), 0, s->stream, make_view(s), a, (float *)nullptr,
                     d_incomplete, (const int *)d_list, (int *)d_list, RaySlab{rank, world, s->z_begin, s->z_end, (int)count});
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

// d_counters: 2 * (n_slab + 1) words -- counts per destination, then the scatter cursors.
int tsdf_ray_list_route(tsdf_handle s, const int32_t *d_list, unsigned count, int n_slab, const int *z_end,
                        unsigned *d_counters, int32_t *d_outbox, int32_t *d_finbox) {
  if (n_slab < 1 || n_slab > TSDF_MAX_SLABS) return TSDF_HIP_E_INVALID;
  TSDF_HIP_TRY(hipMemsetAsync(d_counters, 0, 2 * (size_t)(n_slab + 1) * sizeof(unsigned), s->stream));
  if (!count) return TSDF_HIP_OK;
  RayRoute rt;
  rt.n_slab = n_slab;
  for (int k = 0; k < TSDF_MAX_SLABS; ++k) rt.z_end[k] = k < n_slab ? z_end[k] : INT_MAX;
  const dim3 grid((count + 255u) / 256u), block(256);
  hipLaunchKernelGGL(k_ray_route_count, grid, block, 0, s->stream, (const int *)d_list, count, rt, d_counters);
  hipLaunchKernelGGL(k_ray_route_offsets, dim3(1), dim3(64), 0, s->stream, (const unsigned *)d_counters, d_counters + n_slab + 1, n_slab);
  hipLaunchKernelGGL(k_ray_route_scatter, grid, block, 0, s->stream, (const int *)d_list, count, rt, d_counters + n_slab + 1,
                     (int *)d_outbox, (int *)d_finbox);
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

int tsdf_ray_deliver(tsdf_handle s, const int32_t *d_fin, unsigned count, float *d_out, int64_t n_pix, const double *inv) {
  if (!count) return TSDF_HIP_OK;
  RayDeliver dl;
  dl.to_camera = inv ? 1 : 0;
  for (int i = 0; i < 12; ++i) dl.inv[i] = inv ? inv[i] : 0.0;
  hipLaunchKernelGGL(k_ray_deliver, dim3((count + 255u) / 256u), dim3(256), 0, s->stream, (const int *)d_fin, count, d_out, n_pix, dl);
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

// Planes of halo a Z-slab handle needs on each side for tsdf_hip_raycast_advance: the refinement walk goes
// back at most one main-loop step plus one refinement step, and the trilinear / central-difference samples reach two
// more voxels.  A main-loop step is max(leaf/4, |d| * max_dist_neg) (.cpp:360) and d lies in [-1, max_dist_pos /
// max_dist_neg], so the longest one is max(max_dist_neg, max_dist_pos) -- the hinge value exceeds 1 when the
// truncation is asymmetric (found by tests/evidence/fuzz_product_vs_oracle.py; before, the halo assumed |d| <= 1).
extern "C" int tsdf_hip_render_halo(const tsdf_params *p) {
  if (!p || p->res[2] <= 0 || !(p->size[2] > 0)) return -1;
  const double vs = (double)p->size[2] / p->res[2];
  const double leaf = (double)p->size[0] / p->res[0];
  const double step = std::max(leaf / 4, (double)std::max(p->max_dist_neg, p->max_dist_pos));
  return (int)ceil(step / vs) + 4;
}

// renderColoredView's per-hit lookup (tsdf_volume_octree.cpp:443-448): octree_->getContainingVoxel(v) then
// voxel->getRGB, batched.  found[i] = 0 where the reference gets NULL (or the plane is not held by this handle).
static __global__ void __launch_bounds__(256)
k_lookup_rgb(const GridView g, const int own_lo, const int own_hi, const float *__restrict__ xyz, size_t n,
             unsigned char *__restrict__ rgb, unsigned char *__restrict__ found) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t c;
  const bool hit = lookup_rgb_at(g, own_lo, own_hi, xyz[3 * t], xyz[3 * t + 1], xyz[3 * t + 2], c);
  rgb[3 * t] = (unsigned char)(c & 255u);
  rgb[3 * t + 1] = (unsigned char)((c >> 8) & 255u);
  rgb[3 * t + 2] = (unsigned char)((c >> 16) & 255u);
  found[t] = hit ? 1 : 0;
}

// the same, but the voxel's element index instead of its cached colour (-1 where not found): TSDF_COLOR_LAB volumes
// finish the colour on the host (tsdf_lab_exact_colors)
static __global__ void __launch_bounds__(256)
k_lookup_index(const GridView g, const int own_lo, const int own_hi, const float *__restrict__ xyz, size_t n,
               int64_t *__restrict__ idx) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  int64_t vi;
  bool local;
  int k;
  const bool hit = containing(g, xyz[3 * t], xyz[3 * t + 1], xyz[3 * t + 2], vi, local, k) && local && k >= own_lo && k < own_hi;
  idx[t] = hit ? vi : -1;
}

extern "C" int tsdf_hip_lookup_rgb(tsdf_handle h, const float *xyz, size_t n, uint8_t *rgb, uint8_t *found) {
  if (!h || !xyz || !n || !rgb || !found) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_lookup_rgb(h, xyz, n, rgb, found);
  TSDF_ENTER(h);
  if (h->lab_img) {  // LABNode::getRGB: exact bytes through the host's pow
    int rc = tsdf_ensure_scratch(h, n * 12);
    if (rc) return rc;
    float *d_xyz = (float *)h->scratch.p;
    if ((rc = tsdf_to_device(h, d_xyz, xyz, n * 12))) return rc;
    DevBuf idx_buf;
    if ((rc = idx_buf.alloc(n * sizeof(int64_t)))) return rc;
    int64_t *d_idx = idx_buf.as<int64_t>();
    hipLaunchKernelGGL(k_lookup_index, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, make_view(h), h->z_begin, h->z_end,
                       d_xyz, n, d_idx);
    std::vector<int64_t> idx(n);
    std::vector<uint32_t> words(n);
    rc = tsdf_to_host(h, idx.data(), d_idx, n * sizeof(int64_t));
    if (!rc) rc = tsdf_lab_exact_colors(h, d_idx, n, words.data(), false);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
      const bool hit = idx[i] >= 0;
      found[i] = hit ? 1 : 0;
      rgb[3 * i] = hit ? (uint8_t)(words[i] & 255u) : 0;
      rgb[3 * i + 1] = hit ? (uint8_t)((words[i] >> 8) & 255u) : 0;
      rgb[3 * i + 2] = hit ? (uint8_t)((words[i] >> 16) & 255u) : 0;
    }
    return TSDF_HIP_OK;
  }
  int rc = tsdf_ensure_scratch(h, n * 16);
  if (rc) return rc;
  float *d_xyz = (float *)h->scratch.p;
  unsigned char *d_rgb = (unsigned char *)(d_xyz + 3 * n), *d_found = d_rgb + 3 * n;
  if ((rc = tsdf_to_device(h, d_xyz, xyz, n * 12))) return rc;
  hipLaunchKernelGGL(k_lookup_rgb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, make_view(h), h->z_begin, h->z_end,
                     d_xyz, n, d_rgb, d_found);
  TSDF_HIP_TRY(hipGetLastError());
  if ((rc = tsdf_to_host(h, rgb, d_rgb, n * 3))) return rc;
  return tsdf_to_host(h, found, d_found, n);
}

// Test hook: Octree::getContainingVoxel's voxel index for arbitrary points (idx = i, j, k or -1, -1, -1 for NULL).
// (Measured alternatives to the level-by-level walk -- a boundary-table search and, on dyadic grids, computed
// boundaries -- were slower inside k_raycast: 1.78 and 2.40 ms vs 1.55 ms per 640x480 view at 2048^3; the
// fixed-trip, branch-free walk wins over shorter but divergent searches.)
#ifdef TSDF_HIP_TEST_HOOKS
static __global__ void __launch_bounds__(256)
k_selftest_containing(const GridView g, const float *__restrict__ xyz, size_t n, int *__restrict__ idx) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float x = xyz[3 * t], y = xyz[3 * t + 1], z = xyz[3 * t + 2];
  int64_t vi;
  bool local;
  int k;
  if (containing(g, x, y, z, vi, local, k)) {
    idx[3 * t] = axis_index(g, 0, x);
    idx[3 * t + 1] = axis_index(g, 1, y);
    idx[3 * t + 2] = k;
  } else {
    idx[3 * t] = idx[3 * t + 1] = idx[3 * t + 2] = -1;
  }
}

extern "C" int tsdf_hip_selftest_containing(tsdf_handle h, const float *xyz, size_t n, int32_t *idx) {
  if (!h || !xyz || !n || !idx) return TSDF_HIP_E_INVALID;
  if (h->multi) h = tsdf_multi_first(h);  // the descent only reads the centre tables, which every slab holds
  TSDF_ENTER(h);
  int rc = tsdf_ensure_scratch(h, n * 24);
  if (rc) return rc;
  float *d_xyz = (float *)h->scratch.p;
  int *d_idx = (int *)(d_xyz + 3 * n);
  if ((rc = tsdf_to_device(h, d_xyz, xyz, n * 12))) return rc;
  hipLaunchKernelGGL(k_selftest_containing, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, make_view(h), d_xyz,
                     n, d_idx);
  TSDF_HIP_TRY(hipGetLastError());
  return tsdf_to_host(h, idx, d_idx, n * 12);
}
#endif  // TSDF_HIP_TEST_HOOKS

// getFxn / getGradient / getHessian: the per-point arithmetic is sample_point (tsdf_gridview.h), one thread per point.
static __global__ void __launch_bounds__(256)
k_sample(const GridView g, const int own_lo, const int own_hi, const float *__restrict__ xyz, size_t n,
         float *__restrict__ val, float *__restrict__ grad, float *__restrict__ hess, unsigned char *__restrict__ ok) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float px = xyz[3 * idx], py = xyz[3 * idx + 1], pz = xyz[3 * idx + 2];
  float v, gr[3], hs[3];
  int xi, yi, zi;
  const bool good = sample_point<true>(g, own_lo, own_hi, px, py, pz, v, gr, hs, xi, yi, zi);
  if (ok) ok[idx] = good ? 1 : 0;
  if (val) val[idx] = v;
  if (grad) {
    grad[3 * idx] = gr[0];
    grad[3 * idx + 1] = gr[1];
    grad[3 * idx + 2] = gr[2];
  }
  if (hess) {
    float *hp = hess + 9 * idx;
    const float z = good ? 0.f : NAN;
    hp[0] = hp[4] = hp[8] = z;
    hp[1] = hp[3] = hs[0];
    hp[2] = hp[6] = hs[1];
    hp[5] = hp[7] = hs[2];
  }
}

extern "C" int tsdf_hip_sample(tsdf_handle h, const float *xyz, size_t n, float *val, float *grad, float *hess,
                               uint8_t *ok) {
  if (!h || !xyz || !n) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_sample(h, xyz, n, val, grad, hess, ok);
  TSDF_ENTER(h);
  // scratch layout: xyz[3n] val[n] grad[3n] hess[9n] floats, ok[n] bytes
  const size_t fl = 16 * n;
  int rc = tsdf_ensure_scratch(h, fl * sizeof(float) + n + 16);
  if (rc) return rc;
  float *d_xyz = (float *)h->scratch.p, *d_val = d_xyz + 3 * n, *d_grad = d_val + n, *d_hess = d_grad + 3 * n;
  unsigned char *d_ok = (unsigned char *)(d_hess + 9 * n);
  if ((rc = tsdf_to_device(h, d_xyz, xyz, 3 * n * sizeof(float)))) return rc;
  const GridView g = make_view(h);
  hipLaunchKernelGGL(k_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, g, h->z_begin, h->z_end, d_xyz,
                     n, d_val, d_grad, d_hess, d_ok);
  TSDF_HIP_TRY(hipGetLastError());
  if (val && (rc = tsdf_to_host(h, val, d_val, n * sizeof(float)))) return rc;
  if (grad && (rc = tsdf_to_host(h, grad, d_grad, 3 * n * sizeof(float)))) return rc;
  if (hess && (rc = tsdf_to_host(h, hess, d_hess, 9 * n * sizeof(float)))) return rc;
  if (ok && (rc = tsdf_to_host(h, ok, d_ok, n))) return rc;
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  return TSDF_HIP_OK;
}
