// libtsdf_hip.so -- mergeVolume: resample a second volume at this one's voxel centres under a rigid transform and add the
// samples as weighted observations (tsdf_hip_merge; NOT in the reference, whose volumes can only be fused frame by frame).
//
// k_merge runs one lane per voxel of `dst`, x along the lanes: the read-modify-write of dst's planes is a coalesced stream,
// the eight distance and eight weight loads per voxel from `src` are a gather next to it (a rigid transform keeps
// neighbouring lanes in neighbouring src voxels, so most of the gather is served from L2; no LDS tiling, no roofline claim).
// Per voxel: centre from dst's centre tables -> q = M c in fp32 (k_align_system's order) -> sample_point<false> on src
// (tsdf_gridview.h: value and `ok` bit for bit what tsdf_hip_sample returns) -> gate (ok, all eight neighbour weights >
// min_weight, a value that is not NaN, a containing voxel) -> RGBNode::addObservation(val, w_s, max_weight_dst, c_s) with w_s and
// c_s from the src voxel that CONTAINS q (Octree::getContainingVoxel, tsdf_gridview.h `containing`).  See include/tsdf_hip.h
// for the rule and every refusal, DESIGN.md 3.17 for why the containing voxel's weight.
// Compiled with -ffp-contract=off; no floating-point atomics: the only atomic is the 64-bit count of merged voxels, one per block.
#include <math.h>

#include <algorithm>

#include "tsdf_common.h"
#include "tsdf_gridview.h"

struct MergeArgs {
  float M[12];               // src_from_dst cast to float, row-major 3 x 4
  float min_weight;
  int x0, x1, y0, y1, z0;    // launch box [x0, x1) x [y0, y1) x [z0, z0 + gridDim.z) of dst voxel indices
  int xa;                    // x0 rounded down to 16 voxels: a wave's 64 lanes start on a 64-byte boundary of the row
  int ny;                    // dst geometry (a whole-grid handle: plane index == z)
  int64_t pitch;
  float *d, *w;              // dst planes; w only in the F32W layout
  uint32_t *rgb;             // colour words; byte 3 is the count of a PACKED dst with colour
  uint8_t *k8;               // the count plane of a PACKED dst without colour
  float wmax;                // dst's max_weight
  unsigned kmax;
  const float *ctr[3];       // dst's centre tables (tsdf_hip_centers)
};

// DST_PACKED: dst keeps counts (src is then PACKED with the same max_weight, so every new weight has a count: see
// tsdf_hip_merge).  COLOR: both volumes store colour; otherwise dst's colour bytes are left as they are.
template <bool DST_PACKED, bool COLOR>
static __global__ void __launch_bounds__(256)
k_merge(const GridView g, const MergeArgs a, unsigned long long *__restrict__ n_merged) {
  __shared__ unsigned s_cnt[4];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const int x = a.xa + (int)blockIdx.x * 64 + (int)lane;
  const int y = a.y0 + (int)blockIdx.y * 4 + (int)wave;
  const int z = a.z0 + (int)blockIdx.z;
  const bool in_box = x >= a.x0 && x < a.x1 && y < a.y1;
  bool ok = false, merge = false;
  float val = NAN, q[3] = {0.f, 0.f, 0.f};
  int xi = 0, yi = 0, zi = 0;
  if (in_box) {
    const float cx = a.ctr[0][x], cy = a.ctr[1][y], cz = a.ctr[2][z];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = ((a.M[4 * r] * cx + a.M[4 * r + 1] * cy) + a.M[4 * r + 2] * cz) + a.M[4 * r + 3];
    float gr[3], hs[3];
    ok = sample_point<false>(g, 0, g.nz, q[0], q[1], q[2], val, gr, hs, xi, yi, zi);
  }
  if (__any(ok)) {  // (a wave wholly outside src's sampled region -- most of the padded launch box -- leaves here)
    int64_t vs = 0;
    if (ok) {  // (xi, yi, zi) .. + 1 are inside src
      const int64_t o = ((int64_t)(zi - g.z_first) * g.ny + yi) * g.pitch + xi;
      const int64_t sy = g.pitch, sz = (int64_t)g.ny * g.pitch;
      merge = val == val;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int64_t oc = o + ((c & 4) ? 1 : 0) + ((c & 2) ? sy : 0) + ((c & 1) ? sz : 0);
        merge = merge && (tsdf_load_w(g.pv, oc) > a.min_weight);
      }
      bool local;
      int k;
      merge = merge && containing(g, q[0], q[1], q[2], vs, local, k);  // (a whole grid: always local)
    }
    if (merge) {  // every lane that is not merged neither reads nor writes dst
      const float ws = tsdf_load_w(g.pv, vs);  // one of the eight: > min_weight >= 0, so w + ws > 0
      const int64_t vi = ((int64_t)z * a.ny + y) * a.pitch + x;
      unsigned k_old = 0u;
      uint32_t old = 0u;
      float w, d = a.d[vi];
      if (DST_PACKED) {
        if (a.rgb) {
          old = a.rgb[vi];
          k_old = old >> 24;
        } else {
          k_old = (unsigned)a.k8[vi];
        }
        w = tsdf_decode_w(k_old, a.wmax);
      } else {
        w = a.w[vi];
        if (COLOR) old = a.rgb[vi];
      }
      const float wsum = w + ws;
      uint32_t out = old & 0xffffffu;
      if (COLOR) {  // RGBNode::addObservation, octree.cpp:331-335: the OLD w, static_cast<uint8_t> = cvttss2si & 255
        const uint32_t cs = tsdf_load_rgb(g.pv, vs);
        out = 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float c_old = (float)((old >> (8 * ch)) & 255u);
          const float c_new = (float)((cs >> (8 * ch)) & 255u);
          const float qv = (w * c_old + ws * c_new) / wsum;
          // in [0, 255] for the weights integrateCloud leaves; an F32W dst may hold any float an upload put there (negative,
          // inf, NaN), and then, as in k_integrate_plain: x86 gives INT_MIN, whose low byte is 0, for NaN and anything outside int32
          const bool in_range = qv > -2147483904.f && qv < 2147483648.f;
          out |= (in_range ? ((uint32_t)(int)qv & 255u) : 0u) << (8 * ch);
        }
      }
      d = (d * w + val * ws) / wsum;  // octree.cpp:156
      w = wsum;                       // :157
      if (w > a.wmax) w = a.wmax;     // :158-159
      a.d[vi] = d;
      if (DST_PACKED) {
        unsigned k_new;
        (void)tsdf_encode_w(w, a.wmax, a.kmax, k_new);  // (always representable: tsdf_hip_merge's refusals)
        if (a.rgb)
          a.rgb[vi] = out | (k_new << 24);
        else
          a.k8[vi] = (uint8_t)k_new;
      } else {
        a.w[vi] = w;
        if (COLOR) a.rgb[vi] = out;
      }
    }
  }
  const unsigned long long mask = __ballot(merge);
  if (lane == 0u) s_cnt[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0u) {
    const unsigned n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (n) atomicAdd(n_merged, (unsigned long long)n);
  }
}

// The launch box: src's bounding box (the cube |p| <= size / 2 that sample_point can answer in) taken to dst index space in
// fp64 through the inverse of src_from_dst, its enclosing index box on the spacing of dst's centre tables padded by two voxels
// (the kernel's fp32 transform and the tables' recurrence differ from this arithmetic by far less) and clamped to the grid.  Only an optimisation: a matrix that
// cannot be inverted gets the whole grid.  false: the box is empty.
static bool merge_box(const tsdf_hip_volume *dst, const tsdf_hip_volume *src, const double M[12], int lo[3], int hi[3]) {
  const int res[3] = {dst->nx, dst->ny, dst->nz};
  for (int a = 0; a < 3; ++a) lo[a] = 0, hi[a] = res[a] - 1;
  const double A[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]}, t[3] = {M[3], M[7], M[11]};
  const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
  if (!std::isfinite(det) || det == 0.0) return true;
  const double I[9] = {(A[4] * A[8] - A[5] * A[7]) / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                       (A[5] * A[6] - A[3] * A[8]) / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                       (A[3] * A[7] - A[4] * A[6]) / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = 0; c < 8; ++c) {
    double p[3];
    for (int a = 0; a < 3; ++a) p[a] = (((c >> a) & 1) ? 0.5 : -0.5) * (double)src->p.size[a] - t[a];
    for (int a = 0; a < 3; ++a) {
      const double v = I[3 * a] * p[0] + I[3 * a + 1] * p[1] + I[3 * a + 2] * p[2];                // dst volume coordinates
      // voxel centres at integers, on the spacing of dst's CENTRE TABLES, which is what the kernel transforms: tsdf_node_size
      // (size_x on every axis of an octree grid, whatever setGridSize said for y and z), not p.size[a]
      const double node = (double)tsdf_node_size(dst->p, a);
      const double i = (v + node / 2.0) / node * res[a] - 0.5;
      if (!std::isfinite(i)) return true;
      mn[a] = std::min(mn[a], i);
      mx[a] = std::max(mx[a], i);
    }
  }
  for (int a = 0; a < 3; ++a) {
    const double l = floor(mn[a]) - 2.0, h = ceil(mx[a]) + 2.0;
    if (h < 0.0 || l > (double)(res[a] - 1)) return false;
    lo[a] = (int)std::max(l, 0.0);
    hi[a] = (int)std::min(h, (double)(res[a] - 1));
  }
  return true;
}

static const char *merge_refusal(const tsdf_hip_volume *dst, const tsdf_hip_volume *src) {
  if (dst->multi || src->multi) return "tsdf_hip_merge works on ONE handle each; a multi-GPU set (tsdf_hip_create_multi) is not supported";
  for (const tsdf_hip_volume *v : {dst, src})
    if (v->z_first != 0 || v->nz_alloc != v->nz || v->z_begin != 0 || v->z_end != v->nz)
      return "tsdf_hip_merge: a handle that owns part of its grid (z_begin / z_end) is not supported";
  if (dst->device != src->device) return "tsdf_hip_merge: the two handles are on different devices";
  const tsdf_params &s = src->p;
  if (s.res[0] != s.res[1] || s.res[0] != s.res[2] || s.size[0] != s.size[1] || s.size[0] != s.size[2])
    return "tsdf_hip_merge: src needs cubic voxels on a cubic grid (res and size equal on all axes): getFxn's interpolation assumes them";
  if (dst->p.max_dist_pos != s.max_dist_pos || dst->p.max_dist_neg != s.max_dist_neg)
    return "tsdf_hip_merge: the truncation limits differ (distances are stored divided by max_dist_neg)";
  if (dst->cn[0] || src->cn[0]) return "tsdf_hip_merge: RGB_NORMALIZED / LAB colour state is not supported (TSDF_COLOR_RGB only)";
  if (dst->weight_by_depth || dst->weight_by_variance || src->weight_by_depth || src->weight_by_variance)
    return "tsdf_hip_merge: volumes weighted by depth or by variance are not supported (M_ / nsample_ are not merged)";
  // A PACKED dst keeps w as a count k, w == min(k, max_weight), saturating at kmax = ceil(max_weight).  With src PACKED and
  // the same max_weight both w and w_s are of that form: below max_weight they are small integers, their fp32 sum is exact,
  // and the sum is either an integer < max_weight (the count k + k_s < kmax) or it reaches max_weight and the clamp stores
  // max_weight itself (the count kmax) -- as it does whenever either operand is already max_weight, since w_s > 0.  Every
  // result of the update therefore has a count.  A float-weighted src, or another limit, can give sums no count represents.
  if (dst->packed && !(src->packed && s.max_weight == dst->p.max_weight))
    return "tsdf_hip_merge: a PACKED dst needs a PACKED src with the same max_weight (else a merged weight may have no count); use the F32W layout for dst";
  return nullptr;
}

extern "C" int tsdf_hip_merge(tsdf_handle dst, tsdf_handle src, const double src_from_dst[12], float min_weight, uint64_t *n_merged) {
  if (!dst || !src || !src_from_dst || dst == src || !(min_weight >= 0.f)) return TSDF_HIP_E_INVALID;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(src_from_dst[i])) return TSDF_HIP_E_INVALID;
  if (const char *why = merge_refusal(dst, src)) {
    tsdf_set_error(why);
    return TSDF_HIP_E_UNSUPPORTED;
  }
  {  // a frame that frame pairing holds back in src is part of what the merge reads
    TSDF_ENTER(src);
  }
  TSDF_ENTER(dst);
  if (n_merged) *n_merged = 0;
  int lo[3], hi[3];
  if (!merge_box(dst, src, src_from_dst, lo, hi)) {  // nothing of src reaches dst: nothing is touched
    dst->merge_stats[0] = dst->merge_stats[1] = dst->merge_stats[2] = 0;
    dst->merge_timed = dst->merge_count_pending = false;
    return TSDF_HIP_OK;
  }
  if (const int rc = dst->merge_ev.ensure(3)) return rc;
  if (const int rc = dst->merge_count.reserve(sizeof(unsigned long long), dst->stream)) return rc;
  MergeArgs a;
  for (int i = 0; i < 12; ++i) a.M[i] = (float)src_from_dst[i];
  a.min_weight = min_weight;
  a.x0 = lo[0], a.x1 = hi[0] + 1, a.y0 = lo[1], a.y1 = hi[1] + 1, a.z0 = lo[2];
  a.xa = lo[0] & ~15;
  a.ny = dst->ny, a.pitch = dst->pitch;
  a.d = dst->d, a.w = dst->w, a.rgb = dst->rgb, a.k8 = dst->k8;
  a.wmax = dst->p.max_weight, a.kmax = dst->kmax;
  for (int k = 0; k < 3; ++k) a.ctr[k] = dst->ctr[k];
  const GridView g = make_view(src);
  const dim3 grid((unsigned)((a.x1 - a.xa + 63) / 64), (unsigned)((a.y1 - a.y0 + 3) / 4), (unsigned)(hi[2] - lo[2] + 1)), block(256);
  // everything queued on src's stream so far is read; nothing queued on it later overtakes the read
  TSDF_HIP_TRY(hipEventRecord(dst->merge_ev[2], src->stream));
  TSDF_HIP_TRY(hipStreamWaitEvent(dst->stream, dst->merge_ev[2], 0));
  TSDF_HIP_TRY(hipMemsetAsync(dst->merge_count.p, 0, sizeof(unsigned long long), dst->stream));
  TSDF_HIP_TRY(hipEventRecord(dst->merge_ev[0], dst->stream));
  const bool color = dst->rgb && src->rgb && dst->p.integrate_color && src->p.integrate_color;
  if (dst->packed) {
    if (color)
      hipLaunchKernelGGL((k_merge<true, true>), grid, block, 0, dst->stream, g, a, dst->merge_count.as<unsigned long long>());
    else
      hipLaunchKernelGGL((k_merge<true, false>), grid, block, 0, dst->stream, g, a, dst->merge_count.as<unsigned long long>());
  } else {
    if (color)
      hipLaunchKernelGGL((k_merge<false, true>), grid, block, 0, dst->stream, g, a, dst->merge_count.as<unsigned long long>());
    else
      hipLaunchKernelGGL((k_merge<false, false>), grid, block, 0, dst->stream, g, a, dst->merge_count.as<unsigned long long>());
  }
  TSDF_HIP_TRY(hipGetLastError());
  // Only here, behind everything that can still fail before the kernel is queued: a call that fails earlier leaves dst's record
  // as it was.  Arbitrary distances arrive, as with tsdf_hip_upload: the "band seen" flags no longer describe dst's planes.
  // (The list of tsdf_hip_occupied stays, as after an upload: it names voxels, and their values are gathered when fetched.)
  dst->merge_stats[0] = (uint64_t)(hi[0] - lo[0] + 1) * (uint64_t)(hi[1] - lo[1] + 1) * (uint64_t)(hi[2] - lo[2] + 1);
  dst->merge_stats[1] = 0;
  dst->merge_stats[2] = dst->band_exact ? 1u : 0u;
  dst->band_exact = false;
  dst->merge_timed = dst->merge_count_pending = false;  // (until the second event is recorded)
  TSDF_HIP_TRY(hipEventRecord(dst->merge_ev[1], dst->stream));
  dst->merge_timed = true;
  dst->merge_count_pending = true;
  TSDF_HIP_TRY(hipEventRecord(dst->merge_ev[2], dst->stream));
  TSDF_HIP_TRY(hipStreamWaitEvent(src->stream, dst->merge_ev[2], 0));
  if (n_merged) {
    unsigned long long n = 0;
    TSDF_HIP_TRY(hipMemcpyAsync(&n, dst->merge_count.p, sizeof n, hipMemcpyDeviceToHost, dst->stream));
    TSDF_HIP_TRY(hipStreamSynchronize(dst->stream));
    dst->merge_stats[1] = *n_merged = n;
    dst->merge_count_pending = false;
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_merge_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  out[0] = h->merge_stats[0], out[1] = h->merge_stats[1], out[2] = h->merge_stats[2], out[3] = 0;
  if (h->multi || !h->merge_timed) return TSDF_HIP_OK;
  TSDF_ON_DEVICE(h->device);
  TSDF_HIP_TRY(hipEventSynchronize(h->merge_ev[1]));
  if (h->merge_count_pending) {  // (nothing has been queued on the counter since: the next merge resets this state first)
    unsigned long long n = 0;
    TSDF_HIP_TRY(hipMemcpy(&n, h->merge_count.p, sizeof n, hipMemcpyDeviceToHost));
    h->merge_stats[1] = n;
    h->merge_count_pending = false;
  }
  out[1] = h->merge_stats[1];
  float ms = 0.f;
  TSDF_HIP_TRY(hipEventElapsedTime(&ms, h->merge_ev[0], h->merge_ev[1]));
  out[3] = (uint64_t)(ms * 1000.f);
  return TSDF_HIP_OK;
}
