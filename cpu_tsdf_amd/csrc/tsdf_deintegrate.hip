// libtsdf_hip.so -- take a frame back out of the volume (tsdf_hip_deintegrate; not in the reference, whose running
// averages only grow).  The rule is stated in include/tsdf_hip.h above the entry points and explained in DESIGN.md 3.21.
//
// The frame, the pose and the cull planes in force select the voxels through plain_observe (tsdf_plain_observe.h), the very
// code the plain integrate kernels select them with, so the removed observation d_new and its pixel colour are the ones
// integrateCloud used.  One lane per voxel, x fastest; a wave is 64 consecutive voxels of one row: 256 contiguous bytes per
// plane, dword-coalesced.  It moves the words of the general integrate launch -- d, and the colour / count word, the count
// byte or w -- plus one flag byte per wave at most.  HBM-bound; no LDS, no MFMA.  Compiled with -ffp-contract=off: every
// operation below is rounded on its own, and the divisions are the compiler's IEEE ones, as in k_integrate_plain.
//
// The "band seen" flags and the implied-distance record (tsdf_common.h: band_exact, rest_state) survive.  A wave of this
// kernel is one flag cell's row (64 x 1 x 1 of its 64 x 4 x 1 voxels); it stores the cell's flag, 1, when one of its lanes
// lowers a weight with an observation inside the band: d_new off the hinge value p.  (An observation that the division puts
// exactly ON p -- raw == pos -- moves a voxel no differently from one beyond the band, and sets nothing.)  In a cell whose
// flag is 0 every observed voxel holds p's bits, so d_new == p leaves it there (the equal-bits rule), the voxel whose
// weight reaches 0 returns to the reset state, and any other d_new sets the flag: the cell is as the integrate kernels
// would have left it, which is all the readers (k_integrate's implied distances, k_mc_need, tsdf_hip_occupied) assume.
// Where the record does not say that flag-0 cells rest at THIS p (rest_state != 1 or another hinge value: F32W volumes,
// a non-integer max_weight, truncation limits changed since) every lowered weight sets its cell's flag (flag_all).
#include <string.h>

#include <type_traits>

#include "tsdf_plain_observe.h"

enum {  // k_deintegrate's counters: three stripes of TSDF_CNT_STRIPE slots in the handle's counter array
  TSDF_DCNT_SELECTED = 0,                    // voxels the frame selects (what integrate counts as observed)
  TSDF_DCNT_LOWERED = TSDF_CNT_STRIPE,       // ... whose weight went down (w != 0)
  TSDF_DCNT_CLEARED = 2 * TSDF_CNT_STRIPE,   // ... and, of those, the ones back at the reset state
  TSDF_DCNT_SLOTS = 3 * TSDF_CNT_STRIPE
};

// one atomic per wave and quantity, into the slot of the block's number (plain_count's scheme)
static __device__ __forceinline__ void deintegrate_count(bool selected, bool lowered, bool cleared, unsigned long long *__restrict__ cnt) {
  if (!cnt) return;
  const unsigned long long ms = __ballot(selected), ml = __ballot(lowered), mc = __ballot(cleared);
  if ((threadIdx.x & 63u) == 0u && ms) {
    const unsigned b = (blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y) & (TSDF_CNT_STRIPE - 1u);
    atomicAdd(cnt + TSDF_DCNT_SELECTED + b, (unsigned long long)__popcll(ms));
    if (ml) atomicAdd(cnt + TSDF_DCNT_LOWERED + b, (unsigned long long)__popcll(ml));
    if (mc) atomicAdd(cnt + TSDF_DCNT_CLEARED + b, (unsigned long long)__popcll(mc));
  }
}

// Grid = launch_plain_family's: (x blocks of 256, rows, planes).  band: the flags (NULL: the handle's are not exact, none kept).
template <int ORDER, bool COLOR, bool PACKED>
static __global__ void __launch_bounds__(256)
k_deintegrate(const IntegrateArgs a, float *__restrict__ D, float *__restrict__ Wt, uint32_t *__restrict__ RGB,
              uint8_t *__restrict__ K8, const float *__restrict__ depth, const uint32_t *__restrict__ bgra,
              const double *__restrict__ cam, const float *__restrict__ ctrx, const float *__restrict__ ctry,
              const float *__restrict__ ctrz, uint8_t *__restrict__ band, int flag_all, unsigned long long *__restrict__ cnt) {
  PlainObs o;
  const bool selected = plain_observe<ORDER>(a, cam, ctrx, ctry, ctrz, depth, &o);
  bool lowered = false, cleared = false, in_band = false;
  if (selected) {
    const int64_t vi = o.vi;
    // every word of the voxel is requested before the first is looked at
    const float d = D[vi];
    const uint32_t old = COLOR ? RGB[vi] : 0u;  // byte 3: the PACKED count
    const unsigned k = PACKED ? (COLOR ? old >> 24 : (unsigned)K8[vi]) : 0u;
    const float w = PACKED ? tsdf_decode_w(k, a.wmax) : Wt[vi];
    const uint32_t c = COLOR ? bgra[o.pix] : 0u;  // PCL memory order b, g, r, a
    lowered = w != 0.f;  // w == 0: nothing is written
    const float W = ceilf(w), w1 = W - 1.f;
    cleared = lowered && w1 <= 0.f;
    // the new words, worked out by every selected lane and stored under one predicate each at the end
    float d1 = -1.f;
    uint32_t c1 = 0u;
    if (!cleared) {
      const float num = d * W - o.dn;
      d1 = __float_as_uint(d) == __float_as_uint(o.dn) ? d : num / w1;  // a mean of equal values does not move
      if (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float c_old = (float)((old >> (8 * ch)) & 255u);
          const float c_obs = (float)((c >> (16 - 8 * ch)) & 255u);
          const float x = (W * c_old - c_obs) / w1;
          // nearest: the forward update truncated, a second truncation would bias dark
          c1 |= (uint32_t)(int)(fminf(fmaxf(x, 0.f), 255.f) + 0.5f) << (8 * ch);
        }
        if (PACKED) c1 |= (k - 1u) << 24;
      }
    }
    in_band = lowered && (flag_all || __float_as_uint(o.dn) != __float_as_uint(a.pos_over_neg));
    if (lowered) {
      if (__float_as_uint(d1) != __float_as_uint(d)) D[vi] = d1;
      if (COLOR) RGB[vi] = c1;
      if (PACKED && !COLOR) K8[vi] = cleared ? (uint8_t)0 : (uint8_t)(k - 1u);
      if (!PACKED) Wt[vi] = cleared ? 0.f : w1;
    }
  }
  // this wave's 64 voxels lie in ONE flag cell: cell (x >> 6, y >> 2) of the allocated plane (every writer stores the same 1)
  if (band && __ballot(in_band) != 0ull && (threadIdx.x & 63u) == 0u) {
    const int xc = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), yg = (int)blockIdx.y >> 2;
    if (xc < a.band_fx && yg < a.band_fy) band[((int64_t)(a.zl0 + (int)blockIdx.z) * a.band_fy + yg) * a.band_fx + xc] = 1;
  }
  deintegrate_count(selected, lowered, cleared, cnt);
}

static const char *deintegrate_refusal(const tsdf_hip_volume *h) {
  if (h->multi) return "tsdf_hip_deintegrate works on ONE handle; a multi-GPU set (tsdf_hip_create_multi) is not supported yet";
  if (h->weight_by_depth || h->weight_by_variance || h->vm || h->vn)
    return "tsdf_hip_deintegrate: volumes weighted by depth or by variance are not supported (the observation's weight and M_ / nsample_ are not kept per frame)";
  if (h->cn[0]) return "tsdf_hip_deintegrate: RGB_NORMALIZED / LAB colour state is not supported (TSDF_COLOR_RGB only)";
  return nullptr;
}

// Queue the kernel over the planes the handle's integrate launches write.  `count`: fill the counters.
static int deintegrate_launch(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float T[12], bool count) {
  IntegrateArgs a;
  unsigned planes = 0;
  h->deint_timed = false;
  const bool pose_ok = tsdf_plain_launch_args(h, T, &a, &planes);
  if (count) TSDF_HIP_TRY(hipMemsetAsync(h->counter, 0, TSDF_DCNT_SLOTS * sizeof(unsigned long long), h->stream));
  if (!pose_ok || !planes) return TSDF_HIP_OK;  // a pose that is not finite observes nothing, as in integrate
  const dim3 grid((unsigned)((h->pitch + 255) / 256), (unsigned)h->ny, planes), block(256);
  if (grid.y > 65535u || grid.z > 65535u) {
    tsdf_set_error("grid too large for one launch");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  if (const int rc = h->deint_ev.ensure(2)) return rc;
  // the flags are kept only while they describe the planes; flag-0 cells rest at this launch's hinge value only if the
  // record says so (see the head of this file)
  uint8_t *band = h->band_exact ? h->band : nullptr;
  uint32_t bits;
  memcpy(&bits, &a.pos_over_neg, 4);
  const int flag_all = h->rest_state == 1 && h->rest_bits == bits ? 0 : 1;
  unsigned long long *cnt = count ? h->counter : nullptr;
  const bool sse = h->p.xform_order == TSDF_XFORM_PCL_SSE, color = h->p.integrate_color != 0, packed = h->packed != 0;
  TSDF_HIP_TRY(hipEventRecord(h->deint_ev[0], h->stream));
  auto launch = [&](auto SSE, auto COLOR, auto PACKED) {
    hipLaunchKernelGGL((k_deintegrate<SSE.value ? TSDF_XFORM_PCL_SSE : TSDF_XFORM_LEFT_TO_RIGHT, COLOR.value, PACKED.value>), grid, block, 0,
                       h->stream, a, h->d, h->w, h->rgb, h->k8, d_depth, d_bgra, h->cam64, h->ctr[0], h->ctr[1], h->ctr[2], band,
                       flag_all, cnt);
  };
  auto pick2 = [&](auto SSE, auto COLOR) {
    if (packed) launch(SSE, COLOR, std::true_type{}); else launch(SSE, COLOR, std::false_type{});
  };
  auto pick1 = [&](auto SSE) {
    if (color) pick2(SSE, std::true_type{}); else pick2(SSE, std::false_type{});
  };
  if (sse) pick1(std::true_type{}); else pick1(std::false_type{});
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(h->deint_ev[1], h->stream));
  h->deint_timed = true;
  tsdf_esdf_invalidate(h);  // a distance field describes the planes as they were
  return TSDF_HIP_OK;
}

// Synchronising half: the counters of a counting launch (all zero when nothing was launched).
static int deintegrate_collect(tsdf_handle h, uint64_t *n_removed) {
  unsigned long long c[TSDF_DCNT_SLOTS];
  TSDF_HIP_TRY(hipMemcpyAsync(c, h->counter, sizeof c, hipMemcpyDeviceToHost, h->stream));
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  uint64_t sum[3] = {0, 0, 0};
  for (int i = 0; i < TSDF_DCNT_SLOTS; ++i) sum[i / TSDF_CNT_STRIPE] += c[i];
  for (int q = 0; q < 3; ++q) h->deint_stats[q] = sum[q];
  *n_removed = sum[1];
  return TSDF_HIP_OK;
}

static int deintegrate_frame(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float T[12], uint64_t *n_removed) {
  h->count_slots = 0;  // (the counter array is this call's now)
  if (n_removed) *n_removed = 0;
  const int rc = deintegrate_launch(h, d_depth, d_bgra, T, n_removed != nullptr);
  if (rc || !n_removed) return rc;
  return deintegrate_collect(h, n_removed);
}

static int deintegrate_check(tsdf_handle h, const void *depth, const void *bgra, const float *T) {
  if (!h || !depth || !T) return TSDF_HIP_E_INVALID;
  if (const char *why = deintegrate_refusal(h)) {
    tsdf_set_error(why);
    return TSDF_HIP_E_UNSUPPORTED;
  }
  if (h->p.integrate_color && !bgra) {
    tsdf_set_error("integrate_color is set but no colour image was given");
    return TSDF_HIP_E_INVALID;
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_deintegrate_device(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float cam_from_vol[12],
                                           uint64_t *n_removed) {
  if (const int rc = deintegrate_check(h, d_depth, d_bgra, cam_from_vol)) return rc;
  TSDF_ENTER(h);
  return deintegrate_frame(h, d_depth, h->p.integrate_color ? d_bgra : nullptr, cam_from_vol, n_removed);
}

extern "C" int tsdf_hip_deintegrate(tsdf_handle h, const float *depth, const uint8_t *bgra, const float cam_from_vol[12],
                                    uint64_t *n_removed) {
  if (const int rc = deintegrate_check(h, depth, bgra, cam_from_vol)) return rc;
  TSDF_ENTER(h);
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  const bool color = h->p.integrate_color != 0;
  h->frame_staged = 0;  // (the upload replaces a frame tsdf_hip_organize staged)
  int rc = tsdf_to_device(h, h->frame_depth, depth, npx * sizeof(float));
  if (rc) return rc;
  if (color && (rc = tsdf_to_device(h, h->frame_bgra, bgra, npx * 4))) return rc;
  rc = deintegrate_frame(h, h->frame_depth, color ? h->frame_bgra : nullptr, cam_from_vol, n_removed);
  if (rc) return rc;
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_deintegrate_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  out[0] = h->deint_stats[0], out[1] = h->deint_stats[1], out[2] = h->deint_stats[2], out[3] = 0;
  if (h->multi || !h->deint_timed) return TSDF_HIP_OK;
  TSDF_ON_DEVICE(h->device);
  TSDF_HIP_TRY(hipEventSynchronize(h->deint_ev[1]));
  float ms = 0.f;
  TSDF_HIP_TRY(hipEventElapsedTime(&ms, h->deint_ev[0], h->deint_ev[1]));
  out[3] = (uint64_t)(ms * 1000.f);
  return TSDF_HIP_OK;
}
