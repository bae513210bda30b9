// libtsdf_hip.so -- re-pose a fused frame in one sweep (tsdf_hip_reintegrate; not in the reference).  The definition is stated
// in include/tsdf_hip.h above the entry points and explained in DESIGN.md 3.22: the planes come out, bit for bit, as
// tsdf_hip_deintegrate under the old pose and its planes followed by tsdf_hip_integrate under the new pose and its planes
// leave them.
//
// Both halves select their voxels through plain_observe_at (tsdf_plain_observe.h), each with its own IntegrateArgs: its
// pose, its six cull planes, its own "do the planes bite" verdict.  Voxels are independent of each other, so one lane applies
// the removal rule and then the addition rule (tsdf_voxel_rules.h) to one voxel in registers and stores each word once.
// One lane per voxel column position, x fastest; a wave is 64 consecutive voxels of one row -- one row of one 64 x 4 x 1
// flag cell -- and every thread walks a run of TSDF_REINT_RUN planes: the launch has an eighth of k_deintegrate's workgroups,
// the argument blocks and the row's centres are loaded once per run, and the waves in flight on a SIMD cover
// one another's loads.  g is computed from the centre tables for every voxel (no incremental update along z): the float
// expressions are plain_observe's.  HBM-bound; no LDS, no atomics but the counters', no MFMA.  -ffp-contract=off.
//
// Band flags: a wave stores its cell's flag, 1, where a lane lowers a weight with an in-band observation (k_deintegrate's
// rule, flag_all included, decided from the record as it stood before the call) or observes, under the new pose, a d_new
// whose bits are not the hinge value's.  A voxel observed at exactly p in a flag-0 cell ends at p: by hinge_fixed, or by
// (-1 * 0 + p * 1) / 1 from the reset state.
#include <string.h>

#include <type_traits>
#include <vector>

#include "tsdf_plain_observe.h"
#include "tsdf_voxel_rules.h"

#define TSDF_REINT_RUN 8  // planes per thread (a tuning value: DESIGN.md 3.22)

enum {  // k_reintegrate's counters: five stripes of TSDF_CNT_STRIPE slots in the handle's counter array
  TSDF_RCNT_SELECTED = 0,                   // voxels the old pose selects
  TSDF_RCNT_LOWERED = TSDF_CNT_STRIPE,      // ... whose weight went down (w != 0)
  TSDF_RCNT_CLEARED = 2 * TSDF_CNT_STRIPE,  // ... and, of those, the ones the removal took back to the reset state
  TSDF_RCNT_OBSERVED = 3 * TSDF_CNT_STRIPE, // voxels the new pose brings to addObservation
  TSDF_RCNT_BOTH = 4 * TSDF_CNT_STRIPE,     // voxels both poses select
  TSDF_RCNT_SLOTS = 5 * TSDF_CNT_STRIPE
};

struct ReVoxel {  // one voxel of the z loop: both verdicts, and the words requested for it
  bool so, sn;    // selected by the old pose / observed by the new one
  float dno, dnn; // d_new of either
  float d, w;     // distance; the F32W weight
  uint32_t word;  // the colour word (byte 3: the PACKED count)
  unsigned k8;    // the PACKED count of a volume without colour
  uint32_t co, cn;  // the pixel colours
};

// Grid = (x blocks of 256, rows, ceil(planes / TSDF_REINT_RUN)).  ao / an: the launch arguments of the old / new pose;
// use_old / use_new: 0 where that pose is not finite (it selects nothing).  CULL: a pose's cull planes can bite.
// band: the flags (NULL: the handle's are not exact).
template <int ORDER, bool COLOR, bool PACKED, bool CULL>
static __global__ void __launch_bounds__(256)
k_reintegrate(const IntegrateArgs ao, const IntegrateArgs an_, const int use_old, const int use_new, const int planes,
              float *__restrict__ D, float *__restrict__ Wt, uint32_t *__restrict__ RGB, uint8_t *__restrict__ K8,
              const float *__restrict__ depth, const uint32_t *__restrict__ bgra, const double *__restrict__ cam,
              const float *__restrict__ ctrx, const float *__restrict__ ctry, const float *__restrict__ ctrz,
              uint8_t *__restrict__ band, const int flag_all, unsigned long long *__restrict__ cnt) {
  // The two argument blocks differ in the pose and its cull alone (one handle, one frame size): `an` is ao with those taken
  // from the new pose's block, so that everything else is held once.
  IntegrateArgs an = ao;
#pragma unroll
  for (int i = 0; i < 12; ++i) an.m[i] = an_.m[i];
  an.ref_cull = an_.ref_cull;
#pragma unroll
  for (int i = 0; i < 24; ++i) an.cull[i] = an_.cull[i];
  // !CULL: neither pose's planes can bite (the host's verdict): the 48 plane coefficients stay out of the scalar registers
  if (!CULL) __builtin_assume(ao.ref_cull == 0 && an.ref_cull == 0);
  const int x = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y;
  const int z0 = (int)blockIdx.z * TSDF_REINT_RUN, z1 = min(z0 + TSDF_REINT_RUN, planes);
  const int64_t row = (int64_t)y * ao.pitch + x, plane = (int64_t)ao.plane_rows * ao.pitch;

  // both verdicts, then every word of the voxel requested before the first is looked at.  (A helper on purpose: with these
  // lines written out in the loop the compiler reserves a private segment in two of the sixteen instances.)
  auto fetch = [&](const int zl) {
    ReVoxel v;
    PlainObs oo, on;
    v.so = use_old && plain_observe_at<ORDER>(ao, cam, ctrx, ctry, ctrz, depth, x, y, zl, &oo);
    v.sn = use_new && plain_observe_at<ORDER>(an, cam, ctrx, ctry, ctrz, depth, x, y, zl, &on);
    v.dno = v.so ? oo.dn : 0.f, v.dnn = v.sn ? on.dn : 0.f;
    v.d = v.w = 0.f, v.word = v.k8 = v.co = v.cn = 0u;
    if (v.so || v.sn) {  // (a voxel neither pose selects loads and stores nothing)
      const int64_t vi = (int64_t)(ao.zl0 + zl) * plane + row;
      v.d = D[vi];
      if (COLOR) v.word = RGB[vi];
      if (PACKED && !COLOR) v.k8 = (unsigned)K8[vi];
      if (!PACKED) v.w = Wt[vi];
      if (COLOR && v.so) v.co = bgra[oo.pix];  // PCL memory order b, g, r, a
      if (COLOR && v.sn) v.cn = bgra[on.pix];
    }
    return v;
  };

  unsigned n_sel = 0u, n_low = 0u, n_clr = 0u, n_obs = 0u, n_both = 0u;  // wave-uniform: ballots of this wave over its run
  for (int zl = z0; zl < z1; ++zl) {
    const ReVoxel cur = fetch(zl);
    bool lowered = false, cleared = false, in_band = false;
    if (cur.so || cur.sn) {
      const int64_t vi = (int64_t)(ao.zl0 + zl) * plane + row;
      float d = cur.d;
      uint32_t word = cur.word;
      unsigned k = PACKED ? (COLOR ? word >> 24 : cur.k8) : 0u;
      float w = PACKED ? tsdf_decode_w(k, ao.wmax) : cur.w;
      if (cur.so) {  // the removal rule
        float d1, w1;
        uint32_t c1;
        remove_observation<COLOR, PACKED>(d, word, k, w, cur.co, cur.dno, lowered, cleared, d1, w1, c1);
        in_band = lowered && (flag_all || __float_as_uint(cur.dno) != __float_as_uint(ao.pos_over_neg));
        if (lowered) {
          d = d1, word = c1;
          k = cleared ? 0u : k - 1u;
          w = PACKED ? tsdf_decode_w(k, ao.wmax) : (cleared ? 0.f : w1);
        }
      }
      if (cur.sn) {  // the addition rule, on what the removal left
        const VoxelAdded r = add_observation<COLOR, PACKED>(d, word, k, w, cur.cn, cur.dnn, an.wmax, an.kmax);
        d = r.d1, word = r.c1, k = r.k1, w = r.w1;
        in_band = in_band || __float_as_uint(cur.dnn) != __float_as_uint(an.pos_over_neg);
      }
      if (lowered || cur.sn) {  // each word once
        if (__float_as_uint(d) != __float_as_uint(cur.d)) D[vi] = d;
        if (COLOR) RGB[vi] = word;
        if (PACKED && !COLOR) K8[vi] = (uint8_t)k;
        if (!PACKED) Wt[vi] = w;
      }
    }
    // this wave's 64 voxels lie in ONE flag cell: cell (x >> 6, y >> 2) of the allocated plane (every writer stores the same 1)
    if (band && __ballot(in_band) != 0ull && (threadIdx.x & 63u) == 0u) {
      const int xc = x >> 6, yg = y >> 2;
      if (xc < ao.band_fx && yg < ao.band_fy) band[((int64_t)(ao.zl0 + zl) * ao.band_fy + yg) * ao.band_fx + xc] = 1;
    }
    if (cnt) {
      n_sel += (unsigned)__popcll(__ballot(cur.so)), n_low += (unsigned)__popcll(__ballot(lowered));
      n_clr += (unsigned)__popcll(__ballot(cleared)), n_obs += (unsigned)__popcll(__ballot(cur.sn));
      n_both += (unsigned)__popcll(__ballot(cur.so && cur.sn));
    }
  }
  // one atomic per wave and quantity, into the slot of the block's number (plain_count's scheme)
  if (cnt && (threadIdx.x & 63u) == 0u && (n_sel | n_obs)) {
    const unsigned b = (blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y) & (TSDF_CNT_STRIPE - 1u);
    if (n_sel) atomicAdd(cnt + TSDF_RCNT_SELECTED + b, (unsigned long long)n_sel);
    if (n_low) atomicAdd(cnt + TSDF_RCNT_LOWERED + b, (unsigned long long)n_low);
    if (n_clr) atomicAdd(cnt + TSDF_RCNT_CLEARED + b, (unsigned long long)n_clr);
    if (n_obs) atomicAdd(cnt + TSDF_RCNT_OBSERVED + b, (unsigned long long)n_obs);
    if (n_both) atomicAdd(cnt + TSDF_RCNT_BOTH + b, (unsigned long long)n_both);
  }
}

static const char *reintegrate_refusal(const tsdf_hip_volume *h) {
  if (h->multi) return "tsdf_hip_reintegrate works on ONE handle; a multi-GPU set (tsdf_hip_create_multi) is not supported yet";
  if (h->weight_by_depth || h->weight_by_variance || h->vm || h->vn)
    return "tsdf_hip_reintegrate: volumes weighted by depth or by variance are not supported (the observation's weight and M_ / nsample_ are not kept per frame)";
  if (h->cn[0]) return "tsdf_hip_reintegrate: RGB_NORMALIZED / LAB colour state is not supported (TSDF_COLOR_RGB only)";
  return nullptr;
}

static void set_cull(tsdf_handle h, const float *planes) {  // (what tsdf_hip_set_reference_cull does on one handle)
  h->ref_cull = planes != nullptr;
  for (int i = 0; i < 24; ++i) h->cull_planes[i] = planes ? planes[i] : 0.f;
}

// Queue the kernel over the planes the handle's integrate launches write; planes_new stay in force.  `count`: fill the counters.
static int reintegrate_launch(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float To[12], const float *planes_old,
                              const float Tn[12], const float *planes_new, bool count) {
  // the callers' plane arrays may be the handle's own: work on copies
  float pc[2][24], kept[24];
  const float *po = nullptr, *pn = nullptr;
  if (planes_old) memcpy(pc[0], planes_old, sizeof pc[0]), po = pc[0];
  if (planes_new) memcpy(pc[1], planes_new, sizeof pc[1]), pn = pc[1];
  const bool kept_on = h->ref_cull;
  memcpy(kept, h->cull_planes, sizeof kept);
  IntegrateArgs ao, an;
  unsigned planes = 0;
  h->reint_timed = false;
  set_cull(h, po);  // (ref_cull is decided per pose: only where that pose's planes can bite)
  const bool old_ok = tsdf_plain_launch_args(h, To, &ao, &planes);
  set_cull(h, pn);
  const bool new_ok = tsdf_plain_launch_args(h, Tn, &an, &planes);
  if (count) TSDF_HIP_TRY(hipMemsetAsync(h->counter, 0, TSDF_RCNT_SLOTS * sizeof(unsigned long long), h->stream));
  if ((!old_ok && !new_ok) || !planes) return TSDF_HIP_OK;  // a pose that is not finite selects nothing, as in both calls
  const dim3 grid((unsigned)((h->pitch + 255) / 256), (unsigned)h->ny, (planes + TSDF_REINT_RUN - 1u) / TSDF_REINT_RUN), block(256);
  if (grid.y > 65535u || grid.z > 65535u) {
    set_cull(h, kept_on ? kept : nullptr);
    tsdf_set_error("grid too large for one launch");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  if (const int rc = h->reint_ev.ensure(2)) return rc;
  // the flags are kept only while they describe the planes; whether flag-0 cells rest at this launch's hinge value is read
  // from the record as it stands BEFORE the call (k_deintegrate's flag_all), then the record takes the addition
  uint8_t *band = h->band_exact ? h->band : nullptr;
  uint32_t bits;
  memcpy(&bits, &ao.pos_over_neg, 4);
  const int flag_all = h->rest_state == 1 && h->rest_bits == bits ? 0 : 1;
  if (new_ok) (void)tsdf_plain_implied_distances(h, an, band != nullptr);
  unsigned long long *cnt = count ? h->counter : nullptr;
  const bool sse = h->p.xform_order == TSDF_XFORM_PCL_SSE, color = h->p.integrate_color != 0, packed = h->packed != 0;
  TSDF_HIP_TRY(hipEventRecord(h->reint_ev[0], h->stream));
  const bool cull = ao.ref_cull || an.ref_cull;
  auto launch = [&](auto SSE, auto COLOR, auto PACKED, auto CULL) {
    hipLaunchKernelGGL((k_reintegrate<SSE.value ? TSDF_XFORM_PCL_SSE : TSDF_XFORM_LEFT_TO_RIGHT, COLOR.value, PACKED.value, CULL.value>), grid,
                       block, 0, h->stream, ao, an, old_ok ? 1 : 0, new_ok ? 1 : 0, (int)planes, h->d, h->w, h->rgb, h->k8, d_depth, d_bgra,
                       h->cam64, h->ctr[0], h->ctr[1], h->ctr[2], band, flag_all, cnt);
  };
  auto pick3 = [&](auto SSE, auto COLOR, auto PACKED) {
    if (cull) launch(SSE, COLOR, PACKED, std::true_type{}); else launch(SSE, COLOR, PACKED, std::false_type{});
  };
  auto pick2 = [&](auto SSE, auto COLOR) {
    if (packed) pick3(SSE, COLOR, std::true_type{}); else pick3(SSE, COLOR, std::false_type{});
  };
  auto pick1 = [&](auto SSE) {
    if (color) pick2(SSE, std::true_type{}); else pick2(SSE, std::false_type{});
  };
  if (sse) pick1(std::true_type{}); else pick1(std::false_type{});
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(h->reint_ev[1], h->stream));
  h->reint_timed = true;
  tsdf_esdf_invalidate(h);  // a distance field describes the planes as they were
  return TSDF_HIP_OK;
}

// Synchronising half: the counters of a counting launch (all zero when nothing was launched).
static int reintegrate_collect(tsdf_handle h, uint64_t n[2]) {
  std::vector<unsigned long long> c(TSDF_RCNT_SLOTS);
  TSDF_HIP_TRY(hipMemcpyAsync(c.data(), h->counter, c.size() * sizeof c[0], hipMemcpyDeviceToHost, h->stream));
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  uint64_t sum[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < TSDF_RCNT_SLOTS; ++i) sum[i / TSDF_CNT_STRIPE] += c[i];
  for (int q = 0; q < 5; ++q) h->reint_stats[q] = sum[q];
  n[0] = sum[1], n[1] = sum[3];
  return TSDF_HIP_OK;
}

static int reintegrate_frame(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float To[12], const float *planes_old,
                             const float Tn[12], const float *planes_new, uint64_t *n) {
  h->count_slots = 0;  // (the counter array is this call's now)
  if (n) n[0] = n[1] = 0;
  const int rc = reintegrate_launch(h, d_depth, d_bgra, To, planes_old, Tn, planes_new, n != nullptr);
  if (rc || !n) return rc;
  return reintegrate_collect(h, n);
}

static int reintegrate_check(tsdf_handle h, const void *depth, const void *bgra, const float *To, const float *Tn) {
  if (!h || !depth || !To || !Tn) return TSDF_HIP_E_INVALID;
  if (const char *why = reintegrate_refusal(h)) {
    tsdf_set_error(why);
    return TSDF_HIP_E_UNSUPPORTED;
  }
  if (h->p.integrate_color && !bgra) {
    tsdf_set_error("integrate_color is set but no colour image was given");
    return TSDF_HIP_E_INVALID;
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_reintegrate_device(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float cam_from_vol_old[12],
                                           const float *planes_old, const float cam_from_vol_new[12], const float *planes_new,
                                           uint64_t *n) {
  if (const int rc = reintegrate_check(h, d_depth, d_bgra, cam_from_vol_old, cam_from_vol_new)) return rc;
  TSDF_ENTER(h);
  return reintegrate_frame(h, d_depth, h->p.integrate_color ? d_bgra : nullptr, cam_from_vol_old, planes_old, cam_from_vol_new, planes_new, n);
}

extern "C" int tsdf_hip_reintegrate(tsdf_handle h, const float *depth, const uint8_t *bgra, const float cam_from_vol_old[12],
                                    const float *planes_old, const float cam_from_vol_new[12], const float *planes_new, uint64_t *n) {
  if (const int rc = reintegrate_check(h, depth, bgra, cam_from_vol_old, cam_from_vol_new)) return rc;
  TSDF_ENTER(h);
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  const bool color = h->p.integrate_color != 0;
  h->frame_staged = 0;  // (the upload replaces a frame tsdf_hip_organize staged)
  int rc = tsdf_to_device(h, h->frame_depth, depth, npx * sizeof(float));  // the frame goes up ONCE for both halves
  if (rc) return rc;
  if (color && (rc = tsdf_to_device(h, h->frame_bgra, bgra, npx * 4))) return rc;
  rc = reintegrate_frame(h, h->frame_depth, color ? h->frame_bgra : nullptr, cam_from_vol_old, planes_old, cam_from_vol_new, planes_new, n);
  if (rc) return rc;
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_reintegrate_stats(tsdf_handle h, uint64_t out[6]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  for (int q = 0; q < 5; ++q) out[q] = h->reint_stats[q];
  out[5] = 0;
  if (h->multi || !h->reint_timed) return TSDF_HIP_OK;
  TSDF_ON_DEVICE(h->device);
  TSDF_HIP_TRY(hipEventSynchronize(h->reint_ev[1]));
  float ms = 0.f;
  TSDF_HIP_TRY(hipEventElapsedTime(&ms, h->reint_ev[0], h->reint_ev[1]));
  out[5] = (uint64_t)(ms * 1000.f);
  return TSDF_HIP_OK;
}
