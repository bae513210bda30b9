// The two per-voxel rules a frame's observation enters and leaves the running averages by, as functions of the voxel's words
// in registers, for the kernel that applies them one after the other (tsdf_reintegrate.hip: k_reintegrate):
//   remove_observation   the rule stated above tsdf_hip_deintegrate in include/tsdf_hip.h: k_deintegrate's
//                        arithmetic, statement for statement
//   add_observation      OctreeNode / RGBNode::addObservation with w_new = 1 (octree.cpp:152-163, 328-337): what
//                        k_integrate_plain<..., BY_DEPTH = false> does to a voxel without a variance state
// Both are RESTATED here: k_deintegrate calling remove_observation compiles to the same instructions in another order, not to
// the same code object, and k_integrate_plain interleaves the two weightings with its update, so those two kernels keep
// their own copies.  tests/test_reintegrate_gpu.py pins these against the oracle and against the two calls.
// Every operation is rounded on its own (-ffp-contract=off); the divisions are the compiler's IEEE ones.
// `old`: the colour word (byte 3: the PACKED count), 0 without colour; k: the PACKED count; w: the weight it stands for, or the
// F32W weight; c: the pixel, PCL memory order b, g, r, a.
#pragma once

#include "tsdf_common.h"

// lowered: w != 0, the voxel is written; cleared: ... and is back at the reset state (d1 = -1, w = 0 / k = 0, c1 = 0);
// d1: the new distance (d itself where it does not move); w1 = W - 1: the F32W weight where !cleared; c1: the new colour
// word, with the PACKED count k - 1 in byte 3.
template <bool COLOR, bool PACKED>
static __device__ __forceinline__ void remove_observation(const float d, const uint32_t old, const unsigned k, const float w, const uint32_t c,
                                                          const float dn, bool &lowered, bool &cleared, float &d1_out, float &w1_out,
                                                          uint32_t &c1_out) {
  lowered = w != 0.f;  // w == 0: nothing is written
  const float W = ceilf(w), w1 = W - 1.f;
  cleared = lowered && w1 <= 0.f;
  float d1 = -1.f;
  uint32_t c1 = 0u;
  if (!cleared) {
    const float num = d * W - dn;
    d1 = __float_as_uint(d) == __float_as_uint(dn) ? d : num / w1;  // a mean of equal values does not move
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
  d1_out = d1, w1_out = w1, c1_out = c1;
}

struct VoxelAdded {
  float d1;      // octree.cpp:156
  float w1;      // :157-159 (the F32W weight)
  unsigned k1;   // the PACKED count min(k + 1, kmax)
  uint32_t c1;   // the new colour word, with k1 in byte 3 (PACKED)
};

template <bool COLOR, bool PACKED>
static __device__ __forceinline__ VoxelAdded add_observation(float d, uint32_t old, unsigned k, float w, uint32_t c, float dn, float wmax,
                                                             unsigned kmax) {
  VoxelAdded r;
  const float wn = 1.f;
  const float wsum = w + wn;
  r.k1 = min(k + 1u, kmax);
  r.c1 = 0u;
  if (COLOR) {  // RGBNode::addObservation, octree.cpp:331-335: the OLD w, static_cast<uint8_t> = cvttss2si & 255
    uint32_t out = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float c_old = (float)((old >> (8 * ch)) & 255u);
      const float c_new = (float)((c >> (16 - 8 * ch)) & 255u);
      const float qv = (w * c_old + wn * c_new) / wsum;
      // x86: NaN and anything outside int32 give INT_MIN, whose low byte is 0; v_cvt_i32_f32 gives 0 for NaN
      const bool in_range = qv > -2147483904.f && qv < 2147483648.f;
      out |= (in_range ? ((uint32_t)(int)qv & 255u) : 0u) << (8 * ch);
    }
    r.c1 = PACKED ? out | (r.k1 << 24) : out;
  }
  r.d1 = (d * w + dn * wn) / wsum;  // octree.cpp:156
  r.w1 = wsum > wmax ? wmax : wsum;  // :157-159
  return r;
}
