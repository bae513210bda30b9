// libtsdf_hip.so -- decimating a triangle mesh by vertex clustering (Rossignac-Borrel).
//
// An extension with no counterpart in the reference.  cpu_tsdf::mesh_post::decimateArrays (csrc/prog/mesh_post.h) defines the
// result as one sequential pass, and this file reproduces it bit for bit:
//   1. a finite vertex belongs to the cell floor((double)v / (double)cell_size) per axis, and the vertices of a cell are one
//      cluster; a vertex that is not finite is a cluster of its own; a cell outside [-2^20, 2^20) is refused;
//   2. clusters are numbered by their lowest member;
//   3. a cluster of one keeps its vertex bit for bit; otherwise a double sum from +0.0, one add per member in ascending
//      index, is divided by (double)count and rounded to float once;
//   4. the colour is (2 * sum + count) / (2 * count) per channel, in integers;
//   5. faces go through remap, a face with two equal corners goes, and of the faces with the same three corners the one
//      with the lowest index stays, as it is.
// Kernels:
//   k_dc_key       the cell key per vertex (MP_NO_KEY when it is not finite); raises a flag for a cell out of range
//   rocprim sort   (key, vertex) pairs, stable: the members of a cluster are contiguous and ascend
//   k_dc_heads     the head of a segment is the cluster's first vertex: a flag per INPUT vertex, whose exclusive scan is
//                  rule 2 without a second sort
//   k_dc_reduce    one lane per cluster walks its segment: rules 3 and 4 and remap.  The adds are exactly the host's, in the
//                  host's order -- a tree or atomics would round differently.
//   k_dc_faces     per face: the remapped corners, the degenerate flag, and the sorted triple as two sort keys
//   rocprim sort   twice, stable, least significant key first (the highest corner, then lowest << b | middle with the
//                  degenerate flag on top, b = bits of the cluster count): equal triples are contiguous, lowest face first
//   k_dc_keep      the head of a run of equal triples survives; mp_compact_faces (scan + k_mp_compact) keeps the order
// The cell key, the face remap, the working set, the handle-less call and the indexed mesh of a handle are shared with the
// other two mesh passes (tsdf_meshgrid.h / .hip).
// Cost of k_dc_reduce: a lane's time is its cluster's size, and a wave's that of its largest cluster.  A marched mesh has tens
// to a few hundred members per cluster (56 at most at a cell of 2 voxels, 175 at 4, on the 32^3 test scene); a cell size that
// puts ALL vertices into one cell makes ONE lane walk the whole mesh, as slow as the host pass and in one launch.
// Gather-bound walks and radix sorts: no MFMA, no LDS.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "tsdf_meshgrid.h"

#define DC_C_RANGE 0     // != 0: a finite vertex lies in a cell outside [-2^20, 2^20)
#define DC_C_BAD 1       // != 0: a face names a vertex >= n_verts
#define DC_C_CLUSTERS 2
#define DC_C_NONDEG 3    // faces with three different corners
#define DC_C_KEPT 4
static_assert(DC_C_KEPT < MP_IDX_COUNTERS, "the counters of a handle's indexed-mesh passes share one allocation");

static thread_local MpStats g_dc_stats;  // tsdf_hip_mesh_decimate_stats

// ---- kernels ---------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_dc_key(const float *__restrict__ verts, uint32_t n, double cell, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
         unsigned long long *__restrict__ counters) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n) return;
  bool out = false;
  keys[v] = mp_cell_key(verts[3ull * v], verts[3ull * v + 1ull], verts[3ull * v + 2ull], cell, out);
  if (out) counters[DC_C_RANGE] = 1ull;  // (every writer stores the same 1; the mesh is refused, whatever its keys hold)
  idx[v] = v;
}

// does a segment begin at sorted position i?  (A vertex that is not finite is a segment of its own.)
static __device__ __forceinline__ bool dc_head(const uint64_t *__restrict__ keys, uint32_t i) {
  const uint64_t key = keys[i];
  return i == 0u || key == MP_NO_KEY || keys[i - 1u] != key;
}

static __global__ void __launch_bounds__(256)
k_dc_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ order, uint32_t n, uint8_t *__restrict__ first,
           unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool head = false;
  if (i < n) {
    head = dc_head(keys, i);
    first[order[i]] = head ? 1 : 0;  // the sort is stable: a segment's head is its lowest vertex
  }
  mp_wave_count(head, &counters[DC_C_CLUSTERS]);
}

// outidx: the exclusive scan of `first` over the input vertices (rule 2).  One lane per cluster.
static __global__ void __launch_bounds__(256)
k_dc_reduce(const float *__restrict__ verts, const uint8_t *__restrict__ rgb, const uint64_t *__restrict__ keys,
            const uint32_t *__restrict__ order, uint32_t n, const uint32_t *__restrict__ outidx, uint32_t *__restrict__ remap,
            float *__restrict__ out_verts, uint8_t *__restrict__ out_rgb, uint32_t *__restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !dc_head(keys, i)) return;
  const uint64_t key = keys[i];
  const uint32_t v0 = order[i], o = outidx[v0];
  double s[3] = {0.0, 0.0, 0.0};
  unsigned long long c[3] = {0ull, 0ull, 0ull};
  uint32_t cnt = 0u, j = i;
  do {
    const uint64_t v = order[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += (double)verts[3ull * v + k];
    if (rgb) {
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] += rgb[3ull * v + k];
    }
    remap[v] = o;
    ++cnt;
    ++j;
  } while (j < n && key != MP_NO_KEY && keys[j] == key);
  counts[o] = cnt;
  if (cnt == 1u) {  // the bits, NaN payloads and -0.0 included
    const uint32_t *src = (const uint32_t *)verts + 3ull * v0;
    uint32_t *dst = (uint32_t *)out_verts + 3ull * o;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_verts[3ull * o + k] = (float)(s[k] / (double)cnt);
  }
  if (rgb) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_rgb[3ull * o + k] = (uint8_t)((2ull * c[k] + cnt) / (2ull * cnt));
  }
}

// Rule 5, first half.  A face with three different corners r gets the sort keys hi = max r and lo << b | mid (every corner is
// below 2^b); a degenerate one only bit 2 b of the second key, which puts it behind all others.
static __global__ void __launch_bounds__(256)
k_dc_faces(const uint32_t *__restrict__ faces, uint32_t n_faces, uint64_t n_verts, const uint32_t *__restrict__ remap, unsigned b,
           uint32_t *__restrict__ mapped, uint64_t *__restrict__ key_lm, uint32_t *__restrict__ key_hi, uint32_t *__restrict__ ord,
           unsigned long long *__restrict__ counters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  bool good = false;
  if (f < n_faces) {
    uint32_t r[3];
    good = mp_face_remap(faces, f, n_verts, remap, mapped, r, &counters[DC_C_BAD]);
    const uint32_t lo = min(r[0], min(r[1], r[2])), hi = max(r[0], max(r[1], r[2])), mid = (uint32_t)(((uint64_t)r[0] + r[1] + r[2]) - lo - hi);
    key_lm[f] = good ? ((uint64_t)lo << b) | (uint64_t)mid : 1ull << (2u * b);
    key_hi[f] = good ? hi : 0u;
    ord[f] = f;
  }
  mp_wave_count(good, &counters[DC_C_NONDEG]);
}

// the second key in the order the first sort left
static __global__ void __launch_bounds__(256)
k_dc_gather_key(const uint64_t *__restrict__ key_lm, const uint32_t *__restrict__ ord, uint32_t n_faces, uint64_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n_faces) out[i] = key_lm[ord[i]];
}

static __device__ __forceinline__ uint32_t dc_hi(const uint32_t *__restrict__ mapped, uint32_t f) {
  return max(mapped[3ull * f], max(mapped[3ull * f + 1ull], mapped[3ull * f + 2ull]));
}

// Rule 5, second half, per sorted position: the first face of a run of equal triples survives (both sorts are stable: it is
// the one with the lowest index).
static __global__ void __launch_bounds__(256)
k_dc_keep(const uint64_t *__restrict__ key_lm, const uint32_t *__restrict__ ord, const uint32_t *__restrict__ mapped, uint32_t n_faces,
          unsigned b, uint8_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool k = false;
  if (i < n_faces) {
    const uint64_t key = key_lm[i];
    const uint32_t f = ord[i];
    if (!(key >> (2u * b))) k = i == 0u || key_lm[i - 1u] != key || dc_hi(mapped, ord[i - 1u]) != dc_hi(mapped, f);
    keep[f] = k ? 1 : 0;
  }
  mp_wave_count(k, &counters[DC_C_KEPT]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct DcLayout {
  // MpWork::buf.  What the caller reads afterwards comes first; the arrays of the vertex phase and those of the face phase,
  // which begins when the former are dead, share the rest.
  size_t remap, mapped, faces, keep, offset, tmp, tmp_bytes;
  size_t key_a, key_b, idx_a, idx_b, first, outidx;            // vertex phase
  size_t key_lm, lm_a, lm_b, hi_a, hi_b, ord_a, ord_b, total;  // face phase
  // MpWork::cells, sized once the number of clusters is known: the output vertices
  size_t c_rgb, c_counts, c_total;
};

static int dc_layout(size_t n, size_t f, hipStream_t s, DcLayout &L) {
  if (const int rc = mp_tmp_bytes(std::max(n, f), f, 0, std::max(n, f), s, &L.tmp_bytes)) return rc;
  MpTake take;
  L.remap = take(n * 4), L.mapped = take(f * 12), L.faces = take(f * 12), L.keep = take(f), L.offset = take(f * 4);
  L.tmp = take(L.tmp_bytes);
  const size_t shared = take.o;
  L.key_a = take(n * 8), L.key_b = take(n * 8), L.idx_a = take(n * 4), L.idx_b = take(n * 4), L.first = take(n), L.outidx = take(n * 4);
  const size_t end_v = take.o;
  take.o = shared;
  L.key_lm = take(f * 8), L.lm_a = take(f * 8), L.lm_b = take(f * 8), L.hi_a = take(f * 4), L.hi_b = take(f * 4), L.ord_a = take(f * 4),
  L.ord_b = take(f * 4);
  L.total = std::max(end_v, take.o);
  return TSDF_HIP_OK;
}

static std::string dc_extent_text(const char *who, float cell_size) {
  return std::string(who) + ": a vertex lies outside the 2^21 cells per axis the cell key holds: |coordinate| must stay below 2^20 * cell_size = " +
         std::to_string(1048576.0 * (double)cell_size);
}

// The whole pass on device arrays.  Leaves in MpWork::buf: remap (n_verts), the surviving faces (L.faces, *n_kept x 3), the
// faces' keep flags and offsets; in MpWork::cells: the *n_out output vertices, their colours (d_rgb != NULL) and member
// counts; and the stats of the calling thread.  Leaves the stream idle.
static int dc_core(MpWork &w, hipStream_t s, const float *d_verts, const uint8_t *d_rgb, uint64_t n_verts, const uint32_t *d_faces, uint64_t n_faces,
                   float cell_size, DcLayout &L, uint64_t *n_out, uint64_t *n_kept, const char *who) {
  const uint32_t n = (uint32_t)n_verts, nf = (uint32_t)n_faces;
  int rc = dc_layout(n, nf, s, L);
  if (rc || (rc = w.buf.reserve(L.total, s, "mesh decimate")) || (rc = mp_work_begin(w, MP_IDX_COUNTERS, 2, s))) return rc;
  char *b = (char *)w.buf.p;
  uint64_t *key_a = (uint64_t *)(b + L.key_a), *keys = (uint64_t *)(b + L.key_b);
  uint32_t *idx_a = (uint32_t *)(b + L.idx_a), *order = (uint32_t *)(b + L.idx_b), *outidx = (uint32_t *)(b + L.outidx);
  uint32_t *remap = (uint32_t *)(b + L.remap), *mapped = (uint32_t *)(b + L.mapped), *faces_out = (uint32_t *)(b + L.faces);
  uint32_t *offset = (uint32_t *)(b + L.offset);
  uint8_t *first = (uint8_t *)(b + L.first), *keep = (uint8_t *)(b + L.keep);
  const dim3 blk(256), grid_n((n + 255u) / 256u), grid_f((nf + 255u) / 256u);

  TSDF_HIP_TRY(hipEventRecord(w.ev[0], s));
  hipLaunchKernelGGL(k_dc_key, grid_n, blk, 0, s, d_verts, n, (double)cell_size, key_a, idx_a, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  size_t tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::radix_sort_pairs(b + L.tmp, tmp_bytes, key_a, keys, idx_a, order, (size_t)n, 0u, 64u, s));
  hipLaunchKernelGGL(k_dc_heads, grid_n, blk, 0, s, keys, order, n, first, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::exclusive_scan(b + L.tmp, tmp_bytes, MpKeepIt(first, MpKeepCount()), outidx, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
  // the range flag and the cluster count in one read
  unsigned long long counts[MP_IDX_COUNTERS] = {0};
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  if (counts[DC_C_RANGE]) {
    tsdf_set_error(dc_extent_text(who, cell_size));
    return TSDF_HIP_E_INVALID;
  }
  const uint64_t m = counts[DC_C_CLUSTERS];
  if (m == 0 || m > n) {
    tsdf_set_error(std::string(who) + ": " + std::to_string(m) + " clusters of " + std::to_string(n) + " vertices (this cannot happen)");
    return TSDF_HIP_E_HIP;
  }
  L.c_rgb = mp_up((size_t)m * 12), L.c_counts = L.c_rgb + mp_up((size_t)m * 3), L.c_total = L.c_counts + mp_up((size_t)m * 4);
  if ((rc = w.cells.reserve(L.c_total, s, "mesh decimate"))) return rc;
  char *c = (char *)w.cells.p;
  hipLaunchKernelGGL(k_dc_reduce, grid_n, blk, 0, s, d_verts, d_rgb, keys, order, n, outidx, remap, (float *)c, (uint8_t *)(c + L.c_rgb),
                     (uint32_t *)(c + L.c_counts));
  TSDF_HIP_TRY(hipGetLastError());
  if (nf) {
    unsigned bits = 1u;  // every output index is below 2^bits
    while (bits < 32u && ((uint64_t)1 << bits) < m) ++bits;
    uint64_t *key_lm = (uint64_t *)(b + L.key_lm), *lm_a = (uint64_t *)(b + L.lm_a), *lm_b = (uint64_t *)(b + L.lm_b);
    uint32_t *hi_a = (uint32_t *)(b + L.hi_a), *hi_b = (uint32_t *)(b + L.hi_b), *ord_a = (uint32_t *)(b + L.ord_a), *ord_b = (uint32_t *)(b + L.ord_b);
    hipLaunchKernelGGL(k_dc_faces, grid_f, blk, 0, s, d_faces, nf, n_verts, remap, bits, mapped, key_lm, hi_a, ord_a, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    // The sorts read only the bits that can be set.  The temporary storage was sized for all bits; should fewer bits ever ask
    // for more of it, all bits are sorted (the upper ones are zero: the same order).
    unsigned bits_hi = bits, bits_lm = 2u * bits + 1u;
    size_t need_hi = 0, need_lm = 0;
    TSDF_HIP_TRY(rocprim::radix_sort_pairs(nullptr, need_hi, hi_a, hi_b, ord_a, ord_b, (size_t)nf, 0u, bits_hi, s));
    TSDF_HIP_TRY(rocprim::radix_sort_pairs(nullptr, need_lm, lm_a, lm_b, ord_b, ord_a, (size_t)nf, 0u, bits_lm, s));
    if (need_hi > L.tmp_bytes) bits_hi = 32u;
    if (need_lm > L.tmp_bytes) bits_lm = 64u;
    tmp_bytes = L.tmp_bytes;
    TSDF_HIP_TRY(rocprim::radix_sort_pairs(b + L.tmp, tmp_bytes, hi_a, hi_b, ord_a, ord_b, (size_t)nf, 0u, bits_hi, s));
    hipLaunchKernelGGL(k_dc_gather_key, grid_f, blk, 0, s, key_lm, ord_b, nf, lm_a);
    TSDF_HIP_TRY(hipGetLastError());
    tmp_bytes = L.tmp_bytes;
    TSDF_HIP_TRY(rocprim::radix_sort_pairs(b + L.tmp, tmp_bytes, lm_a, lm_b, ord_b, ord_a, (size_t)nf, 0u, bits_lm, s));
    hipLaunchKernelGGL(k_dc_keep, grid_f, blk, 0, s, lm_b, ord_a, mapped, nf, bits, keep, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    if ((rc = mp_compact_faces(s, b + L.tmp, L.tmp_bytes, mapped, keep, offset, nf, faces_out))) return rc;
  }
  TSDF_HIP_TRY(hipEventRecord(w.ev[1], s));
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  if (counts[DC_C_BAD]) {
    tsdf_set_error(std::string(who) + ": a face names a vertex index >= n_verts");
    return TSDF_HIP_E_INVALID;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
  g_dc_stats.set(n, m, counts[DC_C_NONDEG] - counts[DC_C_KEPT], (uint64_t)(ms * 1000.f));
  *n_out = m;
  *n_kept = counts[DC_C_KEPT];
  return TSDF_HIP_OK;
}

static int dc_check_args(float cell_size, uint64_t n_verts, uint64_t n_faces, const char *who) {
  if (!(cell_size > 0.f) || !std::isfinite(cell_size)) {
    tsdf_set_error(std::string(who) + ": cell_size must be finite and positive");
    return TSDF_HIP_E_INVALID;
  }
  return mp_check_counts(who, n_faces, &n_verts);
}

// tsdf_hip_mesh_decimate, and for a set also the faces' keep flags (n_faces bytes; nullable)
static int dc_mesh(int device, const float *verts, const uint8_t *rgb, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces, float cell_size,
                   uint32_t *remap, float *out_verts, uint8_t *out_rgb, uint32_t *counts, uint64_t *n_out_verts, uint32_t *out_faces,
                   uint64_t *n_out_faces, uint8_t *keep) {
  const char *who = "tsdf_hip_mesh_decimate";
  if (n_out_verts) *n_out_verts = 0;
  if (n_out_faces) *n_out_faces = 0;
  if (const int rc = dc_check_args(cell_size, n_verts, n_faces, who)) return rc;
  if (device < 0) return TSDF_HIP_E_INVALID;
  if ((n_verts && !verts) || ((out_verts || out_rgb || counts) && !n_out_verts) || (out_faces && !n_out_faces) || (out_rgb && !rgb && n_verts)) {
    tsdf_set_error("tsdf_hip_mesh_decimate: verts must not be NULL, out_rgb needs rgb, and out_verts / out_rgb / counts / out_faces need "
                   "n_out_verts / n_out_faces");
    return TSDF_HIP_E_INVALID;
  }
  if (!faces && n_verts / 3 < n_faces) {
    tsdf_set_error("tsdf_hip_mesh_decimate: a triangle soup needs 3 vertices per face");
    return TSDF_HIP_E_INVALID;
  }
  if (n_verts == 0) {
    if (n_faces) {
      tsdf_set_error("tsdf_hip_mesh_decimate: a face names a vertex index >= n_verts");
      return TSDF_HIP_E_INVALID;
    }
    g_dc_stats.zero();
    return TSDF_HIP_OK;
  }
  MpCall c;
  const size_t b_verts = mp_up((size_t)n_verts * 12), b_rgb = rgb ? mp_up((size_t)n_verts * 3) : 0, b_faces = faces ? (size_t)n_faces * 12 : 0;
  int rc = c.open(device, b_verts + b_rgb + b_faces, who);
  if (rc) return rc;
  float *d_verts = (float *)c.in.p;
  uint8_t *d_rgb = rgb ? (uint8_t *)c.in.p + b_verts : nullptr;
  uint32_t *d_faces = faces && n_faces ? (uint32_t *)((char *)c.in.p + b_verts + b_rgb) : nullptr;
  if ((rc = c.upload(d_verts, verts, (size_t)n_verts * 12)) || (d_rgb && (rc = c.upload(d_rgb, rgb, (size_t)n_verts * 3))) ||
      (d_faces && (rc = c.upload(d_faces, faces, b_faces))))
    return rc;
  DcLayout L;
  uint64_t m = 0, kept = 0;
  if ((rc = dc_core(c.work, c.s, d_verts, d_rgb, n_verts, d_faces, n_faces, cell_size, L, &m, &kept, who))) return rc;
  const char *b = (const char *)c.work.buf.p, *o = (const char *)c.work.cells.p;
  if (remap && (rc = c.download(remap, b + L.remap, (size_t)n_verts * 4))) return rc;
  if (out_verts && (rc = c.download(out_verts, o, (size_t)m * 12))) return rc;
  if (out_rgb && (rc = c.download(out_rgb, o + L.c_rgb, (size_t)m * 3))) return rc;
  if (counts && (rc = c.download(counts, o + L.c_counts, (size_t)m * 4))) return rc;
  if (out_faces && (rc = c.download(out_faces, b + L.faces, (size_t)kept * 12))) return rc;
  if (keep && n_faces && (rc = c.download(keep, b + L.keep, (size_t)n_faces))) return rc;
  if (n_out_verts) *n_out_verts = m;
  if (n_out_faces) *n_out_faces = kept;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_decimate(int device, const float *verts, const uint8_t *rgb, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces,
                                      float cell_size, uint32_t *remap, float *out_verts, uint8_t *out_rgb, uint32_t *counts, uint64_t *n_out_verts,
                                      uint32_t *out_faces, uint64_t *n_out_faces) {
  return dc_mesh(device, verts, rgb, n_verts, faces, n_faces, cell_size, remap, out_verts, out_rgb, counts, n_out_verts, out_faces, n_out_faces,
                 nullptr);
}

// A set: the merged soup is on the host, so it takes the host-array route on the first slab's device, and the indexed mesh
// stays on the host too -- what one handle holding the whole grid would fetch.
static int dc_multi(tsdf_handle h, tsdf_flatten_state *st, float cell_size) {
  const uint64_t n = h->mc_ntri;
  const float *verts = nullptr;
  const uint8_t *rgb = nullptr;
  const uint64_t *cell = nullptr;
  tsdf_multi_mesh(h, &verts, &rgb, &cell);
  std::vector<uint8_t> keep((size_t)n);
  st->h_verts.resize((size_t)n * 9);
  st->h_rgb.resize(rgb ? (size_t)n * 9 : 0);
  st->h_faces.resize((size_t)n * 3);
  uint64_t m = 0, kept = 0;
  const int rc = dc_mesh(tsdf_multi_first(h)->device, verts, rgb, 3 * n, nullptr, n, cell_size, nullptr, st->h_verts.data(),
                         rgb ? st->h_rgb.data() : nullptr, nullptr, &m, st->h_faces.data(), &kept, keep.data());
  if (rc) return rc;
  mp_idx_set_host(st, rgb != nullptr, cell, n, m, kept, keep.data());
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_march_decimate(tsdf_handle h, float cell_size, uint64_t *n_verts, uint64_t *n_faces) {
  const char *who = "tsdf_hip_march_decimate";
  if (!h) return TSDF_HIP_E_INVALID;
  if (n_verts) *n_verts = 0;
  if (n_faces) *n_faces = 0;
  tsdf_flatten_state *st = nullptr;
  uint64_t n = 0;
  int rc = dc_check_args(cell_size, 0, 0, who);
  if (rc || (rc = mp_idx_begin(h, who, &st, &n))) return rc;
  if (!n) {
    g_dc_stats.zero();
  } else if (h->multi) {
    if ((rc = dc_multi(h, st, cell_size))) return rc;
  } else {
    TSDF_ENTER(h);
    DcLayout L;
    uint64_t m = 0, kept = 0;
    const uint8_t *d_rgb = h->mc_has_rgb ? h->mc_rgb.as<uint8_t>() : nullptr;
    if ((rc = dc_core(st->work, h->stream, h->mc_verts.as<float>(), d_rgb, 3 * n, nullptr, n, cell_size, L, &m, &kept, who))) return rc;
    if ((rc = mp_idx_layout(h, st, m, kept, "mesh decimate"))) return rc;
    const char *b = (const char *)st->work.buf.p, *c = (const char *)st->work.cells.p;
    char *o = (char *)st->out.p;
    TSDF_HIP_TRY(hipMemcpyAsync(o, c, (size_t)m * 12, hipMemcpyDeviceToDevice, h->stream));
    if (d_rgb) TSDF_HIP_TRY(hipMemcpyAsync(o + st->o_rgb, c + L.c_rgb, (size_t)m * 3, hipMemcpyDeviceToDevice, h->stream));
    if ((rc = mp_idx_fill(h, st, m, kept, (const uint32_t *)(b + L.faces), (const uint8_t *)(b + L.keep), (const uint32_t *)(b + L.offset)))) return rc;
  }
  return mp_idx_end(st, n_verts, n_faces);
}

extern "C" int tsdf_hip_mesh_decimate_stats(uint64_t out[4]) {
  return g_dc_stats.copy_out(out);
}
