// libtsdf_hip.so -- smoothing an indexed triangle mesh: Taubin's lambda | mu (umbrella operator, uniform weights, Jacobi steps).
//
// An extension with no counterpart in the reference.  cpu_tsdf::mesh_post::smoothArrays (csrc/prog/mesh_post.h) defines the
// result as one sequential pass, and this file reproduces it bit for bit:
//   1. N(i) = the j != i that share a face with i, ascending; deg(i) = |N(i)|;
//   2. the multiplicity of the edge {a, b}, a != b, is the number of corner pairs (0,1), (1,2), (2,0) that name it; an edge of
//      multiplicity exactly 1 is a boundary edge;
//   3. fixed[i] = 1 (i or a neighbour is not finite) | 2 (deg(i) == 0) | 4 (keep_boundary and i ends a boundary edge), decided
//      once, from the input; a fixed vertex keeps its words;
//   4. a step with factor f: per component s = +0.0, s += (double)x_j over N(i) ascending, m = s / (double)deg(i),
//      x'_i = (float)(p + f * (m - p)), every vertex reading the step before (two buffers);
//   5. an iteration is a step with lambda and, iff mu != 0, a step with mu.
// Kernels:
//   k_sm_edges     one lane per face: six directed keys a << 32 | b, both directions of the three corner pairs (a == b: the
//                  all-ones sentinel, which sorts last); a face that names a vertex >= n_verts raises a flag
//   rocprim sort   of the 6 n_faces keys: a run of equal keys (a, b) is as long as the multiplicity of {a, b}
//   k_sm_heads     the head of a run is the neighbour entry; a run of one marks a as a boundary vertex
//   rocprim scan + k_sm_cols   the heads' low words, compacted: the CSR column array, ascending per row
//   k_sm_rows      one lane per vertex: the lower bound of v << 32 in the sorted keys -> the row's offset (a vertex in no
//                  face, wherever it lies, gets an empty row)
//   k_sm_pack      the positions as 16-byte records (one dwordx4 gather per neighbour); k_sm_fixed: rule 3 and deg
//   k_sm_step      rule 4, one lane per vertex, from the buffer of the step before into the other; k_sm_unpack: the result
// An inverted index in a fixed order instead of float atomics: the adds are exactly the host's, in the host's order.
// Cost of k_sm_step: a lane's time is its vertex's degree, a wave's that of its largest -- 4 to 8 on a marched mesh; a vertex
// with thousands of neighbours makes one lane walk them all, twice per iteration.  Gather-bound: no MFMA, no LDS.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "tsdf_meshgrid.h"

#define SM_C_BAD 0       // != 0: a face names a vertex >= n_verts
#define SM_C_DIRECTED 1  // entries of the column array: twice the unique undirected edges
#define SM_C_FIXED 2
static_assert(SM_C_FIXED < MP_IDX_COUNTERS, "the counters of a handle's indexed-mesh passes share one allocation");

#define SM_NO_EDGE (~0ull)
#define SM_MAX_FACES 715827882ull  // 6 n_faces directed entries are indexed with 32 bits

static thread_local MpStats g_sm_stats;  // tsdf_hip_mesh_smooth_stats

// ---- kernels ---------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint64_t sm_key(uint32_t a, uint32_t b) {
  return a == b ? SM_NO_EDGE : ((uint64_t)a << 32) | (uint64_t)b;
}

static __global__ void __launch_bounds__(256)
k_sm_edges(const uint32_t *__restrict__ faces, uint32_t n_faces, uint64_t n_verts, uint64_t *__restrict__ keys,
           unsigned long long *__restrict__ counters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= n_faces) return;
  const uint32_t a = faces[3ull * f], b = faces[3ull * f + 1ull], c = faces[3ull * f + 2ull];
  uint64_t *k = keys + 6ull * f;
  if (a >= n_verts || b >= n_verts || c >= n_verts) {
    counters[SM_C_BAD] = 1ull;  // (every writer stores the same 1; the mesh is refused, whatever its keys hold)
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = SM_NO_EDGE;
    return;
  }
  k[0] = sm_key(a, b), k[1] = sm_key(b, a), k[2] = sm_key(b, c), k[3] = sm_key(c, b), k[4] = sm_key(c, a), k[5] = sm_key(a, c);
}

// per sorted position: is it the head of a run of equal keys; a run of one is a boundary edge of its vertex a
static __global__ void __launch_bounds__(256)
k_sm_heads(const uint64_t *__restrict__ keys, uint32_t n_keys, uint8_t *__restrict__ head, uint8_t *__restrict__ boundary,
           unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool h = false;
  if (i < n_keys) {
    const uint64_t key = keys[i];
    h = key != SM_NO_EDGE && (i == 0u || keys[i - 1u] != key);
    head[i] = h ? 1 : 0;
    if (h && (i + 1u == n_keys || keys[i + 1u] != key)) boundary[key >> 32] = 1;  // (every writer stores the same 1)
  }
  mp_wave_count(h, &counters[SM_C_DIRECTED]);
}

// offset: the exclusive scan of head
static __global__ void __launch_bounds__(256)
k_sm_cols(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ head, const uint32_t *__restrict__ offset, uint32_t n_keys,
          uint32_t *__restrict__ cols) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n_keys && head[i]) cols[offset[i]] = (uint32_t)keys[i];
}

// row[v], v = 0 .. n: the heads before the first key >= v << 32.  (The sentinels lie behind every key: their offset is the
// number of all heads, and so is row[n].)
static __global__ void __launch_bounds__(256)
k_sm_rows(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ offset, uint32_t n_keys, uint32_t n,
          const unsigned long long *__restrict__ counters, uint32_t *__restrict__ row) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v > n) return;
  const uint32_t lo = mp_lower_bound(keys, n_keys, (uint64_t)v << 32);
  row[v] = lo < n_keys ? offset[lo] : (uint32_t)counters[SM_C_DIRECTED];
}

static __global__ void __launch_bounds__(256)
k_sm_pack(const uint32_t *__restrict__ verts, uint32_t n, uint4 *__restrict__ pos) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v < n) pos[v] = make_uint4(verts[3ull * v], verts[3ull * v + 1ull], verts[3ull * v + 2ull], 0u);
}

static __device__ __forceinline__ bool sm_finite(const uint4 p) {
  return (p.x & 0x7f800000u) != 0x7f800000u && (p.y & 0x7f800000u) != 0x7f800000u && (p.z & 0x7f800000u) != 0x7f800000u;
}

// rule 3, and deg
static __global__ void __launch_bounds__(256)
k_sm_fixed(const uint4 *__restrict__ pos, const uint32_t *__restrict__ row, const uint32_t *__restrict__ cols, const uint8_t *__restrict__ boundary,
           uint32_t n, int keep_boundary, uint8_t *__restrict__ fixed, uint32_t *__restrict__ degree, unsigned long long *__restrict__ counters) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  uint8_t bits = 0;
  if (v < n) {
    const uint32_t beg = row[v], end = row[v + 1u];
    bool fin = sm_finite(pos[v]);
    for (uint32_t j = beg; j < end && fin; ++j) fin = sm_finite(pos[cols[j]]);
    bits = (uint8_t)((fin ? 0 : 1) | (end == beg ? 2 : 0) | (keep_boundary && boundary[v] ? 4 : 0));
    fixed[v] = bits;
    degree[v] = end - beg;
  }
  mp_wave_count(bits != 0, &counters[SM_C_FIXED]);
}

// Rule 4.  The adds, the division, the subtraction, the product, the sum and the cast are each rounded once (the library is
// built with -ffp-contract=off), in the host's order.
static __global__ void __launch_bounds__(256)
k_sm_step(const uint4 *__restrict__ prev, uint4 *__restrict__ next, const uint32_t *__restrict__ row, const uint32_t *__restrict__ cols,
          const uint8_t *__restrict__ fixed, uint32_t n, double f) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n) return;
  const uint4 p = prev[v];
  if (fixed[v]) {
    next[v] = p;
    return;
  }
  const uint32_t beg = row[v], end = row[v + 1u];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (uint32_t j = beg; j < end; ++j) {
    const uint4 q = prev[cols[j]];
    sx += (double)__uint_as_float(q.x), sy += (double)__uint_as_float(q.y), sz += (double)__uint_as_float(q.z);
  }
  const double d = (double)(end - beg);
  const double px = (double)__uint_as_float(p.x), py = (double)__uint_as_float(p.y), pz = (double)__uint_as_float(p.z);
  const float x = (float)(px + f * (sx / d - px)), y = (float)(py + f * (sy / d - py)), z = (float)(pz + f * (sz / d - pz));
  next[v] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
}

// (a mesh that is refused keeps the caller's vertices: out may be the input)
static __global__ void __launch_bounds__(256)
k_sm_unpack(const uint4 *__restrict__ pos, uint32_t n, const unsigned long long *__restrict__ counters, uint32_t *__restrict__ out) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n || counters[SM_C_BAD]) return;
  const uint4 p = pos[v];
  out[3ull * v] = p.x, out[3ull * v + 1ull] = p.y, out[3ull * v + 2ull] = p.z;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SmLayout {  // MpWork::buf.  The unsorted keys' 8 bytes per entry hold, once the sort has run, the offsets and the columns.
  size_t pos_a, pos_b, row, degree, fixed, boundary, key_a, key_b, head, tmp, tmp_bytes, total;
};

static int sm_layout(size_t n, size_t e, hipStream_t s, SmLayout &L) {
  size_t sort_bytes = 0;
  if (const int rc = mp_tmp_bytes(0, 0, 0, e, s, &L.tmp_bytes)) return rc;
  if (e) TSDF_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, e, 0u, 64u, s));
  L.tmp_bytes = std::max(L.tmp_bytes, sort_bytes);
  MpTake take;
  L.pos_a = take(n * 16), L.pos_b = take(n * 16), L.row = take((n + 1) * 4), L.degree = take(n * 4), L.fixed = take(n), L.boundary = take(n);
  L.key_a = take(e * 8), L.key_b = take(e * 8), L.head = take(e), L.tmp = take(L.tmp_bytes);
  L.total = take.o;
  return TSDF_HIP_OK;
}

// The whole pass on device arrays: d_in (n_verts x 3 floats) -> d_out (may be d_in; written only when no face is refused).
// Leaves in MpWork::buf the fixed bits and the degrees, and the stats of the calling thread.  Every launch is queued without
// a host read in between; the one read, of the counters, follows the last kernel.  Leaves the stream idle.
static int sm_core(MpWork &w, hipStream_t s, const float *d_in, uint64_t n_verts, const uint32_t *d_faces, uint64_t n_faces, float lambda, float mu,
                   int iterations, int keep_boundary, float *d_out, SmLayout &L, uint64_t *n_fixed, const char *who) {
  const uint32_t n = (uint32_t)n_verts, nf = (uint32_t)n_faces, e = 6u * nf;
  int rc = sm_layout(n, e, s, L);
  if (rc || (rc = w.buf.reserve(L.total, s, "mesh smooth")) || (rc = mp_work_begin(w, MP_IDX_COUNTERS, 2, s))) return rc;
  char *b = (char *)w.buf.p;
  uint4 *pos[2] = {(uint4 *)(b + L.pos_a), (uint4 *)(b + L.pos_b)};
  uint32_t *row = (uint32_t *)(b + L.row), *degree = (uint32_t *)(b + L.degree);
  uint8_t *fixed = (uint8_t *)(b + L.fixed), *boundary = (uint8_t *)(b + L.boundary), *head = (uint8_t *)(b + L.head);
  uint64_t *key_a = (uint64_t *)(b + L.key_a), *keys = (uint64_t *)(b + L.key_b);
  uint32_t *offset = (uint32_t *)key_a, *cols = offset + e;
  const dim3 blk(256), grid_n((n + 255u) / 256u), grid_e((e + 255u) / 256u);

  TSDF_HIP_TRY(hipEventRecord(w.ev[0], s));
  TSDF_HIP_TRY(hipMemsetAsync(boundary, 0, (size_t)n, s));
  if (nf) {
    hipLaunchKernelGGL(k_sm_edges, dim3((nf + 255u) / 256u), blk, 0, s, d_faces, nf, n_verts, key_a, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    size_t tmp_bytes = L.tmp_bytes;
    TSDF_HIP_TRY(rocprim::radix_sort_keys(b + L.tmp, tmp_bytes, key_a, keys, (size_t)e, 0u, 64u, s));
    hipLaunchKernelGGL(k_sm_heads, grid_e, blk, 0, s, keys, e, head, boundary, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    tmp_bytes = L.tmp_bytes;
    TSDF_HIP_TRY(rocprim::exclusive_scan(b + L.tmp, tmp_bytes, MpKeepIt(head, MpKeepCount()), offset, 0u, (size_t)e, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_sm_cols, grid_e, blk, 0, s, keys, head, offset, e, cols);
    TSDF_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sm_rows, dim3(n / 256u + 1u), blk, 0, s, keys, offset, e, n, w.count(), row);
  TSDF_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sm_pack, grid_n, blk, 0, s, (const uint32_t *)d_in, n, pos[0]);
  TSDF_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sm_fixed, grid_n, blk, 0, s, pos[0], row, cols, boundary, n, keep_boundary, fixed, degree, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  int at = 0;  // the buffer that holds the last step's result
  for (int it = 0; it < iterations; ++it)
    for (int half = 0; half < (mu != 0.f ? 2 : 1); ++half) {
      hipLaunchKernelGGL(k_sm_step, grid_n, blk, 0, s, pos[at], pos[at ^ 1], row, cols, fixed, n, (double)(half ? mu : lambda));
      TSDF_HIP_TRY(hipGetLastError());
      at ^= 1;
    }
  hipLaunchKernelGGL(k_sm_unpack, grid_n, blk, 0, s, pos[at], n, w.count(), (uint32_t *)d_out);
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(w.ev[1], s));
  unsigned long long counts[MP_IDX_COUNTERS] = {0};
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  if (counts[SM_C_BAD]) {
    tsdf_set_error(std::string(who) + ": a face names a vertex index >= n_verts");
    return TSDF_HIP_E_INVALID;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
  g_sm_stats.set(n, counts[SM_C_DIRECTED] / 2ull, counts[SM_C_FIXED], (uint64_t)(ms * 1000.f));
  *n_fixed = counts[SM_C_FIXED];
  return TSDF_HIP_OK;
}

static int sm_refuse(const char *who, const char *why) {
  tsdf_set_error(std::string(who) + ": " + why);
  return TSDF_HIP_E_INVALID;
}

static int sm_check_args(float lambda, float mu, int iterations, uint64_t n_verts, uint64_t n_faces, const char *who) {
  if (!std::isfinite(lambda) || !(lambda > 0.f && lambda <= 1.f)) return sm_refuse(who, "lambda must be finite and in (0, 1]");
  if (!std::isfinite(mu) || !(mu >= -1.f && mu <= 0.f)) return sm_refuse(who, "mu must be finite and in [-1, 0]");
  if (iterations < 0 || iterations > 1000) return sm_refuse(who, "iterations must be in [0, 1000]");
  if (const int rc = mp_check_counts(who, n_faces, &n_verts)) return rc;
  if (n_faces > SM_MAX_FACES) return sm_refuse(who, "the 6 directed edge entries per face are indexed with 32 bits: more than 715827882 faces are not accepted");
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_smooth(int device, const float *verts, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces, float lambda, float mu,
                                    int iterations, int keep_boundary, float *out_verts, uint8_t *fixed, uint32_t *degree) {
  const char *who = "tsdf_hip_mesh_smooth";
  if (const int rc = sm_check_args(lambda, mu, iterations, n_verts, n_faces, who)) return rc;
  if (device < 0) return TSDF_HIP_E_INVALID;
  if (n_verts && (!verts || !out_verts)) return sm_refuse(who, "verts and out_verts must not be NULL");
  if (!faces && (n_faces || n_verts)) return sm_refuse(who, "a triangle soup shares no vertices, so it has no neighbours to smooth with: flatten or decimate first");
  if (n_verts == 0) {
    if (n_faces) return sm_refuse(who, "a face names a vertex index >= n_verts");
    g_sm_stats.zero();
    return TSDF_HIP_OK;
  }
  MpCall c;
  const size_t b_verts = mp_up((size_t)n_verts * 12), b_faces = (size_t)n_faces * 12;
  int rc = c.open(device, b_verts + b_faces, who);
  if (rc) return rc;
  float *d_verts = (float *)c.in.p;
  uint32_t *d_faces = n_faces ? (uint32_t *)((char *)c.in.p + b_verts) : nullptr;
  if ((rc = c.upload(d_verts, verts, (size_t)n_verts * 12)) || (d_faces && (rc = c.upload(d_faces, faces, b_faces)))) return rc;
  SmLayout L;
  uint64_t n_fixed = 0;
  if ((rc = sm_core(c.work, c.s, d_verts, n_verts, d_faces, n_faces, lambda, mu, iterations, keep_boundary, d_verts, L, &n_fixed, who))) return rc;
  const char *b = (const char *)c.work.buf.p;
  if ((rc = c.download(out_verts, d_verts, (size_t)n_verts * 12))) return rc;
  if (fixed && (rc = c.download(fixed, b + L.fixed, (size_t)n_verts))) return rc;
  if (degree && (rc = c.download(degree, b + L.degree, (size_t)n_verts * 4))) return rc;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_march_smooth(tsdf_handle h, float lambda, float mu, int iterations, int keep_boundary, uint64_t *n_fixed) {
  const char *who = "tsdf_hip_march_smooth";
  if (!h) return TSDF_HIP_E_INVALID;
  if (n_fixed) *n_fixed = 0;
  if (const int rc = sm_check_args(lambda, mu, iterations, 0, 0, who)) return rc;
  tsdf_flatten_state *st = h->fl;
  if (!st || !st->valid)
    return sm_refuse(who, "no indexed mesh: neither tsdf_hip_march_flatten nor tsdf_hip_march_decimate has run since the last tsdf_hip_march / "
                          "tsdf_hip_march_cleanup (a soup shares no vertices: flatten or decimate first)");
  const uint64_t m = st->n_verts, k = st->n_faces;
  if (const int rc = sm_check_args(lambda, mu, iterations, m, k, who)) return rc;
  uint64_t fixed = 0;
  if (!m) {
    g_sm_stats.zero();
  } else if (h->multi) {
    // A set keeps its indexed mesh on the host: the host-array route on the first slab's device, as decimate takes it.
    if (const int rc = tsdf_hip_mesh_smooth(tsdf_multi_first(h)->device, st->h_verts.data(), m, st->h_faces.data(), k, lambda, mu, iterations,
                                            keep_boundary, st->h_verts.data(), nullptr, nullptr))
      return rc;
    fixed = g_sm_stats.v[2];
  } else {
    TSDF_ENTER(h);
    SmLayout L;
    char *o = (char *)st->out.p;
    if (const int rc = sm_core(st->work, h->stream, (const float *)o, m, (const uint32_t *)(o + st->o_faces), k, lambda, mu, iterations, keep_boundary,
                               (float *)o, L, &fixed, who))
      return rc;
  }
  st->nm_valid = false;  // (normals of the vertices before they moved: tsdf_normals.hip)
  if (n_fixed) *n_fixed = fixed;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_smooth_stats(uint64_t out[4]) {
  return g_sm_stats.copy_out(out);
}
