// libtsdf_hip.so -- area-weighted vertex normals of a triangle mesh (meshNormals).
//
// An extension with no counterpart in the reference.  cpu_tsdf::mesh_post::normalArrays (csrc/prog/mesh_post.h) defines the
// result as one sequential pass, and this file reproduces it word for word:
//   1. the face vector of f = (a, b, c): e1 = (double)p_b - (double)p_a, e2 = (double)p_c - (double)p_a, g_f = e1 x e2, every
//      difference, product and subtraction rounded once (no FMA: the library is built with -ffp-contract=off); |g_f| is twice
//      the area.  A face with a coordinate that is not finite at any corner is SKIPPED: it adds nothing and is counted;
//   2. per component s_i = +0.0, then s_i += g_f over the faces that name i in ascending face index, once per corner that
//      names i;
//   3. l2 = (sx * sx + sy * sy) + sz * sz, l = sqrt(l2); l2 == 0: three +0.0f, else ((float)(sx / l), (float)(sy / l),
//      (float)(sz / l)) -- divisions, not a product with a reciprocal;
//   4. flags[i] = 1 (no face names i) | 2 (rule 3 wrote zero) | 4 (a face that names i was skipped);
//   5. the normal points to the side from which a -> b -> c appear counter-clockwise; on a marched mesh: out of the surface,
//      into observed free space.
// Kernels:
//   k_nm_face      one lane per face: g_f as one 32-byte record (three doubles and a word that says "skipped") and three keys
//                  vertex << 32 | face; a face that names a vertex >= n_verts raises a flag (its keys then name vertex 0, so
//                  that whatever follows stays in bounds; the mesh is refused and nothing is written)
//   rocprim sort   of the 3 n_faces keys: the run of a vertex is its faces in ascending order, corner repeats adjacent
//   k_nm_rows      one lane per vertex: the lower bound of v << 32 in the sorted keys (mp_lower_bound, as k_sm_rows)
//   k_nm_vertex    one lane per vertex: walks its run with one 32-byte record gathered per entry, adds in fp64 in that
//                  order, normalises, writes the 12-byte normal and the flag byte
//   k_nm_soup      a soup (face f = vertices 3f, 3f + 1, 3f + 2) needs no sort: one lane per face computes g_f, normalises
//                  +0.0 + g_f and writes it to the face's three vertices
// An inverted index in a fixed order instead of float atomics: the adds are exactly the host's, in the host's order.
// Cost of k_nm_vertex: a lane's time is its vertex's valence (the entries of its run), a wave's that of its largest -- 4 to 8
// on a marched mesh; a vertex named by thousands of faces makes one lane walk them all.  Gather-bound: no MFMA, no LDS.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "tsdf_meshgrid.h"

#define NM_C_BAD 0      // != 0: a face names a vertex >= n_verts
#define NM_C_SKIPPED 1  // faces with a coordinate that is not finite
#define NM_C_ZERO 2     // vertices whose normal is zero (k_nm_soup: faces; each has three vertices)
static_assert(NM_C_ZERO < MP_IDX_COUNTERS, "the counters of a handle's indexed-mesh passes share one allocation");

#define NM_MAX_FACES 1431655765ull  // 3 n_faces entries are indexed with 32 bits

static thread_local MpStats g_nm_stats;  // tsdf_hip_mesh_normals_stats

void tsdf_normals_invalidate(tsdf_hip_volume *v) {
  if (v->fl) v->fl->nm_valid = false;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// Rule 1 for the corners at vertex indices a, b, c.  true: skipped (g is then zero).
static __device__ __forceinline__ bool nm_face_vector(const float *__restrict__ verts, uint64_t a, uint64_t b, uint64_t c, double g[3]) {
  const float ax = verts[3ull * a], ay = verts[3ull * a + 1ull], az = verts[3ull * a + 2ull];
  const float bx = verts[3ull * b], by = verts[3ull * b + 1ull], bz = verts[3ull * b + 2ull];
  const float cx = verts[3ull * c], cy = verts[3ull * c + 1ull], cz = verts[3ull * c + 2ull];
  g[0] = g[1] = g[2] = 0.0;
  if (!(isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(cx) && isfinite(cy) && isfinite(cz)))
    return true;
  const double e1x = (double)bx - (double)ax, e1y = (double)by - (double)ay, e1z = (double)bz - (double)az;
  const double e2x = (double)cx - (double)ax, e2y = (double)cy - (double)ay, e2z = (double)cz - (double)az;
  g[0] = e1y * e2z - e1z * e2y;
  g[1] = e1z * e2x - e1x * e2z;
  g[2] = e1x * e2y - e1y * e2x;
  return false;
}

// Rule 3.  true: zero.
static __device__ __forceinline__ bool nm_normalise(double sx, double sy, double sz, float n[3]) {
  const double l2 = (sx * sx + sy * sy) + sz * sz;
  if (l2 == 0.0) {
    n[0] = n[1] = n[2] = 0.f;
    return true;
  }
  const double l = sqrt(l2);
  n[0] = (float)(sx / l), n[1] = (float)(sy / l), n[2] = (float)(sz / l);
  return false;
}

static __global__ void __launch_bounds__(256)
k_nm_face(const float *__restrict__ verts, const uint32_t *__restrict__ faces, uint32_t n_faces, uint64_t n_verts, double4 *__restrict__ rec,
          uint64_t *__restrict__ keys, unsigned long long *__restrict__ counters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  bool skipped = false;
  if (f < n_faces) {
    uint32_t a = faces[3ull * f], b = faces[3ull * f + 1ull], c = faces[3ull * f + 2ull];
    if (a >= n_verts || b >= n_verts || c >= n_verts) {
      counters[NM_C_BAD] = 1ull;  // (every writer stores the same 1; the mesh is refused, whatever its records hold)
      a = b = c = 0u;
    }
    double g[3];
    skipped = nm_face_vector(verts, a, b, c, g);
    rec[f] = make_double4(g[0], g[1], g[2], skipped ? 1.0 : 0.0);
    uint64_t *k = keys + 3ull * f;
    k[0] = ((uint64_t)a << 32) | f, k[1] = ((uint64_t)b << 32) | f, k[2] = ((uint64_t)c << 32) | f;
  }
  mp_wave_count(skipped, &counters[NM_C_SKIPPED]);
}

// row[v], v = 0 .. n: the entries before the first key >= v << 32 (row[n] = n_keys: every key names a vertex < n)
static __global__ void __launch_bounds__(256)
k_nm_rows(const uint64_t *__restrict__ keys, uint32_t n_keys, uint32_t n, uint32_t *__restrict__ row) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v <= n) row[v] = mp_lower_bound(keys, n_keys, (uint64_t)v << 32);
}

// Rules 2 to 4.  (A skipped face's record is zero, but it is not added: rule 2 speaks of the faces that count.)
static __global__ void __launch_bounds__(256)
k_nm_vertex(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ row, const double4 *__restrict__ rec, uint32_t n,
            float *__restrict__ normals, uint8_t *__restrict__ flags, unsigned long long *__restrict__ counters) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  bool zero = false;
  if (v < n && !counters[NM_C_BAD]) {
    const uint32_t beg = row[v], end = row[v + 1u];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    uint8_t bits = beg == end ? 1 : 0;
    for (uint32_t j = beg; j < end; ++j) {
      const double4 g = rec[(uint32_t)keys[j]];
      if (g.w != 0.0)
        bits |= 4;
      else
        sx += g.x, sy += g.y, sz += g.z;
    }
    float nv[3];
    zero = nm_normalise(sx, sy, sz, nv);
    normals[3ull * v] = nv[0], normals[3ull * v + 1ull] = nv[1], normals[3ull * v + 2ull] = nv[2];
    flags[v] = (uint8_t)(bits | (zero ? 2 : 0));
  }
  mp_wave_count(zero, &counters[NM_C_ZERO]);
}

// The soup: vertex 3f + k is named by face f alone, once, so s = +0.0 + g_f (which turns a -0.0 into +0.0, as rule 2 does).
static __global__ void __launch_bounds__(256)
k_nm_soup(const float *__restrict__ verts, uint32_t n_faces, float *__restrict__ normals, uint8_t *__restrict__ flags,
          unsigned long long *__restrict__ counters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  bool skipped = false, zero = false;
  if (f < n_faces) {
    double g[3];
    skipped = nm_face_vector(verts, 3ull * f, 3ull * f + 1ull, 3ull * f + 2ull, g);
    float nv[3];
    zero = nm_normalise(0.0 + g[0], 0.0 + g[1], 0.0 + g[2], nv);
    const uint8_t bits = (uint8_t)((zero ? 2 : 0) | (skipped ? 4 : 0));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float *o = normals + 9ull * f + 3ull * k;
      o[0] = nv[0], o[1] = nv[1], o[2] = nv[2];
      flags[3ull * f + k] = bits;
    }
  }
  mp_wave_count(skipped, &counters[NM_C_SKIPPED]);
  mp_wave_count(zero, &counters[NM_C_ZERO]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct NmLayout {  // MpWork::buf of an indexed mesh (a soup needs none)
  size_t rec, key_a, key_b, row, tmp, tmp_bytes, total;
};

static unsigned nm_bits(uint64_t v) {  // the bits that hold every value < v
  unsigned b = 0;
  while (b < 32u && (1ull << b) < v) ++b;
  return b;
}

static int nm_layout(size_t n, size_t e, unsigned end_bit, hipStream_t s, NmLayout &L) {
  L.tmp_bytes = 0;
  if (e) TSDF_HIP_TRY(rocprim::radix_sort_keys(nullptr, L.tmp_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, e, 0u, end_bit, s));
  MpTake take;
  L.rec = take(e / 3 * 32), L.key_a = take(e * 8), L.key_b = take(e * 8), L.row = take((n + 1) * 4), L.tmp = take(L.tmp_bytes);
  L.total = take.o;
  return TSDF_HIP_OK;
}

// The whole pass on device arrays: d_verts (n_verts x 3 floats), d_faces (n_faces x 3; soup: not read, n_faces is 0 or
// n_verts / 3) -> d_normals (n_verts x 3 floats), d_flags (n_verts bytes), both written only when no face is refused.  Leaves
// the stats of the calling thread.  Every launch is queued without a host read in between; the one read, of the counters,
// follows the last kernel.  Leaves the stream idle.
static int nm_core(MpWork &w, hipStream_t s, const float *d_verts, uint64_t n_verts, const uint32_t *d_faces, bool soup, uint64_t n_faces,
                   float *d_normals, uint8_t *d_flags, uint64_t *n_zero, const char *who) {
  const uint32_t n = (uint32_t)n_verts, nf = (uint32_t)n_faces, e = 3u * nf;
  const dim3 blk(256), grid_n((n + 255u) / 256u), grid_f((nf + 255u) / 256u);
  int rc = TSDF_HIP_OK;
  NmLayout L;
  if (!soup) {
    const unsigned end_bit = 32u + nm_bits(n_verts);
    if ((rc = nm_layout(n, e, end_bit, s, L)) || (rc = w.buf.reserve(L.total, s, "mesh normals"))) return rc;
  }
  if ((rc = mp_work_begin(w, MP_IDX_COUNTERS, 2, s))) return rc;
  TSDF_HIP_TRY(hipEventRecord(w.ev[0], s));
  if (soup) {
    if (nf) {
      hipLaunchKernelGGL(k_nm_soup, grid_f, blk, 0, s, d_verts, nf, d_normals, d_flags, w.count());
      TSDF_HIP_TRY(hipGetLastError());
    } else {  // vertices and no face: rule 4's bits 1 | 2 everywhere
      TSDF_HIP_TRY(hipMemsetAsync(d_normals, 0, (size_t)n * 12, s));
      TSDF_HIP_TRY(hipMemsetAsync(d_flags, 3, (size_t)n, s));
    }
  } else {
    char *b = (char *)w.buf.p;
    double4 *rec = (double4 *)(b + L.rec);
    uint64_t *key_a = (uint64_t *)(b + L.key_a), *keys = (uint64_t *)(b + L.key_b);
    uint32_t *row = (uint32_t *)(b + L.row);
    if (nf) {
      hipLaunchKernelGGL(k_nm_face, grid_f, blk, 0, s, d_verts, d_faces, nf, n_verts, rec, key_a, w.count());
      TSDF_HIP_TRY(hipGetLastError());
      size_t tmp_bytes = L.tmp_bytes;
      TSDF_HIP_TRY(rocprim::radix_sort_keys(b + L.tmp, tmp_bytes, key_a, keys, (size_t)e, 0u, 32u + nm_bits(n_verts), s));
    }
    hipLaunchKernelGGL(k_nm_rows, dim3(n / 256u + 1u), blk, 0, s, keys, e, n, row);
    TSDF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_nm_vertex, grid_n, blk, 0, s, keys, row, rec, n, d_normals, d_flags, w.count());
    TSDF_HIP_TRY(hipGetLastError());
  }
  TSDF_HIP_TRY(hipEventRecord(w.ev[1], s));
  unsigned long long counts[MP_IDX_COUNTERS] = {0};
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  if (counts[NM_C_BAD]) {
    tsdf_set_error(std::string(who) + ": a face names a vertex index >= n_verts");
    return TSDF_HIP_E_INVALID;
  }
  const uint64_t zero = soup ? (nf ? 3ull * counts[NM_C_ZERO] : n_verts) : counts[NM_C_ZERO];
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
  g_nm_stats.set(n_verts, counts[NM_C_SKIPPED], zero, (uint64_t)(ms * 1000.f));
  *n_zero = zero;
  return TSDF_HIP_OK;
}

static int nm_refuse(const char *who, const char *why) {
  tsdf_set_error(std::string(who) + ": " + why);
  return TSDF_HIP_E_INVALID;
}

static int nm_check_counts(const char *who, uint64_t n_verts, bool soup, uint64_t n_faces) {
  if (const int rc = mp_check_counts(who, n_faces, &n_verts)) return rc;
  if (n_faces > NM_MAX_FACES) return nm_refuse(who, "the 3 entries per face are indexed with 32 bits: more than 1431655765 faces are not accepted");
  if (soup && (n_verts % 3ull || (n_faces && n_faces != n_verts / 3ull)))
    return nm_refuse(who, "a triangle soup has 3 vertices per face: n_verts must be a multiple of 3 and n_faces 0 or n_verts / 3");
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_normals(int device, const float *verts, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces, float *out_normals,
                                     uint8_t *flags) {
  const char *who = "tsdf_hip_mesh_normals";
  const bool soup = faces == nullptr;
  if (const int rc = nm_check_counts(who, n_verts, soup, n_faces)) return rc;
  if (device < 0) return TSDF_HIP_E_INVALID;
  if (n_verts && (!verts || !out_normals)) return nm_refuse(who, "verts and out_normals must not be NULL");
  if (n_verts == 0) {
    if (n_faces) return nm_refuse(who, "a face names a vertex index >= n_verts");
    g_nm_stats.zero();
    return TSDF_HIP_OK;
  }
  MpCall c;
  MpTake take;
  const size_t o_verts = take((size_t)n_verts * 12), o_faces = take(soup ? 0 : (size_t)n_faces * 12), o_normals = take((size_t)n_verts * 12),
               o_flags = take((size_t)n_verts);
  int rc = c.open(device, take.o, who);
  if (rc) return rc;
  char *in = (char *)c.in.p;
  if ((rc = c.upload(in + o_verts, verts, (size_t)n_verts * 12)) || (!soup && (rc = c.upload(in + o_faces, faces, (size_t)n_faces * 12)))) return rc;
  uint64_t zero = 0;
  if ((rc = nm_core(c.work, c.s, (const float *)(in + o_verts), n_verts, (const uint32_t *)(in + o_faces), soup, n_faces, (float *)(in + o_normals),
                    (uint8_t *)(in + o_flags), &zero, who)))
    return rc;
  if ((rc = c.download(out_normals, in + o_normals, (size_t)n_verts * 12))) return rc;
  if (flags && (rc = c.download(flags, in + o_flags, (size_t)n_verts))) return rc;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_march_normals(tsdf_handle h, uint64_t *n_verts, uint64_t *n_zero) {
  const char *who = "tsdf_hip_march_normals";
  if (!h) return TSDF_HIP_E_INVALID;
  if (n_verts) *n_verts = 0;
  if (n_zero) *n_zero = 0;
  if (!h->mc_valid) return nm_refuse(who, "the last tsdf_hip_march on this handle did not succeed, or none has run");
  if (!h->fl) h->fl = new tsdf_flatten_state();
  tsdf_flatten_state *st = h->fl;
  st->nm_valid = false;
  const bool soup = !st->valid;  // no indexed mesh: the soup of the last march / cleanup
  const uint64_t n = soup ? 3ull * h->mc_ntri : st->n_verts, k = soup ? h->mc_ntri : st->n_faces;
  if (const int rc = nm_check_counts(who, n, soup, k)) return rc;
  uint64_t zero = 0;
  if (!n) {
    g_nm_stats.zero();
  } else if (h->multi) {
    // A set keeps its meshes on the host: the host-array route on the first slab's device, as smooth takes it.
    static const uint32_t none[3] = {0, 0, 0};  // (an empty vector's data() may be NULL: an indexed mesh without faces is no soup)
    const float *verts = st->h_verts.data();
    const uint8_t *rgb = nullptr;
    const uint64_t *cell = nullptr;
    if (soup) tsdf_multi_mesh(h, &verts, &rgb, &cell);
    st->h_normals.resize((size_t)n * 3);
    if (const int rc = tsdf_hip_mesh_normals(tsdf_multi_first(h)->device, verts, n, soup ? nullptr : (k ? st->h_faces.data() : none), k,
                                             st->h_normals.data(), nullptr))
      return rc;
    zero = g_nm_stats.v[2];
  } else {
    TSDF_ENTER(h);
    const size_t o_flags = mp_up((size_t)n * 12);
    if (const int rc = st->nm_out.reserve(o_flags + (size_t)n, h->stream, "mesh normals")) return rc;
    const char *o = (const char *)st->out.p;
    if (const int rc = nm_core(st->work, h->stream, soup ? h->mc_verts.as<float>() : (const float *)o, n, soup ? nullptr : (const uint32_t *)(o + st->o_faces), soup,
                               k, (float *)st->nm_out.p, (uint8_t *)st->nm_out.p + o_flags, &zero, who))
      return rc;
  }
  st->nm_valid = true;
  st->nm_n = n;
  if (n_verts) *n_verts = n;
  if (n_zero) *n_zero = zero;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_march_fetch_normals(tsdf_handle h, float *normals) {
  const char *who = "tsdf_hip_march_fetch_normals";
  if (!h) return TSDF_HIP_E_INVALID;
  const tsdf_flatten_state *st = h->fl;
  if (!st || !st->nm_valid)
    return nm_refuse(who, "no normals: tsdf_hip_march_normals has not run since the last tsdf_hip_march / _march_cleanup / _march_flatten / "
                          "_march_decimate / _march_smooth or tsdf_hip_reset");
  const size_t n = (size_t)st->nm_n;
  if (!n) return TSDF_HIP_OK;
  if (!normals) return nm_refuse(who, "normals must not be NULL");
  if (h->multi) {
    memcpy(normals, st->h_normals.data(), n * 12);
    return TSDF_HIP_OK;
  }
  TSDF_ENTER(h);
  if (const int rc = tsdf_to_host(h, normals, st->nm_out.p, n * 12)) return rc;
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_normals_stats(uint64_t out[4]) {
  return g_nm_stats.copy_out(out);
}
