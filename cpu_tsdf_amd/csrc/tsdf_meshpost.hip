// libtsdf_hip.so -- floater removal of a triangle mesh.
//
// Replaces cleanupMesh of the reference's `integrate` program (src/prog/integrate.cpp:152-214), as this repository's host
// restatement cpu_tsdf::mesh_post::cleanupMesh (csrc/prog/mesh_post.h) defines it operation for operation: faces whose
// centroids form a connected group (links: centroid distance strictly below face_dist, candidates from the 27 grid cells of
// edge face_dist around a face's own) of at most min_neighbors faces are removed.  The result is a SET, so it parallelises
// exactly:
//   k_mp_centroid  centroid ((v0 + v1) + v2) / 3.f and the host's cell key per face; non-finite centroids get the key ~0
//   rocprim sort   (key, face) pairs; k_mp_gather writes the centroids in sorted order and marks run heads, a scan numbers
//                  the cells, mp_cells_build makes the cell table and each cell's 27 neighbour cells (tsdf_meshgrid.hip;
//                  mp_cell_key, mp_for_links and k_mp_compact are in tsdf_meshgrid.h: tsdf_flatten.hip builds the same
//                  grid of vertices)
//   k_mp_degree    links per face, leaving at min_neighbors: a face with that many links is HEAVY -- its group has more than
//                  min_neighbors faces whatever else it holds.  On a surface nearly every face is heavy after a few tests.
//   k_mp_link      the LIGHT faces enumerate all their links and join a lock-free union-find (CAS hooking of the larger root
//                  under the smaller, path halving); a link to a heavy face joins that face's tree as well
//   k_mp_count     per tree: "holds a heavy face" or the number of (light) members
//   k_mp_keep      keep = heavy, or in a tree with a heavy face, or in a tree of more than min_neighbors faces
// A tree without a heavy face is a whole group (every member enumerated every link), so its size is the group's size; a tree
// with one lies inside a group that is large enough.  No kernel waits for another workgroup: the only
// loops over shared state are CAS retries, each of which fails only because another thread's CAS succeeded.
// Gather-bound pointer chasing and a radix sort: no MFMA.
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "tsdf_meshgrid.h"

// ---- state -----------------------------------------------------------------------------------------------------------------
#define MP_TEST_SLOTS 64  // counters[MP_C_TESTS ..]: link tests, striped (one address for every wave costs milliseconds)
#define MP_C_FINITE 0     // faces with a finite centroid
#define MP_C_BAD 1        // != 0: a face names a vertex >= n_verts
#define MP_C_KEPT 2
#define MP_C_TESTS 8
#define MP_COUNTERS (MP_C_TESTS + MP_TEST_SLOTS)

struct tsdf_meshpost_state {  // per handle (tsdf_hip_volume::mp); a set has none: its mesh goes through tsdf_hip_mesh_cleanup
  MpWork work;
};

static thread_local MpStats g_mp_stats;  // tsdf_hip_mesh_cleanup_stats

void tsdf_meshpost_release(tsdf_hip_volume *v) {
  if (!v->mp) return;
  TsdfDeviceScope scope(v->device);
  delete v->mp;
  v->mp = nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

// mesh_post.h:124 -- ((v0 + v1) + v2) / 3.f per component (the build keeps -ffp-contract=off and hipcc's correctly rounded
// float division).  false: the face names a vertex that does not exist.
static __device__ __forceinline__ bool mp_centroid(const float *__restrict__ verts, uint64_t n_verts, const uint32_t *__restrict__ faces,
                                                   uint32_t f, float c[3]) {
  uint64_t v0 = 3ull * f, v1 = v0 + 1ull, v2 = v0 + 2ull;
  if (faces) v0 = faces[3ull * f], v1 = faces[3ull * f + 1ull], v2 = faces[3ull * f + 2ull];
  if (v0 >= n_verts || v1 >= n_verts || v2 >= n_verts) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = ((verts[3ull * v0 + k] + verts[3ull * v1 + k]) + verts[3ull * v2 + k]) / 3.f;
  return true;
}

static __global__ void __launch_bounds__(256)
k_mp_centroid(const float *__restrict__ verts, uint64_t n_verts, const uint32_t *__restrict__ faces, uint32_t n, double cell,
              uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, unsigned long long *__restrict__ counters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  bool fin = false;
  if (f < n) {
    float c[3] = {0.f, 0.f, 0.f};
    uint64_t key = MP_NO_KEY;
    bool wraps = false;  // (cells that alias under the key's masks share a bucket, as on the host)
    if (!mp_centroid(verts, n_verts, faces, f, c))
      counters[MP_C_BAD] = 1ull;  // (every writer stores the same 1)
    else
      key = mp_cell_key(c[0], c[1], c[2], cell, wraps);
    fin = key != MP_NO_KEY;
    keys[f] = key;
    idx[f] = f;
  }
  mp_wave_count(fin, &counters[MP_C_FINITE]);
}

// sorted position i -> centroid of the face there (computed again from the vertices: the same operations give the same
// bits, and the unsorted centroids need not be kept), and "first face of its cell"
static __global__ void __launch_bounds__(256)
k_mp_gather(const float *__restrict__ verts, uint64_t n_verts, const uint32_t *__restrict__ faces, const uint32_t *__restrict__ order,
            const uint64_t *__restrict__ keys, uint32_t n, float4 *__restrict__ cen, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  float c[3] = {0.f, 0.f, 0.f};
  if (key != MP_NO_KEY) (void)mp_centroid(verts, n_verts, faces, order[i], c);
  cen[i] = make_float4(c[0], c[1], c[2], 0.f);
  head[i] = mp_cell_head(keys, i, key);
}

static __device__ __forceinline__ void mp_add_tests(unsigned tests, unsigned long long *counters) {
  unsigned long long t = tests;
  for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&counters[MP_C_TESTS + blockIdx.x % MP_TEST_SLOTS], t);
}

static __global__ void __launch_bounds__(256)
k_mp_degree(const MpGrid g, uint32_t min_nb, uint8_t *__restrict__ heavy, uint32_t *__restrict__ parent,
            unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  unsigned tests = 0u;
  if (i < g.n_fin) {
    uint32_t deg = 0u;
    if (min_nb) mp_for_links(g, i, tests, [&](uint32_t) { return ++deg < min_nb; });
    heavy[i] = deg >= min_nb ? 1 : 0;
    parent[i] = i;
  }
  mp_add_tests(tests, counters);
}

// Union-find on `parent` (every entry <= its index, roots point at themselves).  All accesses are agent-scope atomics: the
// XCDs' L2s are not coherent for plain accesses inside one kernel.  A stale read could only name an older ancestor.
static __device__ __forceinline__ uint32_t mp_find(uint32_t *parent, uint32_t x) {
  uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    const uint32_t gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving: x is no root and never becomes one
    x = p;
    p = gp;
  }
  return x;
}

static __device__ __forceinline__ void mp_union(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = mp_find(parent, a);
    b = mp_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b, b = t;
    }
    // hook the larger root under the smaller (no cycle can form); fails only if another thread hooked a first
    uint32_t expect = a;
    if (__hip_atomic_compare_exchange_strong(&parent[a], &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

static __global__ void __launch_bounds__(256)
k_mp_link(const MpGrid g, const uint8_t *__restrict__ heavy, uint32_t *__restrict__ parent, unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  unsigned tests = 0u;
  if (i < g.n_fin && !heavy[i])
    mp_for_links(g, i, tests, [&](uint32_t j) {
      if (heavy[j] || j < i) mp_union(parent, i, j);  // (a light j > i makes this union itself)
      return true;
    });
  mp_add_tests(tests, counters);
}

static __global__ void __launch_bounds__(256)
k_mp_count(uint32_t n_fin, const uint8_t *__restrict__ heavy, uint32_t *__restrict__ parent, uint8_t *__restrict__ any_heavy,
           uint32_t *__restrict__ members) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_fin) return;
  const uint32_t r = mp_find(parent, i);
  if (heavy[i])
    any_heavy[r] = 1;
  else
    atomicAdd(&members[r], 1u);
}

// positions >= n_fin hold the faces without a finite centroid: groups of one (mesh_post.h:132-145 seeds a group with every
// face, and forNeighbours gives such a face no link, not even to itself)
static __global__ void __launch_bounds__(256)
k_mp_keep(uint32_t n, uint32_t n_fin, uint32_t min_nb, const uint32_t *__restrict__ order, const uint8_t *__restrict__ heavy,
          uint32_t *__restrict__ parent, const uint8_t *__restrict__ any_heavy, const uint32_t *__restrict__ members,
          uint8_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool k = false;
  if (i < n) {
    if (i >= n_fin) {
      k = 1u > min_nb;
    } else if (heavy[i]) {
      k = true;
    } else {
      const uint32_t r = mp_find(parent, i);
      k = any_heavy[r] || members[r] > min_nb;
    }
    keep[order[i]] = k ? 1 : 0;
  }
  mp_wave_count(k, &counters[MP_C_KEPT]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct MpLayout {  // the per-face arrays inside MpWork::buf
  size_t key_a, key_b, idx_a, idx_b, cen, cellno, heavy, any_heavy, keep, tmp, tmp_bytes, total;
};

static int mp_layout(size_t n, hipStream_t s, MpLayout &L) {
  if (const int rc = mp_tmp_bytes(n, 0, n, n, s, &L.tmp_bytes)) return rc;
  MpTake take;
  L.key_a = take(n * 8), L.key_b = take(n * 8), L.idx_a = take(n * 4), L.idx_b = take(n * 4), L.cen = take(n * 16);
  L.cellno = take(n * 4), L.heavy = take(n), L.any_heavy = take(n), L.keep = take(n);
  L.tmp = take(L.tmp_bytes);
  L.total = take.o;
  return TSDF_HIP_OK;
}

// The whole pass on device arrays: keep[f] (in MpWork::buf at L.keep) for the n faces, *n_kept, and the stats of the calling
// thread.  Leaves the stream idle.
static int mp_core(MpWork &w, hipStream_t s, const float *d_verts, uint64_t n_verts, const uint32_t *d_faces, uint64_t n_faces, float face_dist,
                   int min_neighbors, MpLayout &L, uint64_t *n_kept) {
  const uint32_t n = (uint32_t)n_faces, min_nb = (uint32_t)min_neighbors;
  int rc = mp_layout(n, s, L);
  if (rc || (rc = w.buf.reserve(L.total, s, "mesh cleanup")) || (rc = mp_work_begin(w, MP_COUNTERS, 4, s))) return rc;
  char *b = (char *)w.buf.p;
  uint64_t *key_a = (uint64_t *)(b + L.key_a), *key_b = (uint64_t *)(b + L.key_b);
  uint32_t *idx_a = (uint32_t *)(b + L.idx_a), *idx_b = (uint32_t *)(b + L.idx_b), *cellno = (uint32_t *)(b + L.cellno);
  float4 *cen = (float4 *)(b + L.cen);
  uint8_t *heavy = (uint8_t *)(b + L.heavy), *any_heavy = (uint8_t *)(b + L.any_heavy), *keep = (uint8_t *)(b + L.keep);
  // free once the sort has run: the unsorted keys' 8 n bytes hold the union-find, the unsorted indices the run heads
  uint32_t *parent = (uint32_t *)key_a, *members = parent + n, *head = idx_a;
  const dim3 blk(256), grid_n((n + 255u) / 256u);

  TSDF_HIP_TRY(hipEventRecord(w.ev[0], s));
  hipLaunchKernelGGL(k_mp_centroid, grid_n, blk, 0, s, d_verts, n_verts, d_faces, n, (double)face_dist, key_a, idx_a, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  size_t tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::radix_sort_pairs(b + L.tmp, tmp_bytes, key_a, key_b, idx_a, idx_b, (size_t)n, 0u, 64u, s));
  hipLaunchKernelGGL(k_mp_gather, grid_n, blk, 0, s, d_verts, n_verts, d_faces, idx_b, key_b, n, cen, head);
  TSDF_HIP_TRY(hipGetLastError());
  tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::inclusive_scan(b + L.tmp, tmp_bytes, head, cellno, (size_t)n, rocprim::plus<uint32_t>(), s));
  TSDF_HIP_TRY(hipEventRecord(w.ev[1], s));
  unsigned long long counts[MP_COUNTERS] = {0};
  uint32_t n_cells = 0;
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), MP_C_TESTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipMemcpyAsync(&n_cells, cellno + (n - 1u), sizeof n_cells, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  if (counts[MP_C_BAD]) {
    tsdf_set_error("tsdf_hip_mesh_cleanup: a face names a vertex index >= n_verts");
    return TSDF_HIP_E_INVALID;
  }
  const uint32_t n_fin = (uint32_t)counts[MP_C_FINITE];
  // (the cell table is sized before the second timed interval opens: a hipMalloc is not device work)
  if (n_fin && (rc = mp_cells_reserve(w, n_cells, s, "mesh cleanup"))) return rc;
  TSDF_HIP_TRY(hipEventRecord(w.ev[2], s));
  if (n_fin) {
    const float r2 = (float)((double)face_dist * (double)face_dist);  // mesh_post.h:129
    MpGrid g{cen, cellno, nullptr, nullptr, n_fin, r2};
    if ((rc = mp_cells_build(w, s, key_b, head, n, n_cells, g))) return rc;
    TSDF_HIP_TRY(hipMemsetAsync(any_heavy, 0, n, s));
    TSDF_HIP_TRY(hipMemsetAsync(members, 0, (size_t)n * 4, s));
    const dim3 grid_f((n_fin + 255u) / 256u);
    hipLaunchKernelGGL(k_mp_degree, grid_f, blk, 0, s, g, min_nb, heavy, parent, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mp_link, grid_f, blk, 0, s, g, heavy, parent, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mp_count, grid_f, blk, 0, s, n_fin, heavy, parent, any_heavy, members);
    TSDF_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_mp_keep, grid_n, blk, 0, s, n, n_fin, min_nb, idx_b, heavy, parent, any_heavy, members, keep, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(w.ev[3], s));
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  // device time = the two intervals on the stream; the host's read of the counts between them (a copy of 8 words, a
  // synchronise, the sizing of the cell table) is not in it
  float ms = 0.f, ms2 = 0.f;
  (void)hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
  (void)hipEventElapsedTime(&ms2, w.ev[2], w.ev[3]);
  ms += ms2;
  uint64_t tests = 0;
  for (int i = 0; i < MP_TEST_SLOTS; ++i) tests += counts[MP_C_TESTS + i];
  g_mp_stats.set(n, n - counts[MP_C_KEPT], tests, (uint64_t)(ms * 1000.f));
  *n_kept = counts[MP_C_KEPT];
  return TSDF_HIP_OK;
}

static int mp_check_args(float face_dist, int min_neighbors, uint64_t n_faces, const char *who) {
  if (!(face_dist > 0.f) || !std::isfinite(face_dist) || min_neighbors < 0) {
    tsdf_set_error(std::string(who) + ": face_dist must be finite and positive, min_neighbors >= 0");
    return TSDF_HIP_E_INVALID;
  }
  return mp_check_counts(who, n_faces, nullptr);
}

extern "C" int tsdf_hip_mesh_cleanup(int device, const float *verts, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces, float face_dist,
                                     int min_neighbors, uint8_t *keep, uint64_t *n_kept) {
  if (n_kept) *n_kept = 0;
  if (const int rc = mp_check_args(face_dist, min_neighbors, n_faces, "tsdf_hip_mesh_cleanup")) return rc;
  if (device < 0) return TSDF_HIP_E_INVALID;
  if (n_faces == 0) {
    g_mp_stats.zero();
    return TSDF_HIP_OK;
  }
  if (!verts || !keep || n_verts == 0 || (!faces && n_verts / 3 < n_faces)) {
    tsdf_set_error("tsdf_hip_mesh_cleanup: verts and keep must not be NULL, and a triangle soup needs 3 vertices per face");
    return TSDF_HIP_E_INVALID;
  }
  MpCall c;
  const size_t b_verts = mp_up((size_t)n_verts * 12), b_faces = faces ? (size_t)n_faces * 12 : 0;
  int rc = c.open(device, b_verts + b_faces, "tsdf_hip_mesh_cleanup");
  if (rc) return rc;
  float *d_verts = (float *)c.in.p;
  uint32_t *d_faces = faces ? (uint32_t *)((char *)c.in.p + b_verts) : nullptr;
  if ((rc = c.upload(d_verts, verts, (size_t)n_verts * 12)) || (faces && (rc = c.upload(d_faces, faces, b_faces)))) return rc;
  MpLayout L;
  uint64_t kept = 0;
  if ((rc = mp_core(c.work, c.s, d_verts, n_verts, d_faces, n_faces, face_dist, min_neighbors, L, &kept))) return rc;
  if ((rc = c.download(keep, (char *)c.work.buf.p + L.keep, (size_t)n_faces))) return rc;
  if (n_kept) *n_kept = kept;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_march_cleanup(tsdf_handle h, float face_dist, int min_neighbors, uint64_t *n_tri) {
  if (!h) return TSDF_HIP_E_INVALID;
  if (n_tri) *n_tri = 0;
  if (const int rc = mp_check_args(face_dist, min_neighbors, 0, "tsdf_hip_march_cleanup")) return rc;
  if (!h->mc_valid) {
    tsdf_set_error("tsdf_hip_march_cleanup: the last tsdf_hip_march on this handle did not succeed, or none has run");
    return TSDF_HIP_E_INVALID;
  }
  tsdf_flatten_invalidate(h);  // (the soup is about to change)
  if (h->multi) return tsdf_multi_march_cleanup(h, face_dist, min_neighbors, n_tri);
  TSDF_ENTER(h);
  const uint64_t n = h->mc_ntri;
  if (const int rc = mp_check_args(face_dist, min_neighbors, n, "tsdf_hip_march_cleanup")) return rc;
  if (!n) {
    g_mp_stats.zero();
    return TSDF_HIP_OK;
  }
  if (!h->mp) h->mp = new tsdf_meshpost_state();
  tsdf_meshpost_state *st = h->mp;
  MpLayout L;
  uint64_t kept = 0;
  int rc = mp_core(st->work, h->stream, h->mc_verts.as<float>(), 3 * n, nullptr, n, face_dist, min_neighbors, L, &kept);
  if (rc) return rc;
  if (kept < n && kept) {
    // stable compaction of vertices, colours and cell keys: each array into the handle's scratch and back (the working set's
    // cell numbers are done with: their 4 n bytes take the offsets)
    char *b = (char *)st->work.buf.p;
    const uint8_t *keep = (const uint8_t *)(b + L.keep);
    uint32_t *offset = (uint32_t *)(b + L.cellno);
    size_t tmp_bytes = L.tmp_bytes;
    TSDF_HIP_TRY(rocprim::exclusive_scan(b + L.tmp, tmp_bytes, MpKeepIt(keep, MpKeepCount()), offset, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                                         h->stream));
    if ((rc = tsdf_ensure_scratch(h, (size_t)kept * 36))) return rc;
    const dim3 blk(256);
    hipLaunchKernelGGL((k_mp_compact<float, 9>), dim3((unsigned)((9 * n + 255) / 256)), blk, 0, h->stream, h->mc_verts.as<float>(), keep, offset, 9 * n,
                       (float *)h->scratch.p);
    TSDF_HIP_TRY(hipGetLastError());
    TSDF_HIP_TRY(hipMemcpyAsync(h->mc_verts.p, h->scratch.p, (size_t)kept * 36, hipMemcpyDeviceToDevice, h->stream));
    if (h->mc_has_rgb) {
      hipLaunchKernelGGL((k_mp_compact<uint8_t, 9>), dim3((unsigned)((9 * n + 255) / 256)), blk, 0, h->stream, h->mc_rgb.as<uint8_t>(), keep, offset, 9 * n,
                         (uint8_t *)h->scratch.p);
      TSDF_HIP_TRY(hipGetLastError());
      TSDF_HIP_TRY(hipMemcpyAsync(h->mc_rgb.p, h->scratch.p, (size_t)kept * 9, hipMemcpyDeviceToDevice, h->stream));
    }
    hipLaunchKernelGGL((k_mp_compact<uint64_t, 1>), dim3((unsigned)((n + 255) / 256)), blk, 0, h->stream, h->mc_cell.as<uint64_t>(), keep, offset, n,
                       (uint64_t *)h->scratch.p);
    TSDF_HIP_TRY(hipGetLastError());
    TSDF_HIP_TRY(hipMemcpyAsync(h->mc_cell.p, h->scratch.p, (size_t)kept * 8, hipMemcpyDeviceToDevice, h->stream));
    TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  h->mc_ntri = kept;
  if (n_tri) *n_tri = kept;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_cleanup_stats(uint64_t out[4]) {
  return g_mp_stats.copy_out(out);
}
