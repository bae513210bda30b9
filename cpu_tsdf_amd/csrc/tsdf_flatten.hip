// libtsdf_hip.so -- merging the duplicate vertices of a triangle mesh.
//
// Replaces flattenVertices of the reference's `integrate` program (src/prog/integrate.cpp:103-150), as this repository's
// host restatement cpu_tsdf::mesh_post::flattenVertices (csrc/prog/mesh_post.h) defines it operation for operation.  That
// pass is a serial loop over the vertices in index order; its RESULT is a function of the input alone.
// Two vertices are NEIGHBOURS when the host's test holds between them (symmetric bit for bit); then
//   1. vertex i is a SEED (opens an output vertex) iff no earlier seed is its neighbour: the lexicographically first
//      maximal independent set of the neighbour graph in index order.  Iterated to a fixed point: an undecided vertex is
//      MERGED as soon as one earlier neighbour is a seed, and a SEED as soon as all earlier neighbours are merged.  The
//      lowest undecided vertex always decides, so at most n rounds; in fact as many as the longest index-ordered chain.
//   2. remap[j] of a merged vertex is the output index of the HIGHEST seed among its neighbours (the loop lets every seed
//      overwrite its neighbours' entries: the last writer wins); of a seed, its own.
//   3. the output index of a seed is the number of seeds before it: an exclusive scan of the seed flags.
// Kernels:
//   k_fl_key       the host's cell key per finite vertex (a non-finite vertex is in no cell: a seed that merges nothing)
//   rocprim sort   (key, vertex) pairs, stable; k_fl_gather writes the positions in sorted order and marks run heads, a scan
//                  numbers the cells, mp_cells_build (tsdf_meshgrid.hip) makes the cell table
//   k_fl_round     one round of rule 1 over the list of still undecided vertices, which it compacts for the next round
//   k_fl_remap     rule 2; rocprim scan: rule 3; k_fl_out: remap and the seed list by output index
//   k_fl_faces     per face: remapped corners, keep = all three differ; mp_compact_faces (scan + k_mp_compact) keeps the order
// The state word of a vertex carries the round that decided it, and a round ignores what the same round decided: every
// round sees exactly the state the round before left, whatever the order the workgroups run in (so the number of rounds is
// the depth of the dependency chains, the same in every run), and no kernel waits for another workgroup.
// Gather-bound pointer chasing and a radix sort: no MFMA.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "tsdf_meshgrid.h"

// ---- state -----------------------------------------------------------------------------------------------------------------
#define FL_C_FINITE 0  // vertices with three finite coordinates
#define FL_C_BAD 1     // != 0: a face names a vertex >= n_verts
#define FL_C_ROUNDS 2  // rounds that found an undecided vertex
#define FL_C_SEEDS 3
#define FL_C_KEPT 4
#define FL_C_LIST 5  // three list lengths in rotation: round r reads r % 3, appends to (r + 1) % 3, zeroes (r + 2) % 3
#define FL_COUNTERS MP_IDX_COUNTERS
#define FL_MAX_ROUNDS 0x7fffffffu  // the state word holds round << 1

// (tsdf_flatten_state, the indexed mesh of a handle, and the mp_idx_* that write it are in tsdf_meshgrid.h / .hip:
// tsdf_decimate.hip writes it too)

static thread_local MpStats g_fl_stats;  // tsdf_hip_mesh_flatten_stats

void tsdf_flatten_invalidate(tsdf_hip_volume *v) {
  if (v->fl) v->fl->valid = v->fl->nm_valid = false;  // (normals describe the mesh they were made from: tsdf_normals.hip)
}

void tsdf_flatten_release(tsdf_hip_volume *v) {
  if (!v->fl) return;
  TsdfDeviceScope scope(v->device);  // (a set keeps its indexed mesh on the host: work and out are empty)
  delete v->fl;
  v->fl = nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_fl_key(const float *__restrict__ verts, uint32_t n, double cell, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
         unsigned long long *__restrict__ counters) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  bool fin = false;
  if (v < n) {
    const float x = verts[3ull * v], y = verts[3ull * v + 1ull], z = verts[3ull * v + 2ull];
    bool wraps = false;  // (cells that alias under the key's masks share a bucket, as on the host)
    const uint64_t key = mp_cell_key(x, y, z, cell, wraps);
    fin = key != MP_NO_KEY;
    keys[v] = key;
    idx[v] = v;
  }
  mp_wave_count(fin, &counters[FL_C_FINITE]);
}

// sorted position i -> position of the vertex there, and "first vertex of its cell"
static __global__ void __launch_bounds__(256)
k_fl_gather(const float *__restrict__ verts, const uint32_t *__restrict__ order, const uint64_t *__restrict__ keys, uint32_t n,
            float4 *__restrict__ pos, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const uint64_t v = order[i];
  pos[i] = make_float4(verts[3ull * v], verts[3ull * v + 1ull], verts[3ull * v + 2ull], 0.f);
  head[i] = mp_cell_head(keys, i, key);
}

// State of the vertex at a sorted position: 0 = undecided, else (round that decided it) << 1 | (1 = seed, 0 = merged).
// Written once, by the thread that owns the vertex; read by others in later launches (and, ignored, in the same one).  The
// accesses are agent-scope atomics, as in mp_find: a plain load may be served from a line another launch left in a cache.
static __device__ __forceinline__ uint32_t fl_load(const uint32_t *state, uint32_t i) {
  return __hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Round `round` (1, 2, ..) of rule 1.  list_in == NULL: every finite vertex (round 1); otherwise the cnt[slot_in] positions
// the round before left undecided.  A vertex that stays undecided goes to list_out.  The grid covers an upper bound of the
// list's length (the host reads the true one only every few rounds).
static __global__ void __launch_bounds__(256)
k_fl_round(const MpGrid g, const uint32_t *__restrict__ order, uint32_t *__restrict__ state, const uint32_t *__restrict__ list_in,
           uint32_t *__restrict__ list_out, unsigned long long *__restrict__ counters, int slot_in, int slot_out, int slot_zero, uint32_t round) {
  unsigned long long *cnt = counters + FL_C_LIST;
  const uint32_t n_in = list_in ? (uint32_t)cnt[slot_in] : g.n_fin;
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    cnt[slot_zero] = 0ull;  // (the next round appends there; nobody touches it in this one)
    if (n_in) counters[FL_C_ROUNDS] += 1ull;
  }
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  bool still = false;
  uint32_t i = 0u;
  if (t < n_in) {
    i = list_in ? list_in[t] : t;
    const uint32_t me = order[i];
    bool merged = false, pending = false;
    unsigned tests = 0u;
    mp_for_links(g, i, tests, [&](uint32_t j) {
      if (order[j] > me) return true;  // only earlier vertices decide (j != i, so never equal)
      const uint32_t s = fl_load(state, j);
      if (s == 0u || (s >> 1) >= round) {
        pending = true;  // undecided when this round began
        return true;
      }
      merged = (s & 1u) != 0u;
      return !merged;
    });
    if (merged)
      __hip_atomic_store(&state[i], round << 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (!pending)
      __hip_atomic_store(&state[i], (round << 1) | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      still = true;
  }
  // one atomic per wave; the order inside the list does not matter
  const unsigned long long m = __ballot(still);
  if (m) {
    const unsigned lane = threadIdx.x & 63u, leader = (unsigned)__ffsll((long long)m) - 1u;
    uint32_t base = 0u;
    if (lane == leader) base = (uint32_t)atomicAdd(&cnt[slot_out], (unsigned long long)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (still) list_out[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
  }
}

// Rule 2, per ORIGINAL vertex index: is it a seed, and which seed's output vertex it takes.
static __global__ void __launch_bounds__(256)
k_fl_remap(const MpGrid g, uint32_t n, const uint32_t *__restrict__ order, const uint32_t *__restrict__ state, uint8_t *__restrict__ flag,
           uint32_t *__restrict__ seed_of, unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool seed = false;
  if (i < n) {
    const uint32_t me = order[i];
    uint32_t best = me;
    seed = i >= g.n_fin || (fl_load(state, i) & 1u);  // positions >= n_fin: not finite, no neighbour, not even itself
    if (!seed) {
      best = 0u;  // (a merged vertex has a seed among its neighbours: that is what merged it)
      unsigned tests = 0u;
      mp_for_links(g, i, tests, [&](uint32_t j) {
        if (fl_load(state, j) & 1u) best = max(best, order[j]);
        return true;
      });
    }
    flag[me] = seed ? 1 : 0;
    seed_of[me] = best;
  }
  mp_wave_count(seed, &counters[FL_C_SEEDS]);
}

// outidx: the exclusive scan of flag (rule 3)
static __global__ void __launch_bounds__(256)
k_fl_out(uint32_t n, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ seed_of, const uint32_t *__restrict__ outidx,
         uint32_t *__restrict__ remap, uint32_t *__restrict__ seeds) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n) return;
  remap[v] = outidx[seed_of[v]];
  if (flag[v]) seeds[outidx[v]] = v;
}

// mesh_post.h:107-115: the corners through remap; a face with two equal corners goes
static __global__ void __launch_bounds__(256)
k_fl_faces(const uint32_t *__restrict__ faces, uint32_t n_faces, uint64_t n_verts, const uint32_t *__restrict__ remap,
           uint32_t *__restrict__ mapped, uint8_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  bool k = false;
  if (f < n_faces) {
    uint32_t r[3];
    k = mp_face_remap(faces, f, n_verts, remap, mapped, r, &counters[FL_C_BAD]);
    keep[f] = k ? 1 : 0;
  }
  mp_wave_count(k, &counters[FL_C_KEPT]);
}

// output vertex o = the seed's position and, on the device-resident path, its colour
static __global__ void __launch_bounds__(256)
k_fl_gather_out(const float *__restrict__ verts, const uint8_t *__restrict__ rgb, const uint32_t *__restrict__ seeds, uint32_t m,
                float *__restrict__ out_verts, uint8_t *__restrict__ out_rgb) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o >= m) return;
  const uint64_t v = seeds[o];
#pragma unroll
  for (int k = 0; k < 3; ++k) out_verts[3ull * o + k] = verts[3ull * v + k];
  if (rgb) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_rgb[3ull * o + k] = rgb[3ull * v + k];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct FlLayout {  // the arrays inside MpWork::buf
  size_t key_a, key_b, idx_a, idx_b, pos, cellno, flag, remap, seeds, mapped, faces, keep, offset, tmp, tmp_bytes, total;
};

static int fl_layout(size_t n, size_t f, hipStream_t s, FlLayout &L) {
  if (const int rc = mp_tmp_bytes(n, 0, n, std::max(n, f), s, &L.tmp_bytes)) return rc;
  MpTake take;
  L.key_a = take(n * 8), L.key_b = take(n * 8), L.idx_a = take(n * 4), L.idx_b = take(n * 4), L.pos = take(n * 16);
  L.cellno = take(n * 4), L.flag = take(n), L.remap = take(n * 4), L.seeds = take(n * 4);
  L.mapped = take(f * 12), L.faces = take(f * 12), L.keep = take(f), L.offset = take(f * 4);
  L.tmp = take(L.tmp_bytes);
  L.total = take.o;
  return TSDF_HIP_OK;
}

// The whole pass on device arrays.  Leaves in MpWork::buf: remap (n_verts), seeds (*n_out), the surviving faces (L.faces,
// *n_kept x 3), the faces' keep flags and, when a face went, their offsets; and the stats of the calling thread.  Leaves the
// stream idle.
static int fl_core(MpWork &w, hipStream_t s, const float *d_verts, uint64_t n_verts, const uint32_t *d_faces, uint64_t n_faces, float min_dist,
                   FlLayout &L, uint64_t *n_out, uint64_t *n_kept, const char *who) {
  const uint32_t n = (uint32_t)n_verts, nf = (uint32_t)n_faces;
  int rc = fl_layout(n, nf, s, L);
  if (rc || (rc = w.buf.reserve(L.total, s, "mesh flatten")) || (rc = mp_work_begin(w, FL_COUNTERS, 2, s))) return rc;
  char *b = (char *)w.buf.p;
  uint64_t *key_a = (uint64_t *)(b + L.key_a), *key_b = (uint64_t *)(b + L.key_b);
  uint32_t *idx_a = (uint32_t *)(b + L.idx_a), *order = (uint32_t *)(b + L.idx_b), *cellno = (uint32_t *)(b + L.cellno);
  float4 *pos = (float4 *)(b + L.pos);
  uint8_t *flag = (uint8_t *)(b + L.flag), *keep = (uint8_t *)(b + L.keep);
  uint32_t *remap = (uint32_t *)(b + L.remap), *seeds = (uint32_t *)(b + L.seeds), *mapped = (uint32_t *)(b + L.mapped);
  uint32_t *faces_out = (uint32_t *)(b + L.faces), *offset = (uint32_t *)(b + L.offset);
  // free once the sort has run: the unsorted keys' 8 n bytes hold the state and one list, the unsorted indices the run heads
  // and then the other list; free once the cell table stands: the sorted keys' 8 n bytes hold rule 2's and rule 3's arrays
  uint32_t *state = (uint32_t *)key_a, *list[2] = {state + n, idx_a}, *head = idx_a;
  uint32_t *seed_of = (uint32_t *)key_b, *outidx = seed_of + n;
  const dim3 blk(256), grid_n((n + 255u) / 256u);

  TSDF_HIP_TRY(hipEventRecord(w.ev[0], s));
  hipLaunchKernelGGL(k_fl_key, grid_n, blk, 0, s, d_verts, n, (double)min_dist, key_a, idx_a, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  size_t tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::radix_sort_pairs(b + L.tmp, tmp_bytes, key_a, key_b, idx_a, order, (size_t)n, 0u, 64u, s));
  hipLaunchKernelGGL(k_fl_gather, grid_n, blk, 0, s, d_verts, order, key_b, n, pos, head);
  TSDF_HIP_TRY(hipGetLastError());
  tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::inclusive_scan(b + L.tmp, tmp_bytes, head, cellno, (size_t)n, rocprim::plus<uint32_t>(), s));
  unsigned long long counts[FL_COUNTERS] = {0};
  uint32_t n_cells = 0;
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipMemcpyAsync(&n_cells, cellno + (n - 1u), sizeof n_cells, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  const uint32_t n_fin = (uint32_t)counts[FL_C_FINITE];
  MpGrid g{pos, cellno, nullptr, nullptr, n_fin, 0.f};
  if (n_fin) {
    if ((rc = mp_cells_reserve(w, n_cells, s, "mesh flatten")) || (rc = mp_cells_build(w, s, key_b, head, n, n_cells, g))) return rc;
    TSDF_HIP_TRY(hipMemsetAsync(state, 0, (size_t)n * 4, s));
    // mesh_post.h:96,103: the squared distance is compared with min_dist * min_dist AND with min_dist itself
    // (integrate.cpp:124), so with the smaller of the two; its root is <= min_dist, so the 27 cells hold every neighbour
    const float r2 = (float)((double)min_dist * (double)min_dist);
    g.r2 = r2 < min_dist ? r2 : min_dist;
    // rule 1.  The host reads the list's length only once per batch of rounds; the rounds of a batch after the one that
    // emptied the list find nothing to do.
    uint32_t undecided = n_fin, round = 0u, batch = 4u;
    while (undecided) {
      if (round >= n_fin || round + batch >= FL_MAX_ROUNDS) {
        tsdf_set_error(std::string(who) + ": " + std::to_string(undecided) + " vertices are undecided after " + std::to_string(round) +
                       " rounds (every round decides at least the lowest one: this cannot happen)");
        return TSDF_HIP_E_HIP;
      }
      const dim3 grid_u((undecided + 255u) / 256u);
      for (uint32_t k = 0; k < batch; ++k) {
        ++round;
        hipLaunchKernelGGL(k_fl_round, grid_u, blk, 0, s, g, order, state, round == 1u ? nullptr : list[round & 1u], list[(round + 1u) & 1u],
                           w.count(), (int)(round % 3u), (int)((round + 1u) % 3u), (int)((round + 2u) % 3u), round);
        TSDF_HIP_TRY(hipGetLastError());
      }
      unsigned long long left = 0;
      TSDF_HIP_TRY(hipMemcpyAsync(&left, w.count() + FL_C_LIST + (round + 1u) % 3u, sizeof left, hipMemcpyDeviceToHost, s));
      TSDF_HIP_TRY(hipStreamSynchronize(s));
      undecided = (uint32_t)left;
      batch = std::min(64u, batch * 2u);
    }
  }
  hipLaunchKernelGGL(k_fl_remap, grid_n, blk, 0, s, g, n, order, state, flag, seed_of, w.count());
  TSDF_HIP_TRY(hipGetLastError());
  tmp_bytes = L.tmp_bytes;
  TSDF_HIP_TRY(rocprim::exclusive_scan(b + L.tmp, tmp_bytes, MpKeepIt(flag, MpKeepCount()), outidx, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_fl_out, grid_n, blk, 0, s, n, flag, seed_of, outidx, remap, seeds);
  TSDF_HIP_TRY(hipGetLastError());
  if (nf) {
    hipLaunchKernelGGL(k_fl_faces, dim3((nf + 255u) / 256u), blk, 0, s, d_faces, nf, n_verts, remap, mapped, keep, w.count());
    TSDF_HIP_TRY(hipGetLastError());
    if ((rc = mp_compact_faces(s, b + L.tmp, L.tmp_bytes, mapped, keep, offset, nf, faces_out))) return rc;
  }
  TSDF_HIP_TRY(hipEventRecord(w.ev[1], s));
  TSDF_HIP_TRY(hipMemcpyAsync(counts, w.count(), sizeof counts, hipMemcpyDeviceToHost, s));
  TSDF_HIP_TRY(hipStreamSynchronize(s));
  if (counts[FL_C_BAD]) {
    tsdf_set_error(std::string(who) + ": a face names a vertex index >= n_verts");
    return TSDF_HIP_E_INVALID;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
  g_fl_stats.set(n, counts[FL_C_SEEDS], counts[FL_C_ROUNDS], (uint64_t)(ms * 1000.f));
  *n_out = counts[FL_C_SEEDS];
  *n_kept = counts[FL_C_KEPT];
  return TSDF_HIP_OK;
}

static int fl_check_args(float min_dist, uint64_t n_verts, uint64_t n_faces, const char *who) {
  if (!(min_dist > 0.f) || !std::isfinite(min_dist)) {
    tsdf_set_error(std::string(who) + ": min_dist must be finite and positive");
    return TSDF_HIP_E_INVALID;
  }
  return mp_check_counts(who, n_faces, &n_verts);
}

extern "C" int tsdf_hip_mesh_flatten(int device, const float *verts, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces, float min_dist,
                                     uint32_t *remap, uint32_t *seeds, uint64_t *n_out_verts, uint32_t *out_faces, uint64_t *n_out_faces) {
  if (n_out_verts) *n_out_verts = 0;
  if (n_out_faces) *n_out_faces = 0;
  if (const int rc = fl_check_args(min_dist, n_verts, n_faces, "tsdf_hip_mesh_flatten")) return rc;
  if (device < 0) return TSDF_HIP_E_INVALID;
  if ((n_verts && !verts) || (seeds && !n_out_verts) || (out_faces && !n_out_faces)) {
    tsdf_set_error("tsdf_hip_mesh_flatten: verts must not be NULL, and seeds / out_faces need n_out_verts / n_out_faces");
    return TSDF_HIP_E_INVALID;
  }
  if (!faces && n_verts / 3 < n_faces) {
    tsdf_set_error("tsdf_hip_mesh_flatten: a triangle soup needs 3 vertices per face");
    return TSDF_HIP_E_INVALID;
  }
  if (n_verts == 0) {
    if (n_faces) {
      tsdf_set_error("tsdf_hip_mesh_flatten: a face names a vertex index >= n_verts");
      return TSDF_HIP_E_INVALID;
    }
    g_fl_stats.zero();
    return TSDF_HIP_OK;
  }
  MpCall c;
  const size_t b_verts = mp_up((size_t)n_verts * 12), b_faces = faces ? (size_t)n_faces * 12 : 0;
  int rc = c.open(device, b_verts + b_faces, "tsdf_hip_mesh_flatten");
  if (rc) return rc;
  float *d_verts = (float *)c.in.p;
  uint32_t *d_faces = faces && n_faces ? (uint32_t *)((char *)c.in.p + b_verts) : nullptr;
  if ((rc = c.upload(d_verts, verts, (size_t)n_verts * 12)) || (d_faces && (rc = c.upload(d_faces, faces, b_faces)))) return rc;
  FlLayout L;
  uint64_t m = 0, kept = 0;
  if ((rc = fl_core(c.work, c.s, d_verts, n_verts, d_faces, n_faces, min_dist, L, &m, &kept, "tsdf_hip_mesh_flatten"))) return rc;
  const char *b = (const char *)c.work.buf.p;
  if (remap && (rc = c.download(remap, b + L.remap, (size_t)n_verts * 4))) return rc;
  if (seeds && (rc = c.download(seeds, b + L.seeds, (size_t)m * 4))) return rc;
  if (out_faces && (rc = c.download(out_faces, b + L.faces, (size_t)kept * 12))) return rc;
  if (n_out_verts) *n_out_verts = m;
  if (n_out_faces) *n_out_faces = kept;
  return TSDF_HIP_OK;
}

// A set: the merged soup is on the host, so it takes the host-array entry point on the first slab's device, and the indexed
// mesh stays on the host too -- what one handle holding the whole grid would fetch.
static int fl_multi(tsdf_handle h, tsdf_flatten_state *st, float min_dist) {
  const uint64_t n = h->mc_ntri;
  const float *verts = nullptr;
  const uint8_t *rgb = nullptr;
  const uint64_t *cell = nullptr;
  tsdf_multi_mesh(h, &verts, &rgb, &cell);
  std::vector<uint32_t> remap((size_t)n * 3), seeds((size_t)n * 3);
  st->h_faces.resize((size_t)n * 3);
  uint64_t m = 0, kept = 0;
  const int rc = tsdf_hip_mesh_flatten(tsdf_multi_first(h)->device, verts, 3 * n, nullptr, n, min_dist, remap.data(), seeds.data(), &m,
                                       st->h_faces.data(), &kept);
  if (rc) return rc;
  std::vector<uint8_t> keep((size_t)n);  // mesh_post.h:107-115, as k_fl_faces decided
  for (uint64_t f = 0; f < n; ++f) {
    const uint32_t a = remap[3 * f], b = remap[3 * f + 1], c = remap[3 * f + 2];
    keep[f] = a != b && b != c && c != a;
  }
  mp_idx_set_host(st, rgb != nullptr, cell, n, m, kept, keep.data());
  for (uint64_t o = 0; o < m; ++o) {
    memcpy(&st->h_verts[3 * o], verts + 3ull * seeds[o], 3 * sizeof(float));
    if (rgb) memcpy(&st->h_rgb[3 * o], rgb + 3ull * seeds[o], 3);
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_march_flatten(tsdf_handle h, float min_dist, uint64_t *n_verts, uint64_t *n_faces) {
  const char *who = "tsdf_hip_march_flatten";
  if (!h) return TSDF_HIP_E_INVALID;
  if (n_verts) *n_verts = 0;
  if (n_faces) *n_faces = 0;
  tsdf_flatten_state *st = nullptr;
  uint64_t n = 0;
  int rc = fl_check_args(min_dist, 0, 0, who);
  if (rc || (rc = mp_idx_begin(h, who, &st, &n))) return rc;
  if (!n) {
    g_fl_stats.zero();
  } else if (h->multi) {
    if ((rc = fl_multi(h, st, min_dist))) return rc;
  } else {
    TSDF_ENTER(h);
    FlLayout L;
    uint64_t m = 0, kept = 0;
    if ((rc = fl_core(st->work, h->stream, h->mc_verts.as<float>(), 3 * n, nullptr, n, min_dist, L, &m, &kept, who))) return rc;
    if ((rc = mp_idx_layout(h, st, m, kept, "mesh flatten"))) return rc;
    const char *b = (const char *)st->work.buf.p;
    char *o = (char *)st->out.p;
    hipLaunchKernelGGL(k_fl_gather_out, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, h->mc_verts.as<float>(), h->mc_has_rgb ? h->mc_rgb.as<uint8_t>() : nullptr,
                       (const uint32_t *)(b + L.seeds), (uint32_t)m, (float *)o, (uint8_t *)(o + st->o_rgb));
    TSDF_HIP_TRY(hipGetLastError());
    if ((rc = mp_idx_fill(h, st, m, kept, (const uint32_t *)(b + L.faces), (const uint8_t *)(b + L.keep), (const uint32_t *)(b + L.offset)))) return rc;
  }
  return mp_idx_end(st, n_verts, n_faces);
}

extern "C" int tsdf_hip_march_fetch_indexed(tsdf_handle h, float *verts, uint8_t *rgb, uint32_t *faces, uint64_t *cell) {
  if (!h) return TSDF_HIP_E_INVALID;
  tsdf_flatten_state *st = h->fl;
  if (!st || !st->valid) {
    tsdf_set_error("tsdf_hip_march_fetch_indexed: no indexed mesh: tsdf_hip_march_flatten has not run since the last tsdf_hip_march / "
                   "tsdf_hip_march_cleanup");
    return TSDF_HIP_E_INVALID;
  }
  if (rgb && !st->has_rgb && st->n_verts) {
    tsdf_set_error("the last tsdf_hip_march ran without a colour mode");
    return TSDF_HIP_E_INVALID;
  }
  const size_t m = (size_t)st->n_verts, k = (size_t)st->n_faces;
  if (h->multi) {
    if (verts && m) memcpy(verts, st->h_verts.data(), m * 12);
    if (rgb && m) memcpy(rgb, st->h_rgb.data(), m * 3);
    if (faces && k) memcpy(faces, st->h_faces.data(), k * 12);
    if (cell && k) memcpy(cell, st->h_cell.data(), k * 8);
    return TSDF_HIP_OK;
  }
  if (!m) return TSDF_HIP_OK;
  TSDF_ENTER(h);
  const char *o = (const char *)st->out.p;
  int rc = TSDF_HIP_OK;
  if (verts && (rc = tsdf_to_host(h, verts, o, m * 12))) return rc;
  if (rgb && (rc = tsdf_to_host(h, rgb, o + st->o_rgb, m * 3))) return rc;
  if (faces && k && (rc = tsdf_to_host(h, faces, o + st->o_faces, k * 12))) return rc;
  if (cell && k && (rc = tsdf_to_host(h, cell, o + st->o_cell, k * 8))) return rc;
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_mesh_flatten_stats(uint64_t out[4]) {
  return g_fl_stats.copy_out(out);
}
