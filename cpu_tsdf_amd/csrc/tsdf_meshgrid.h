// Internal: what the three mesh passes on the GPU -- tsdf_meshpost.hip (cleanupMesh), tsdf_flatten.hip (flattenVertices) and
// tsdf_decimate.hip (decimateMesh) -- share.  Declared here and defined in tsdf_meshgrid.hip: the cell table (the uniform grid
// of cpu_tsdf::mesh_post::PointGrid, csrc/prog/mesh_post.h, over points sorted by the host's cell key), the working set of a
// pass, a handle-less call with its copies of caller memory (PinnedStage, tsdf_own.h: pinned memory directly, pageable
// memory through two pinned slots of MP_STAGE bytes), and the indexed mesh of a handle.  tsdf_smooth.hip (smoothMesh), which moves the vertices of that indexed mesh, and tsdf_normals.hip (meshNormals),
// which reads it or the soup, use the working set, the call and the staging too, and mp_lower_bound.  Defined here, because the passes' own kernels inline or instantiate them: mp_cell_key, mp_for_links (the host's
// forNeighbours), mp_face_remap and k_mp_compact.
#pragma once

#include <optional>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/iterator/transform_iterator.hpp>

#include "tsdf_common.h"

#define MP_STAGE (4u << 20)  // bytes per slot of the pinned staging buffer of the host-array entry point

#define MP_NO_KEY (~0ull)  // a point (face centroid, vertex) that is not finite: in no cell (PointGrid skips it), last in the sorted order

// PointGrid::c / key (mesh_post.h:55-62): floor((double)v / cell), 21 bits per axis; MP_NO_KEY for a point that is not finite.
// Cells that alias under the masks share a bucket, as on the host (the distance test rejects what is far); out_of_range is
// for the pass that cannot live with that (decimate): a cell lies outside [-2^20, 2^20).
static __device__ __forceinline__ uint64_t mp_cell_key(float x, float y, float z, double cell, bool &out_of_range) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return MP_NO_KEY;
  const double fx = floor((double)x / cell), fy = floor((double)y / cell), fz = floor((double)z / cell);
  out_of_range = !(fx >= -1048576.0 && fx < 1048576.0) || !(fy >= -1048576.0 && fy < 1048576.0) || !(fz >= -1048576.0 && fz < 1048576.0);
  const long long cx = (long long)fx, cy = (long long)fy, cz = (long long)fz;
  return ((uint64_t)(cx & 0x1fffff) << 42) | ((uint64_t)(cy & 0x1fffff) << 21) | (uint64_t)(cz & 0x1fffff);
}

// is sorted position i the first point of its cell?
static __device__ __forceinline__ uint32_t mp_cell_head(const uint64_t *__restrict__ keys, uint32_t i, uint64_t key) {
  return key != MP_NO_KEY && (i == 0u || keys[i - 1u] != key) ? 1u : 0u;
}

// one atomic per wave: how many of its lanes say yes
static __device__ __forceinline__ void mp_wave_count(bool yes, unsigned long long *counter) {
  const unsigned long long m = __ballot(yes);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// the first position of the ascending keys[0 .. n_keys) whose key is >= want (n_keys: none is): the row offsets of an inverted
// index whose keys carry the row in their high word
static __device__ __forceinline__ uint32_t mp_lower_bound(const uint64_t *__restrict__ keys, uint32_t n_keys, uint64_t want) {
  uint32_t lo = 0u, hi = n_keys;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo;
}

struct MpGrid {
  const float4 *cen;
  const uint32_t *cellno;
  const int32_t *nbr;
  const uint32_t *cell_start;  // n_cells + 1 entries
  uint32_t n_fin;
  float r2;
};

// f(j) for every j != i with a link to i (mesh_post.h:44-47: (ex * ex + ey * ey) + ez * ez < r2 in float, strict), the own
// cell first; f returns false to stop.  The link test is symmetric bit for bit (ex only changes sign).
template <typename F>
static __device__ __forceinline__ void mp_for_links(const MpGrid &g, uint32_t i, unsigned &tests, F f) {
  const float4 p = g.cen[i];
  const int32_t *nb = g.nbr + 27ull * (g.cellno[i] - 1u);
  for (int k = 0; k < 27; ++k) {
    const int32_t c = nb[k < 14 ? 13 - k : k];  // 13, 12 .. 0, 14 .. 26
    if (c < 0) continue;
    const uint32_t e = g.cell_start[c + 1];
    for (uint32_t j = g.cell_start[c]; j < e; ++j) {
      if (j == i) continue;
      const float4 q = g.cen[j];
      const float ex = q.x - p.x, ey = q.y - p.y, ez = q.z - p.z;
      ++tests;
      if ((ex * ex + ey * ey) + ez * ez < g.r2)
        if (!f(j)) return;
    }
  }
}

// mesh_post.h:107-115: the corners of face f (faces == NULL: the soup's 3 f, 3 f + 1, 3 f + 2) through remap, into r and
// mapped.  true: all three differ.  A face that names a vertex >= n_verts raises *bad and maps to 0, 0, 0.
static __device__ __forceinline__ bool mp_face_remap(const uint32_t *__restrict__ faces, uint32_t f, uint64_t n_verts,
                                                     const uint32_t *__restrict__ remap, uint32_t *__restrict__ mapped, uint32_t r[3],
                                                     unsigned long long *__restrict__ bad) {
  uint64_t a = 3ull * f, b = a + 1ull, c = a + 2ull;
  if (faces) a = faces[3ull * f], b = faces[3ull * f + 1ull], c = faces[3ull * f + 2ull];
  bool good = false;
  r[0] = r[1] = r[2] = 0u;
  if (a >= n_verts || b >= n_verts || c >= n_verts) {
    *bad = 1ull;  // (every writer stores the same 1)
  } else {
    r[0] = remap[a], r[1] = remap[b], r[2] = remap[c];
    good = r[0] != r[1] && r[1] != r[2] && r[2] != r[0];
  }
  mapped[3ull * f] = r[0], mapped[3ull * f + 1ull] = r[1], mapped[3ull * f + 2ull] = r[2];
  return good;
}

// stable compaction of per-triangle records of K elements: one thread per input element
template <typename T, int K>
static __global__ void __launch_bounds__(256)
k_mp_compact(const T *__restrict__ src, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ offset, uint64_t n_elems,
             T *__restrict__ dst) {
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= n_elems) return;
  const uint64_t t = e / (uint64_t)K;
  if (keep[t]) dst[(uint64_t)offset[t] * K + (e - t * K)] = src[e];
}

struct MpKeepCount {
  __host__ __device__ uint32_t operator()(uint8_t k) const { return k ? 1u : 0u; }
};
using MpKeepIt = rocprim::transform_iterator<const uint8_t *, MpKeepCount, uint32_t>;

struct MpWork {  // the working set of one pass: a handle's, or a handle-less call's
  DevBuf buf;       // per-point and per-face arrays + rocprim's temporary storage
  DevBuf cells;     // per-cell arrays (sized once the number of occupied cells is known)
  DevBuf counters;  // unsigned long long each
  EventSet<4> ev;   // timed intervals on the stream (cleanup: two; flatten, decimate: one, ev[0 .. 1])
  unsigned long long *count() const { return counters.as<unsigned long long>(); }
};

// on first use the n_counters counters and the first n_events events; queues the zeroing of the counters
int mp_work_begin(MpWork &w, int n_counters, int n_events, hipStream_t s);

static inline size_t mp_up(size_t v) { return (v + 255) / 256 * 256; }

struct MpTake {  // arrays one behind the other, each on a multiple of 256 bytes: take(bytes) is the next one's offset
  size_t o = 0;
  size_t operator()(size_t bytes) {
    const size_t at = o;
    o += mp_up(bytes);
    return at;
  }
};

// rocprim's temporary storage, the largest of: radix_sort_pairs of n_sort64 (uint64_t, uint32_t) pairs over 64 bits and of
// n_sort32 (uint32_t, uint32_t) pairs over 32, an inclusive scan of n_scan uint32_t, an exclusive scan of n_keep keep flags
int mp_tmp_bytes(size_t n_sort64, size_t n_sort32, size_t n_scan, size_t n_keep, hipStream_t s, size_t *bytes);

// The cell table of n points sorted by key (head: mp_cell_head; g.cellno: the inclusive scan of head, n_cells its last entry;
// g.n_fin: the points with a key), in two steps: room in MpWork::cells, which may allocate; then, queued on the stream, one
// entry per occupied cell, the sentinel cell_start[n_cells] = n_fin and each cell's 27 neighbours, which complete g.
int mp_cells_reserve(MpWork &w, uint32_t n_cells, hipStream_t s, const char *who);
int mp_cells_build(MpWork &w, hipStream_t s, const uint64_t *keys, const uint32_t *head, uint32_t n, uint32_t n_cells, MpGrid &g);

// offset = the exclusive scan of keep; faces_out = the rows of mapped (3 per face) whose keep flag is set, in order
int mp_compact_faces(hipStream_t s, void *tmp, size_t tmp_bytes, const uint32_t *mapped, const uint8_t *keep, uint32_t *offset, uint32_t n_faces,
                     uint32_t *faces_out);

// refuses more than 2^31 faces or vertices (n_verts == NULL: a pass that indexes faces only)
int mp_check_counts(const char *who, uint64_t n_faces, const uint64_t *n_verts);

struct MpStats {  // the four words of a pass's *_stats entry point; each pass keeps a thread_local one
  uint64_t v[4] = {0, 0, 0, 0};
  void zero() { v[0] = v[1] = v[2] = v[3] = 0; }
  void set(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { v[0] = a, v[1] = b, v[2] = c, v[3] = d; }
  int copy_out(uint64_t out[4]) const {
    if (!out) return TSDF_HIP_E_INVALID;
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return TSDF_HIP_OK;
  }
};

// A host-array entry point: everything it allocates goes when it returns (there is no handle to keep it for).  Its copies of
// caller memory are the handle's (PinnedStage, tsdf_own.h) with slots of MP_STAGE bytes, which they were not always: pageable
// results now come back overlapped, not chunk after chunk; an upload from pinned memory waits for its copy before it returns,
// as tsdf_to_device does; and a pageable upload no longer ends with a stream synchronise, the slots' busy flags guarding them
// for the way back.  The bytes and their order are the same.
struct MpCall {
  std::optional<TsdfDeviceScope> scope;  // (first, so restored last)
  hipStream_t s = nullptr;
  DevBuf in;  // the caller's arrays on the device
  MpWork work;
  PinnedStage stage{MP_STAGE};
  ~MpCall();
  // after the caller's own argument checks: is there such a device; on it, a stream and in_bytes for the inputs
  int open(int device, size_t in_bytes, const char *who);
  int upload(void *dst, const void *src, size_t bytes) { return stage.to_device(dst, src, bytes, s); }
  int download(void *dst, const void *src, size_t bytes) { return stage.to_host(dst, src, bytes, s); }
};

#define MP_IDX_COUNTERS 8  // MpWork::counters of the passes that share a handle's tsdf_flatten_state (flatten, decimate)

struct tsdf_flatten_state {  // per handle (tsdf_hip_volume::fl): the indexed mesh of tsdf_hip_march_flatten / _decimate
  MpWork work;
  bool valid = false, has_rgb = false;
  uint64_t n_verts = 0, n_faces = 0;
  DevBuf out;  // one handle: vertices, faces, cell keys, colours (device)
  size_t o_faces = 0, o_cell = 0, o_rgb = 0;
  std::vector<float> h_verts;  // a multi-GPU set: the same on the host, like its soup
  std::vector<uint8_t> h_rgb;
  std::vector<uint32_t> h_faces;
  std::vector<uint64_t> h_cell;
  // tsdf_hip_march_normals (tsdf_normals.hip): the normals of the indexed mesh while it is valid, else of the soup, in a buffer
  // of their own; every later march, cleanup, flatten, decimate, smooth or reset drops them (nm_valid)
  bool nm_valid = false;
  uint64_t nm_n = 0;       // vertices they describe
  DevBuf nm_out;           // one handle: normals, flags (device)
  std::vector<float> h_normals;  // a multi-GPU set: on the host
};

// tsdf_hip_march_flatten / _decimate after their own argument checks: refuses without a marched soup, or one too large for
// 32-bit indices; else *st is the handle's state, no longer valid, and *n the soup's triangles (0: only mp_idx_end is left)
int mp_idx_begin(tsdf_handle h, const char *who, tsdf_flatten_state **st, uint64_t *n);
// One handle (the soup stays as it is: the indexed mesh has buffers of its own): mp_idx_layout sizes st->out for m vertices
// and kept faces; the caller queues its vertices to st->out and colours to st->out + st->o_rgb; mp_idx_fill adds the
// compacted faces and the cell keys of the faces whose keep flag is set, and waits.
int mp_idx_layout(tsdf_handle h, tsdf_flatten_state *st, uint64_t m, uint64_t kept, const char *who);
int mp_idx_fill(tsdf_handle h, tsdf_flatten_state *st, uint64_t m, uint64_t kept, const uint32_t *d_faces, const uint8_t *d_keep,
                const uint32_t *d_offset);
// A set, once the host-array entry point has filled st->h_*: trims them to m vertices and kept faces, and keeps the cell
// keys (cell: one per triangle of the soup) of the faces whose keep flag is set.
void mp_idx_set_host(tsdf_flatten_state *st, bool has_rgb, const uint64_t *cell, uint64_t n, uint64_t m, uint64_t kept, const uint8_t *keep);
int mp_idx_end(tsdf_flatten_state *st, uint64_t *n_verts, uint64_t *n_faces);
