// Internal: what the two mesh passes on the GPU -- tsdf_meshpost.hip (cleanupMesh) and tsdf_flatten.hip (flattenVertices) --
// share: the uniform grid of cpu_tsdf::mesh_post::PointGrid (csrc/prog/mesh_post.h) as device arrays, and the plumbing
// around it.  Both passes sort their points (face centroids / vertices) by the host's cell key, and then
//   k_mp_cells     one entry per occupied cell: key and first sorted position
//   k_mp_cellnbr   each cell's 27 neighbour cells as indices into that table
//   mp_for_links   the points strictly within the radius of point i, from those 27 cells: the host's forNeighbours
//   k_mp_compact   stable compaction of per-face records behind a scan of the keep flags
//   MpWork / mp_reserve / mp_to_device / mp_to_host   the working set, and caller memory (pinned: direct; pageable: staged)
//   tsdf_flatten_state   the indexed mesh of a handle, which tsdf_hip_march_flatten and tsdf_hip_march_decimate
//                  (tsdf_decimate.hip: vertex clustering, on the same cell keys, sort and compaction) both write
// Everything here is static: each translation unit compiles its own copy.
#pragma once

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/iterator/transform_iterator.hpp>

#include "tsdf_common.h"

#define MP_STAGE (4u << 20)  // bytes per slot of the pinned staging buffer of the host-array entry point

#define MP_NO_KEY (~0ull)  // a point (face centroid, vertex) that is not finite: in no cell (PointGrid skips it), last in the sorted order

// cellno: the inclusive scan of head (cell of position i = cellno[i] - 1)
static __global__ void __launch_bounds__(256)
k_mp_cells(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ head, const uint32_t *__restrict__ cellno, uint32_t n,
           uint64_t *__restrict__ cell_key, uint32_t *__restrict__ cell_start) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !head[i]) return;
  const uint32_t c = cellno[i] - 1u;
  cell_key[c] = keys[i];
  cell_start[c] = i;
}

// the 27 cells PointGrid::forNeighbours visits (mesh_post.h:39-43), as indices into the cell table (-1: empty); slot
// (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), so slot 13 is the cell itself
static __global__ void __launch_bounds__(256)
k_mp_cellnbr(const uint64_t *__restrict__ cell_key, uint32_t n_cells, int32_t *__restrict__ nbr) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= 27ull * n_cells) return;
  const uint32_t c = (uint32_t)(t / 27ull), s = (uint32_t)(t - 27ull * c);
  const uint64_t key = cell_key[c];
  const int dx = (int)(s % 3u) - 1, dy = (int)((s / 3u) % 3u) - 1, dz = (int)(s / 9u) - 1;
  const uint64_t want = ((((key >> 42) + (uint64_t)(int64_t)dx) & 0x1fffffull) << 42) | ((((key >> 21) + (uint64_t)(int64_t)dy) & 0x1fffffull) << 21) |
                        ((key + (uint64_t)(int64_t)dz) & 0x1fffffull);
  uint32_t lo = 0u, hi = n_cells;  // the keys ascend
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (cell_key[mid] < want)
      lo = mid + 1u;
    else
      hi = mid;
  }
  nbr[t] = lo < n_cells && cell_key[lo] == want ? (int32_t)lo : -1;
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
  void *buf = nullptr;  // per-point and per-face arrays + rocprim's temporary storage
  size_t cap = 0;
  void *cells = nullptr;  // per-cell arrays (sized once the number of occupied cells is known)
  size_t cells_cap = 0;
  unsigned long long *counters = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // timed intervals on the stream (cleanup: two; flatten: one, ev[0 .. 1])
};

static void mp_work_free(MpWork &w) {
  if (w.buf) (void)hipFree(w.buf);
  if (w.cells) (void)hipFree(w.cells);
  if (w.counters) (void)hipFree(w.counters);
  for (hipEvent_t e : w.ev)
    if (e) (void)hipEventDestroy(e);
  w = MpWork();
}

static int mp_reserve(void **p, size_t *cap, size_t need, hipStream_t s, const char *who = "mesh cleanup") {
  if (need <= *cap && *p) return TSDF_HIP_OK;
  if (*p) {
    TSDF_HIP_TRY(hipStreamSynchronize(s));
    TSDF_HIP_TRY(hipFree(*p));
    *p = nullptr, *cap = 0;
  }
  if (hipMalloc(p, need) != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    tsdf_set_error(std::string(who) + ": " + std::to_string(need) + " bytes of device memory for the working set are not available");
    return TSDF_HIP_E_NOMEM;
  }
  *cap = need;
  return TSDF_HIP_OK;
}

static inline size_t mp_up(size_t v) { return (v + 255) / 256 * 256; }

// Is `p` host memory the runtime knows as pinned?  (As tsdf_to_host / tsdf_to_device decide: the DMA engine then reads and
// writes it directly.)
static bool mp_is_pinned(const void *p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

struct MpStage {  // two pinned slots for pageable caller memory
  char *pinned = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~MpStage() {
    if (pinned) (void)hipHostFree(pinned);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int ready() {
    if (pinned) return TSDF_HIP_OK;
    TSDF_HIP_TRY(hipHostMalloc((void **)&pinned, 2 * (size_t)MP_STAGE, hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) TSDF_HIP_TRY(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    return TSDF_HIP_OK;
  }
};

static int mp_to_device(MpStage &st, void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (!bytes) return TSDF_HIP_OK;
  if (bytes >= (64u << 10) && mp_is_pinned(src)) {
    TSDF_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return TSDF_HIP_OK;
  }
  if (const int rc = st.ready()) return rc;
  for (size_t off = 0, k = 0; off < bytes; off += MP_STAGE, ++k) {
    const int slot = (int)(k & 1);
    if (k >= 2) TSDF_HIP_TRY(hipEventSynchronize(st.ev[slot]));  // the copy that last read this slot has finished
    const size_t len = std::min((size_t)MP_STAGE, bytes - off);
    memcpy(st.pinned + (size_t)slot * MP_STAGE, (const char *)src + off, len);
    TSDF_HIP_TRY(hipMemcpyAsync((char *)dst + off, st.pinned + (size_t)slot * MP_STAGE, len, hipMemcpyHostToDevice, s));
    TSDF_HIP_TRY(hipEventRecord(st.ev[slot], s));
  }
  TSDF_HIP_TRY(hipStreamSynchronize(s));  // (the slots are free again for the way back)
  return TSDF_HIP_OK;
}

static int mp_to_host(MpStage &st, void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (!bytes) return TSDF_HIP_OK;
  if (bytes >= (64u << 10) && mp_is_pinned(dst)) {
    TSDF_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    TSDF_HIP_TRY(hipStreamSynchronize(s));
    return TSDF_HIP_OK;
  }
  if (const int rc = st.ready()) return rc;
  for (size_t off = 0; off < bytes; off += MP_STAGE) {
    const size_t len = std::min((size_t)MP_STAGE, bytes - off);
    TSDF_HIP_TRY(hipMemcpyAsync(st.pinned, (const char *)src + off, len, hipMemcpyDeviceToHost, s));
    TSDF_HIP_TRY(hipStreamSynchronize(s));
    memcpy((char *)dst + off, st.pinned, len);
  }
  return TSDF_HIP_OK;
}

#define MP_IDX_COUNTERS 8  // MpWork::counters of the passes that share a handle's tsdf_flatten_state (flatten, decimate)

struct tsdf_flatten_state {  // per handle (tsdf_hip_volume::fl): the indexed mesh of tsdf_hip_march_flatten / _decimate
  MpWork work;
  bool valid = false, has_rgb = false;
  uint64_t n_verts = 0, n_faces = 0;
  void *out = nullptr;  // one handle: vertices, faces, cell keys, colours (device)
  size_t out_cap = 0, o_faces = 0, o_cell = 0, o_rgb = 0;
  std::vector<float> h_verts;  // a multi-GPU set: the same on the host, like its soup
  std::vector<uint8_t> h_rgb;
  std::vector<uint32_t> h_faces;
  std::vector<uint64_t> h_cell;
};
