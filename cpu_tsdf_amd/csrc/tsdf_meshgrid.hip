// libtsdf_hip.so -- what the three mesh passes share (tsdf_meshgrid.h): the cell table over sorted points, the working set, a
// handle-less call with its staged copies of caller memory, and the indexed mesh a handle keeps.
//
// The passes themselves are tsdf_meshpost.hip (cleanupMesh), tsdf_flatten.hip (flattenVertices) and tsdf_decimate.hip
// (decimateMesh); each is its own algorithm plus calls into this file.  Two small kernels and host plumbing: no MFMA.
#include <string.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "tsdf_meshgrid.h"

// ---- the cell table ----------------------------------------------------------------------------------------------------------

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

struct MpCellLayout {  // MpWork::cells: cell_key (at 0), cell_start, nbr
  size_t start, nbr, total;
  explicit MpCellLayout(size_t n_cells)
      : start(mp_up(n_cells * 8)), nbr(start + mp_up((n_cells + 1) * 4)), total(nbr + n_cells * 27 * 4) {}
};

int mp_cells_reserve(MpWork &w, uint32_t n_cells, hipStream_t s, const char *who) {
  return w.cells.reserve(MpCellLayout(n_cells).total, s, who);
}

int mp_cells_build(MpWork &w, hipStream_t s, const uint64_t *keys, const uint32_t *head, uint32_t n, uint32_t n_cells, MpGrid &g) {
  const MpCellLayout C(n_cells);
  uint64_t *cell_key = (uint64_t *)w.cells.p;
  uint32_t *cell_start = (uint32_t *)((char *)w.cells.p + C.start);
  int32_t *nbr = (int32_t *)((char *)w.cells.p + C.nbr);
  const dim3 blk(256);
  hipLaunchKernelGGL(k_mp_cells, dim3((n + 255u) / 256u), blk, 0, s, keys, head, g.cellno, n, cell_key, cell_start);
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(cell_start + n_cells), (int)g.n_fin, 1, s));
  hipLaunchKernelGGL(k_mp_cellnbr, dim3((unsigned)((27ull * n_cells + 255ull) / 256ull)), blk, 0, s, cell_key, n_cells, nbr);
  TSDF_HIP_TRY(hipGetLastError());
  g.nbr = nbr, g.cell_start = cell_start;
  return TSDF_HIP_OK;
}

// ---- the working set ---------------------------------------------------------------------------------------------------------
int mp_work_begin(MpWork &w, int n_counters, int n_events, hipStream_t s) {
  if (const int rc = w.counters.reserve((size_t)n_counters * sizeof(unsigned long long), s)) return rc;
  if (const int rc = w.ev.ensure(n_events)) return rc;
  TSDF_HIP_TRY(hipMemsetAsync(w.count(), 0, (size_t)n_counters * sizeof(unsigned long long), s));
  return TSDF_HIP_OK;
}

int mp_tmp_bytes(size_t n_sort64, size_t n_sort32, size_t n_scan, size_t n_keep, hipStream_t s, size_t *bytes) {
  size_t t[4] = {0, 0, 0, 0};
  if (n_sort64)
    TSDF_HIP_TRY(rocprim::radix_sort_pairs(nullptr, t[0], (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                           n_sort64, 0u, 64u, s));
  if (n_sort32)
    TSDF_HIP_TRY(rocprim::radix_sort_pairs(nullptr, t[1], (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                           n_sort32, 0u, 32u, s));
  if (n_scan) TSDF_HIP_TRY(rocprim::inclusive_scan(nullptr, t[2], (uint32_t *)nullptr, (uint32_t *)nullptr, n_scan, rocprim::plus<uint32_t>(), s));
  if (n_keep)
    TSDF_HIP_TRY(rocprim::exclusive_scan(nullptr, t[3], MpKeepIt(nullptr, MpKeepCount()), (uint32_t *)nullptr, 0u, n_keep, rocprim::plus<uint32_t>(), s));
  *bytes = *std::max_element(t, t + 4);
  return TSDF_HIP_OK;
}

int mp_compact_faces(hipStream_t s, void *tmp, size_t tmp_bytes, const uint32_t *mapped, const uint8_t *keep, uint32_t *offset, uint32_t n_faces,
                     uint32_t *faces_out) {
  TSDF_HIP_TRY(rocprim::exclusive_scan(tmp, tmp_bytes, MpKeepIt(keep, MpKeepCount()), offset, 0u, (size_t)n_faces, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL((k_mp_compact<uint32_t, 3>), dim3((unsigned)((3ull * n_faces + 255ull) / 256ull)), dim3(256), 0, s, mapped, keep, offset,
                     3ull * n_faces, faces_out);
  TSDF_HIP_TRY(hipGetLastError());
  return TSDF_HIP_OK;
}

int mp_check_counts(const char *who, uint64_t n_faces, const uint64_t *n_verts) {
  if ((n_verts && *n_verts > (1ull << 31)) || n_faces > (1ull << 31)) {
    tsdf_set_error(std::string(who) + (n_verts ? ": vertex and face indices are 32-bit; more than 2^31 vertices or faces are not accepted"
                                               : ": face indices are 32-bit; more than 2^31 faces are not accepted"));
    return TSDF_HIP_E_INVALID;
  }
  return TSDF_HIP_OK;
}

// ---- a handle-less call ------------------------------------------------------------------------------------------------------
MpCall::~MpCall() {  // (the members free their memory after this, the stream being idle)
  if (s) (void)hipStreamSynchronize(s);
  if (s) (void)hipStreamDestroy(s);
}

int MpCall::open(int device, size_t in_bytes, const char *who) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return TSDF_HIP_E_NODEVICE;
  }
  if (device >= n_dev) return TSDF_HIP_E_INVALID;
  scope.emplace(device);
  TSDF_HIP_TRY(scope->err);
  TSDF_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  if (in.alloc(in_bytes)) {
    tsdf_set_error(std::string(who) + ": " + std::to_string(in_bytes) + " bytes of device memory for the mesh are not available");
    return TSDF_HIP_E_NOMEM;
  }
  return TSDF_HIP_OK;
}

// ---- the indexed mesh of a handle ----------------------------------------------------------------------------------------------
int mp_idx_begin(tsdf_handle h, const char *who, tsdf_flatten_state **st_out, uint64_t *n_out) {
  if (!h->mc_valid) {
    tsdf_set_error(std::string(who) + ": the last tsdf_hip_march on this handle did not succeed, or none has run");
    return TSDF_HIP_E_INVALID;
  }
  if (!h->fl) h->fl = new tsdf_flatten_state();
  tsdf_flatten_state *st = *st_out = h->fl;
  st->valid = st->nm_valid = false;
  const uint64_t n = *n_out = h->mc_ntri, n_verts = 3 * n;
  if (const int rc = mp_check_counts(who, n, &n_verts)) return rc;
  if (!n) st->n_verts = st->n_faces = 0;
  return TSDF_HIP_OK;
}

int mp_idx_layout(tsdf_handle h, tsdf_flatten_state *st, uint64_t m, uint64_t kept, const char *who) {
  MpTake take;
  take((size_t)m * 12);  // the vertices, at 0
  st->o_faces = take((size_t)kept * 12), st->o_cell = take((size_t)kept * 8), st->o_rgb = take((size_t)m * 3);
  return st->out.reserve(take.o, h->stream, who);
}

int mp_idx_fill(tsdf_handle h, tsdf_flatten_state *st, uint64_t m, uint64_t kept, const uint32_t *d_faces, const uint8_t *d_keep,
                const uint32_t *d_offset) {
  char *o = (char *)st->out.p;
  const uint64_t n = h->mc_ntri;
  if (kept) {
    TSDF_HIP_TRY(hipMemcpyAsync(o + st->o_faces, d_faces, (size_t)kept * 12, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL((k_mp_compact<uint64_t, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->mc_cell.as<uint64_t>(), d_keep, d_offset, n,
                       (uint64_t *)(o + st->o_cell));
    TSDF_HIP_TRY(hipGetLastError());
  }
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  st->has_rgb = h->mc_has_rgb;
  st->n_verts = m, st->n_faces = kept;
  return TSDF_HIP_OK;
}

void mp_idx_set_host(tsdf_flatten_state *st, bool has_rgb, const uint64_t *cell, uint64_t n, uint64_t m, uint64_t kept, const uint8_t *keep) {
  st->h_verts.resize((size_t)m * 3);
  st->h_rgb.resize(has_rgb ? (size_t)m * 3 : 0);
  st->h_faces.resize((size_t)kept * 3);
  st->h_cell.clear();
  for (uint64_t f = 0; f < n; ++f)
    if (keep[f]) st->h_cell.push_back(cell[f]);
  st->has_rgb = has_rgb;
  st->n_verts = m, st->n_faces = kept;
}

int mp_idx_end(tsdf_flatten_state *st, uint64_t *n_verts, uint64_t *n_faces) {
  st->valid = true;
  if (n_verts) *n_verts = st->n_verts;
  if (n_faces) *n_faces = st->n_faces;
  return TSDF_HIP_OK;
}
