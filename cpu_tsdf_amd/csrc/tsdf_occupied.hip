// libtsdf_hip.so -- the observed surface band as a voxel list.
//
// Replaces TSDFVolumeOctree::getOccupiedVoxelIndices (src/lib/tsdf_volume_octree.cpp:590-609): the leaves with
// w > 0 && fabs(d) < 1, in the order OctreeNode::getLeaves walks them (src/lib/octree.cpp:99-109, children as split()
// makes them, :257-264) = Morton order with x as the high bit of every triple, the order tsdf_hip_march emits cells in.
//   k_occ_scan    ONE streaming pass over the distance plane of the box; the weight (any layout, through PlaneView) is read
//                 only for quads that hold an in-band distance; survivors become one 64-bit Morton key each
//   rocprim sort  of the keys over the bits a coordinate can set
//   k_occ_emit    key -> (x, y, z) and a gather of d / w / rgb into SoA outputs, run by the fetch calls
// HBM-bound streaming and a radix sort: no MFMA.
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "tsdf_common.h"
#include "tsdf_morton.h"

// ---- per-handle state (tsdf_hip_volume::occ) ------------------------------------------------------------------------------
// What a call leaves behind is the SORTED key list in a buffer of its own: the unsorted keys borrow tsdf_hip_march's cell
// buffer (mc_keys) and the sort's temporary storage the handle's scratch, both free again when tsdf_hip_occupied returns, so
// neither a download nor a march disturbs the result.
struct tsdf_occ_state {
  bool valid = false;      // a tsdf_hip_occupied has completed on this handle
  uint64_t n = 0;
  DevBuf keys;             // sorted Morton keys, one uint64_t each
  uint64_t d_bytes = 0;    // distance bytes the scan requested
  bool used_flags = false;
  EventSet<5> ev;                                                    // scan begin / end, sort end, emit begin / end
  float ms[3] = {0.f, 0.f, 0.f};                                     // scan, count read-back + sort, emit (of the fetches since)
  bool emit_pending = false;  // ev[3], ev[4] bracket an emit whose time has not been read yet
  // a multi-GPU set: the merged list (host) and where each entry came from (slab << 48 | index in the slab's list)
  std::vector<int32_t> m_idx;
  std::vector<uint64_t> m_src;
  std::vector<uint64_t> m_n;    // per slab: entries it contributed
  std::vector<uint8_t> m_used;  // per slab: the box touches it (else its own state is not ours)
};

static tsdf_occ_state *occ_state(tsdf_hip_volume *v) {  // created by the first tsdf_hip_occupied on the handle
  if (!v->occ) v->occ = new tsdf_occ_state();
  return v->occ;
}

void tsdf_occupied_release(tsdf_hip_volume *v) {
  if (!v->occ) return;
  TsdfDeviceScope scope(v->device);
  delete v->occ;
  v->occ = nullptr;
}

void tsdf_occupied_invalidate(tsdf_hip_volume *v) {
  if (v->occ) v->occ->valid = false;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
struct OccArgs {
  int x0, y0, z0, x1, y1, z1;  // the box [x0, x1) x [y0, y1) x [z0, z1), global voxel indices, inside the owned planes
  int xb, yb;                  // tile origin: x0 rounded down to a flag cell (64), y0 to a row group (4)
  int ny, z_first;
  int64_t pitch;
  const float *d;
  PlaneView pv;
  const uint8_t *band;         // the "band seen" flags, or NULL: read every quad
  int fx, fy;
};

#define OCC_ZB 8          // planes a block walks
#define OCC_BYTE_SLOTS 64  // counters[2 ..]: requested bytes, striped (one address for every block costs milliseconds)

// Which quads may the scan leave unread?  A voxel is listed iff w > 0 && |d| < 1.  While tsdf_hip_volume::band_exact holds,
// every distance of an owned plane is what the flag-keeping integrate kernels (k_integrate, k_integrate_p, k_integrate2)
// made of the reset value -1, and a flag of 0 says that no launch since the reset observed a voxel of that 64 x 4 x 1 cell
// with `act && !(raw > pos)` (any_div in tsdf_integrate.hip: each of those kernels sets the cell's flag in every branch that
// updates a distance with any_div true -- the fast ladder and the IEEE fallback alike -- and a wave only rests its distances
// when no lane has any_div).  So each voxel of such a cell is either never observed, d == -1, or was only ever observed beyond
// the positive truncation limit, every observation contributing dn = p = max_dist_pos / max_dist_neg (hpp:189-192).  With
// p >= 1 the running mean never leaves [1, inf): the first observation stores (-1 * 0 + p) / 1 = p, and from d >= 1, w >= 0
// every rounding step of (d * w + p) / (w + 1) is monotone -- fl(d * w) >= w, fl(fl(d * w) + p) >= fl(w + 1), and a correctly
// rounded quotient of x >= y > 0 is >= 1 (the kernels' scale-free divider is exact where its guard passes and IEEE elsewhere;
// a wave resting at the hinge keeps its bits).  Either way |d| >= 1: nothing of the cell is listed, and its quads are not read.
// With p < 1 (max_dist_pos < max_dist_neg) free space itself sits inside the band and the flags say nothing about |d| < 1: the
// host then passes band == NULL.  The plain kernels (RGB_NORMALIZED / LAB, the depth / variance weightings, TSDF_HIP_PLAIN_KERNEL)
// keep no flags and clear band_exact at launch, as do uploads, loads, plane copies and tsdf_hip_device_planes: every quad is read.
//
// A block is 4 waves; a wave owns 64 quads (four flag cells) of the four rows of one row group and walks OCC_ZB planes.  The
// survivors of a lane are 16 bits per plane (row r at bits 4r .. 4r + 3) kept in registers; when the walk is done the lanes'
// counts are scanned across the wave (one __ballot per bit of the count gives the lane rank), the four waves' totals meet in
// LDS, ONE atomic per block reserves the output range, and every lane writes its keys.
template <int WL>  // 0 = F32W (float plane), 1 = PACKED with colour (count in byte 3), 2 = PACKED count plane
static __global__ void __launch_bounds__(256)
k_occ_scan(const OccArgs a, uint64_t *__restrict__ keys, uint64_t capacity, unsigned long long *__restrict__ counters) {
  __shared__ unsigned s_cnt[4];
  __shared__ unsigned long long s_base, s_bytes;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0u) s_bytes = 0ull;
  __syncthreads();
  const int x4 = a.xb + (int)blockIdx.x * 256 + (int)lane * 4;
  const int yw = a.yb + ((int)blockIdx.y * 4 + (int)wave) * 4;
  const int zs = a.z0 + (int)blockIdx.z * OCC_ZB, ze = min(zs + OCC_ZB, a.z1);
  // voxels of this lane's 4 x 4 tile that lie in the box (a box may cut quads and row groups)
  unsigned tm = 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      tm |= (x4 + j >= a.x0 && x4 + j < a.x1 && yw + r >= a.y0 && yw + r < a.y1 ? 1u : 0u) << (4 * r + j);
  unsigned long long m_lo = 0ull, m_hi = 0ull;  // planes 0-3 / 4-7, 16 bits each
  unsigned rdb = 0u;
  if (tm) {
#pragma unroll
    for (int zi = 0; zi < OCC_ZB; ++zi) {
      const int z = zs + zi;
      if (z >= ze) break;  // (block-uniform)
      // (tm != 0: x4 < nx and a row of the group < ny, so the flag cell exists)
      if (a.band && !a.band[((int64_t)(z - a.z_first) * a.fy + (yw >> 2)) * a.fx + (x4 >> 6)]) continue;
      const int64_t base = ((int64_t)(z - a.z_first) * a.ny + yw) * a.pitch + x4;
      uint4 q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        q[r] = make_uint4(0x3f800000u, 0x3f800000u, 0x3f800000u, 0x3f800000u);  // 1.f: not inside the band
        if ((tm >> (4 * r)) & 15u) {  // pitch is a multiple of 4 and x4 < nx: the quad lies inside the row
          q[r] = *reinterpret_cast<const uint4 *>(a.d + base + (int64_t)r * a.pitch);
          rdb += 16u;
        }
      }
      unsigned dm = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // on the bit patterns: |d| < 1 <=> (bits & 0x7fffffff) < bits(1.f); a NaN compares as large and is not listed
        const unsigned u[4] = {q[r].x, q[r].y, q[r].z, q[r].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) dm |= ((u[j] & 0x7fffffffu) < 0x3f800000u ? 1u : 0u) << (4 * r + j);
      }
      dm &= tm;
      if (dm) {  // the weights, only of the quads that hold an in-band distance
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (!((dm >> (4 * r)) & 15u)) continue;
          const int64_t i = base + (int64_t)r * a.pitch;
          float w[4];
          if (WL == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.pv.w + i);
            w[0] = __uint_as_float(v.x), w[1] = __uint_as_float(v.y), w[2] = __uint_as_float(v.z), w[3] = __uint_as_float(v.w);
          } else if (WL == 1) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.pv.rgb + i);
            w[0] = tsdf_decode_w(v.x >> 24, a.pv.wmax), w[1] = tsdf_decode_w(v.y >> 24, a.pv.wmax);
            w[2] = tsdf_decode_w(v.z >> 24, a.pv.wmax), w[3] = tsdf_decode_w(v.w >> 24, a.pv.wmax);
          } else {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(a.pv.k8 + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = tsdf_decode_w((v >> (8 * j)) & 255u, a.pv.wmax);
          }
          unsigned wm = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) wm |= (w[j] > 0.f ? 1u : 0u) << j;
          dm &= ~(15u << (4 * r)) | (wm << (4 * r));
        }
      }
      if (zi < 4)
        m_lo |= (unsigned long long)dm << (16 * zi);
      else
        m_hi |= (unsigned long long)dm << (16 * (zi - 4));
    }
  }
  // lane rank: the count (0 .. 128) bit by bit, one 64-bit ballot each
  const unsigned cnt = (unsigned)__popcll(m_lo) + (unsigned)__popcll(m_hi);
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  unsigned rank = 0u, total = 0u;
  if (__ballot(cnt != 0u)) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned long long bk = __ballot((cnt >> k) & 1u);
      rank += (unsigned)__popcll(bk & lanes_below) << k;
      total += (unsigned)__popcll(bk) << k;
    }
  }
  unsigned long long b = rdb;
  if (__ballot(rdb != 0u)) {
    for (int o = 32; o; o >>= 1) b += __shfl_xor(b, o);
    if (lane == 0u) atomicAdd(&s_bytes, b);
  }
  if (lane == 0u) s_cnt[wave] = total;
  __syncthreads();
  if (tid == 0u) {
    const unsigned long long all = (unsigned long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    s_base = all ? atomicAdd(&counters[0], all) : 0ull;
    if (s_bytes) atomicAdd(&counters[2 + (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) % OCC_BYTE_SLOTS], s_bytes);
  }
  __syncthreads();
  if (!cnt) return;
  unsigned long long slot = s_base + rank;
  for (unsigned k = 0; k < wave; ++k) slot += s_cnt[k];
  // x4 and yw are multiples of 4: the two low bits of x and y are the voxel's place in the tile, no carry
  const uint64_t kxy = (tsdf_spread3((uint64_t)x4) << 2) | (tsdf_spread3((uint64_t)yw) << 1);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    unsigned long long m = half ? m_hi : m_lo;
    while (m) {
      const unsigned bit = (unsigned)__builtin_ctzll(m);
      m &= m - 1ull;
      const unsigned zi = (bit >> 4) + 4u * (unsigned)half, r = (bit >> 2) & 3u, j = bit & 3u;
      if (slot < capacity)
        keys[slot] = kxy | (tsdf_spread3((uint64_t)j) << 2) | (tsdf_spread3((uint64_t)r) << 1) | tsdf_spread3((uint64_t)(zs + (int)zi));
      ++slot;
    }
  }
}

struct OccEmitArgs {
  int ny, z_first;
  int64_t pitch;
  const float *d;
  PlaneView pv;
};

// Emit: one thread per listed voxel decodes its key and gathers; d / w / rgb words leave as one word per consecutive thread,
// the index triples and the 3-byte colours through LDS so that consecutive threads store consecutive words of the block's
// 3072 / 768 contiguous output bytes.  rgb32 (device callers): r | g << 8 | b << 16; rgb8 (host callers): r, g, b bytes,
// 4-byte aligned at the block's first voxel (the host stages chunks of a multiple of 256 voxels).
static __global__ void __launch_bounds__(256)
k_occ_emit(const OccEmitArgs a, const uint64_t *__restrict__ keys, uint64_t n, int32_t *__restrict__ idx, float *__restrict__ d,
           float *__restrict__ w, uint32_t *__restrict__ rgb32, uint8_t *__restrict__ rgb8) {
  __shared__ int32_t s_xyz[256 * 3];
  __shared__ uint32_t s_col[256];
  const uint64_t c0 = (uint64_t)blockIdx.x * 256u, i = c0 + threadIdx.x;
  if (i < n) {
    const uint64_t key = keys[i];
    const int x = (int)tsdf_compact3(key >> 2), y = (int)tsdf_compact3(key >> 1), z = (int)tsdf_compact3(key);
    const int64_t vi = tsdf_index(a.pitch, a.ny, a.z_first, x, y, z);
    s_xyz[3 * threadIdx.x] = x, s_xyz[3 * threadIdx.x + 1] = y, s_xyz[3 * threadIdx.x + 2] = z;
    if (d) d[i] = a.d[vi];
    if (w) w[i] = tsdf_load_w(a.pv, vi);
    const uint32_t col = (rgb32 || rgb8) && a.pv.rgb ? tsdf_load_rgb(a.pv, vi) : 0u;
    if (rgb32) rgb32[i] = col;
    s_col[threadIdx.x] = col;
  }
  __syncthreads();
  const unsigned m = (unsigned)min((uint64_t)256u, n - c0);  // (c0 < n by the grid's size)
  if (idx)
    for (unsigned j = threadIdx.x; j < 3u * m; j += 256u) idx[3ull * c0 + j] = s_xyz[j];
  if (rgb8) {
    auto byte_at = [&](unsigned b) -> uint32_t { return (s_col[b / 3u] >> (8u * (b % 3u))) & 255u; };
    const unsigned nb = 3u * m, words = nb >> 2;
    uint8_t *out = rgb8 + 3ull * c0;
    for (unsigned k = threadIdx.x; k < words; k += 256u)
      reinterpret_cast<uint32_t *>(out)[k] = byte_at(4u * k) | (byte_at(4u * k + 1u) << 8) | (byte_at(4u * k + 2u) << 16) | (byte_at(4u * k + 3u) << 24);
    if (threadIdx.x < (nb & 3u)) out[4u * words + threadIdx.x] = (uint8_t)byte_at(4u * words + threadIdx.x);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int occ_unsupported_rgb(tsdf_handle h) {
  if (!h->cn[0]) return TSDF_HIP_OK;
  tsdf_set_error("tsdf_hip_occupied_fetch: the exact colour bytes of an RGB_NORMALIZED / LAB volume come from the host's pow; "
                 "use tsdf_hip_lookup_rgb (or tsdf_hip_download) for them");
  return TSDF_HIP_E_UNSUPPORTED;
}

static int occ_nomem(uint64_t n, size_t bytes) {
  tsdf_set_error("tsdf_hip_occupied: the key buffers of " + std::to_string(n) + " listed voxels need " + std::to_string(bytes) +
                 " bytes of device memory, which are not available; extract a smaller box");
  (void)hipGetLastError();
  return TSDF_HIP_E_NOMEM;
}

// room for `bytes` in b; out of memory is this entry point's own message, about the n voxels and the `told` bytes
static int occ_reserve(tsdf_handle h, DevBuf &b, size_t bytes, uint64_t n, size_t told) {
  const int rc = b.reserve(bytes, h->stream, "tsdf_hip_occupied");
  return rc == TSDF_HIP_E_NOMEM ? occ_nomem(n, told) : rc;
}

static int occ_multi(tsdf_handle h, const int32_t box[6], uint64_t *n);
static int occ_multi_fetch(tsdf_handle h, int32_t *idx, float *d, float *w, uint8_t *rgb);

extern "C" int tsdf_hip_occupied(tsdf_handle h, const int32_t box[6], uint64_t *n) {
  if (!h) return TSDF_HIP_E_INVALID;
  if (n) *n = 0;
  if (h->multi) return occ_multi(h, box, n);
  TSDF_ENTER(h);
  tsdf_occ_state *st = occ_state(h);
  st->valid = false;
  st->n = 0;
  if (h->nx >= (1 << 21) || h->ny >= (1 << 21) || h->nz >= (1 << 21)) return TSDF_HIP_E_UNSUPPORTED;
  OccArgs a;
  if (box) {
    a.x0 = box[0], a.y0 = box[1], a.z0 = box[2];
    if (box[3] <= 0 || box[4] <= 0 || box[5] <= 0 || a.x0 < 0 || a.y0 < 0 || box[3] > h->nx - a.x0 || box[4] > h->ny - a.y0 ||
        a.z0 < h->z_begin || box[5] > h->z_end - a.z0) {
      tsdf_set_error("tsdf_hip_occupied: box outside the planes this handle owns");
      return TSDF_HIP_E_INVALID;
    }
    a.x1 = a.x0 + box[3], a.y1 = a.y0 + box[4], a.z1 = a.z0 + box[5];
  } else {
    a.x0 = a.y0 = 0, a.z0 = h->z_begin;
    a.x1 = h->nx, a.y1 = h->ny, a.z1 = h->z_end;
  }
  a.xb = a.x0 & ~63, a.yb = a.y0 & ~3;
  a.ny = h->ny, a.z_first = h->z_first, a.pitch = h->pitch;
  a.d = h->d;
  a.pv = tsdf_plane_view(h);
  // the flags decide only while they describe the planes AND free space rests outside the band (see k_occ_scan)
  const float hinge = h->p.max_dist_pos / h->p.max_dist_neg;  // pos_over_neg of the integrate launches
  const bool use_flags = h->band_exact && h->band && tsdf_tuning().mc_skip && h->p.max_dist_neg > 0.f && hinge >= 1.f;
  a.band = use_flags ? h->band : nullptr;
  a.fx = h->band_fx, a.fy = h->band_fy;
  const dim3 grid((unsigned)((a.x1 - a.xb + 255) / 256), (unsigned)((a.y1 - a.yb + 15) / 16), (unsigned)((a.z1 - a.z0 + OCC_ZB - 1) / OCC_ZB));
  if (grid.y > 65535u || grid.z > 65535u) return TSDF_HIP_E_UNSUPPORTED;
  if (const int rc = st->ev.ensure(5)) return rc;
  st->ms[0] = st->ms[1] = st->ms[2] = 0.f;
  st->emit_pending = false;
  unsigned long long counts[2 + OCC_BYTE_SLOTS] = {0};
  // pass 1 with the capacity at hand (tsdf_hip_march's cell buffer, shared); if the band turned out larger, grow and repeat
  for (int attempt = 0; attempt < 2; ++attempt) {
    const size_t cap = h->mc_keys.cap / sizeof(uint64_t);
    TSDF_HIP_TRY(hipMemsetAsync(h->counter, 0, sizeof counts, h->stream));
    TSDF_HIP_TRY(hipEventRecord(st->ev[0], h->stream));
    if (!h->packed)
      hipLaunchKernelGGL(k_occ_scan<0>, grid, dim3(256), 0, h->stream, a, h->mc_keys.as<uint64_t>(), (uint64_t)cap, h->counter);
    else if (h->rgb)
      hipLaunchKernelGGL(k_occ_scan<1>, grid, dim3(256), 0, h->stream, a, h->mc_keys.as<uint64_t>(), (uint64_t)cap, h->counter);
    else
      hipLaunchKernelGGL(k_occ_scan<2>, grid, dim3(256), 0, h->stream, a, h->mc_keys.as<uint64_t>(), (uint64_t)cap, h->counter);
    TSDF_HIP_TRY(hipGetLastError());
    TSDF_HIP_TRY(hipEventRecord(st->ev[1], h->stream));
    TSDF_HIP_TRY(hipMemcpyAsync(counts, h->counter, sizeof counts, hipMemcpyDeviceToHost, h->stream));
    TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
    if (counts[0] <= cap) break;
    if (attempt == 1) {  // (the planes changed between the two passes: not something a caller of one handle can do)
      tsdf_set_error("tsdf_hip_occupied: the volume changed during the call");
      return TSDF_HIP_E_INVALID;
    }
    const size_t need = (size_t)counts[0] + (size_t)counts[0] / 8 + 1024;
    if (const int rc = occ_reserve(h, h->mc_keys, need * sizeof(uint64_t), counts[0], need * sizeof(uint64_t) + (size_t)counts[0] * sizeof(uint64_t)))
      return rc;
  }
  const uint64_t count = counts[0];
  (void)hipEventElapsedTime(&st->ms[0], st->ev[0], st->ev[1]);  // the last (successful) scan
  st->d_bytes = 0;
  for (int i = 0; i < OCC_BYTE_SLOTS; ++i) st->d_bytes += counts[2 + i];
  st->used_flags = use_flags;
  if (count) {
    // sort by the Morton key -> the reference's leaf order; only the bits a coordinate can set take part
    int coord_bits = 1;
    while ((1 << coord_bits) < std::max(h->nx, std::max(h->ny, h->nz))) ++coord_bits;
    const unsigned key_bits = 3u * (unsigned)coord_bits;
    if (count * sizeof(uint64_t) > st->keys.cap) {
      const size_t cap = (size_t)count + (size_t)count / 8 + 1024;
      if (const int rc = occ_reserve(h, st->keys, cap * sizeof(uint64_t), count, cap * sizeof(uint64_t))) return rc;
    }
    uint64_t *const found = h->mc_keys.as<uint64_t>(), *const sorted = st->keys.as<uint64_t>();
    size_t tmp_bytes = 0;
    TSDF_HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, found, sorted, (size_t)count, 0u, key_bits, h->stream));
    if (const int rc = occ_reserve(h, h->scratch, tmp_bytes, count, tmp_bytes)) return rc;
    TSDF_HIP_TRY(rocprim::radix_sort_keys(h->scratch.p, tmp_bytes, found, sorted, (size_t)count, 0u, key_bits, h->stream));
    TSDF_HIP_TRY(hipEventRecord(st->ev[2], h->stream));
    TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipEventElapsedTime(&st->ms[1], st->ev[1], st->ev[2]);  // count read-back, buffer growth, sort
  }
  st->n = count;
  st->valid = true;
  if (n) *n = count;
  return TSDF_HIP_OK;
}

static OccEmitArgs occ_emit_args(tsdf_handle h) {
  OccEmitArgs e;
  e.ny = h->ny, e.z_first = h->z_first, e.pitch = h->pitch;
  e.d = h->d;
  e.pv = tsdf_plane_view(h);
  return e;
}

static void occ_collect_emit_time(tsdf_occ_state *st) {
  if (!st->emit_pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(st->ev[4]) == hipSuccess && hipEventElapsedTime(&ms, st->ev[3], st->ev[4]) == hipSuccess) st->ms[2] += ms;
  st->emit_pending = false;
}

extern "C" int tsdf_hip_occupied_fetch(tsdf_handle h, int32_t *idx, float *d, float *w, uint8_t *rgb) {
  if (!h) return TSDF_HIP_E_INVALID;
  if (h->multi) return occ_multi_fetch(h, idx, d, w, rgb);
  TSDF_ENTER(h);
  tsdf_occ_state *st = h->occ;
  if (!st || !st->valid) {
    tsdf_set_error("tsdf_hip_occupied_fetch: no tsdf_hip_occupied has completed on this handle");
    return TSDF_HIP_E_INVALID;
  }
  int rc = TSDF_HIP_OK;
  if (rgb && (rc = occ_unsupported_rgb(h))) return rc;
  if (!st->n || (!idx && !d && !w && !rgb)) return TSDF_HIP_OK;
  // staged through the handle's scratch in chunks of a multiple of 256 voxels (24 bytes per voxel at most)
  const size_t chunk = (size_t)std::min<uint64_t>(st->n, 4u << 20);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t b_idx = idx ? up(chunk * 12) : 0, b_d = d ? up(chunk * 4) : 0, b_w = w ? up(chunk * 4) : 0, b_rgb = rgb ? up(chunk * 3) : 0;
  if ((rc = tsdf_ensure_scratch(h, b_idx + b_d + b_w + b_rgb))) return rc;
  char *sp = (char *)h->scratch.p;
  int32_t *s_idx = idx ? (int32_t *)sp : nullptr;
  float *s_d = d ? (float *)(sp + b_idx) : nullptr;
  float *s_w = w ? (float *)(sp + b_idx + b_d) : nullptr;
  uint8_t *s_rgb = rgb ? (uint8_t *)(sp + b_idx + b_d + b_w) : nullptr;
  const OccEmitArgs e = occ_emit_args(h);
  for (uint64_t off = 0; off < st->n; off += chunk) {
    const uint64_t c = std::min<uint64_t>(chunk, st->n - off);
    occ_collect_emit_time(st);
    TSDF_HIP_TRY(hipEventRecord(st->ev[3], h->stream));
    hipLaunchKernelGGL(k_occ_emit, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, h->stream, e, st->keys.as<uint64_t>() + off, c, s_idx, s_d, s_w,
                       (uint32_t *)nullptr, s_rgb);
    TSDF_HIP_TRY(hipGetLastError());
    TSDF_HIP_TRY(hipEventRecord(st->ev[4], h->stream));
    st->emit_pending = true;
    if (idx && (rc = tsdf_to_host(h, idx + 3 * off, s_idx, (size_t)c * 12))) return rc;
    if (d && (rc = tsdf_to_host(h, d + off, s_d, (size_t)c * 4))) return rc;
    if (w && (rc = tsdf_to_host(h, w + off, s_w, (size_t)c * 4))) return rc;
    if (rgb && (rc = tsdf_to_host(h, rgb + 3 * off, s_rgb, (size_t)c * 3))) return rc;
  }
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  occ_collect_emit_time(st);
  return TSDF_HIP_OK;
}

// The same into DEVICE buffers of the caller, asynchronous on the handle's stream: the emit kernel writes them directly.
extern "C" int tsdf_hip_occupied_fetch_device(tsdf_handle h, int32_t *d_idx, float *d_d, float *d_w, uint32_t *d_rgb) {
  if (!h) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_occupied_fetch_device (the merged list of a multi-GPU set lives on the host)");
  TSDF_ENTER(h);
  tsdf_occ_state *st = h->occ;
  if (!st || !st->valid) {
    tsdf_set_error("tsdf_hip_occupied_fetch_device: no tsdf_hip_occupied has completed on this handle");
    return TSDF_HIP_E_INVALID;
  }
  if (d_rgb)
    if (const int rc = occ_unsupported_rgb(h)) return rc;
  if (!st->n || (!d_idx && !d_d && !d_w && !d_rgb)) return TSDF_HIP_OK;
  if (st->n > 0xffffffffull * 256ull) return TSDF_HIP_E_UNSUPPORTED;
  occ_collect_emit_time(st);
  TSDF_HIP_TRY(hipEventRecord(st->ev[3], h->stream));
  hipLaunchKernelGGL(k_occ_emit, dim3((unsigned)((st->n + 255) / 256)), dim3(256), 0, h->stream, occ_emit_args(h), st->keys.as<uint64_t>(), st->n, d_idx,
                     d_d, d_w, d_rgb, (uint8_t *)nullptr);
  TSDF_HIP_TRY(hipGetLastError());
  TSDF_HIP_TRY(hipEventRecord(st->ev[4], h->stream));
  st->emit_pending = true;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_occupied_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  out[0] = out[1] = out[2] = out[3] = 0;
  tsdf_occ_state *st = h->occ;
  if (!st || !st->valid) return TSDF_HIP_OK;
  if (h->multi) {  // sums over the slabs the box touched; "flags decided" only if they did on every one; the slowest slab's time
    out[2] = 1;
    for (size_t k = 0; k < st->m_n.size(); ++k) {
      const tsdf_occ_state *ss = tsdf_multi_slab(h, (int)k)->occ;
      if (!ss || !ss->valid || !st->m_used[k]) continue;  // (the box misses this slab)
      out[1] += ss->d_bytes;
      out[2] &= ss->used_flags ? 1u : 0u;
      out[3] = std::max<uint64_t>(out[3], (uint64_t)((ss->ms[0] + ss->ms[1]) * 1000.f));
    }
    out[0] = st->n;
    return TSDF_HIP_OK;
  }
  out[0] = st->n;
  out[1] = st->d_bytes;
  out[2] = st->used_flags ? 1u : 0u;
  out[3] = (uint64_t)((st->ms[0] + st->ms[1]) * 1000.f);
  return TSDF_HIP_OK;
}

// Report-only: device milliseconds by phase (HIP events on the handle's stream) -- ms[0] k_occ_scan of the last
// tsdf_hip_occupied, ms[1] its count read-back + sort, ms[2] k_occ_emit summed over the fetches since.
extern "C" int tsdf_hip_occupied_timing(tsdf_handle h, float ms[3]) {
  if (!h || !ms) return TSDF_HIP_E_INVALID;
  ms[0] = ms[1] = ms[2] = 0.f;
  if (h->multi) {  // the slowest slab, phase by phase
    tsdf_occ_state *st = h->occ;
    for (size_t k = 0; st && k < st->m_n.size(); ++k) {
      float m[3];
      if (!st->m_used[k] || tsdf_hip_occupied_timing(tsdf_multi_slab(h, (int)k), m)) continue;
      for (int i = 0; i < 3; ++i) ms[i] = std::max(ms[i], m[i]);
    }
    return TSDF_HIP_OK;
  }
  tsdf_occ_state *st = h->occ;
  if (!st || !st->valid) return TSDF_HIP_OK;
  TSDF_ON_DEVICE(h->device);
  occ_collect_emit_time(st);
  for (int i = 0; i < 3; ++i) ms[i] = st->ms[i];
  return TSDF_HIP_OK;
}

// ---- multi-GPU set ---------------------------------------------------------------------------------------------------------
// Every slab scans the part of the box it owns, on its own stream, from a host thread of its own (as tsdf_multi_march runs
// the slabs' meshes); the sorted slab lists are merged by key on the host.  z is the LOW bit of every key triple, so the
// slabs interleave: runs are taken from the slab with the smallest key up to the smallest key of the others.
static inline uint64_t occ_key_host(const int32_t *p) { return tsdf_morton_key((uint64_t)p[0], (uint64_t)p[1], (uint64_t)p[2]); }

static int occ_multi(tsdf_handle h, const int32_t box[6], uint64_t *n_out) {
  if (const int rc = tsdf_multi_flush(h)) return rc;  // (frame pairing: slabs launch what they hold first)
  const int n = tsdf_hip_slab_count(h);
  tsdf_occ_state *st = occ_state(h);
  st->valid = false;
  st->n = 0;
  int32_t b[6] = {0, 0, 0, h->nx, h->ny, h->nz};
  if (box) {
    memcpy(b, box, sizeof b);
    if (b[3] <= 0 || b[4] <= 0 || b[5] <= 0 || b[0] < 0 || b[1] < 0 || b[2] < 0 || b[3] > h->nx - b[0] || b[4] > h->ny - b[1] ||
        b[5] > h->nz - b[2]) {
      tsdf_set_error("tsdf_hip_occupied: box outside the grid");
      return TSDF_HIP_E_INVALID;
    }
  }
  struct Part {
    std::vector<int32_t> idx;
    uint64_t n = 0;
    bool used = false;
    int rc = 0;
    std::string err;
  };
  std::vector<Part> part(n);
  std::vector<std::thread> th;
  for (int k = 0; k < n; ++k) {
    tsdf_handle s = tsdf_multi_slab(h, k);
    const int z0 = std::max(b[2], s->z_begin), z1 = std::min(b[2] + b[5], s->z_end);
    if (z1 <= z0) continue;
    part[k].used = true;
    th.emplace_back([&part, s, k, z0, z1, b]() {
      Part &p = part[k];
      const int32_t sb[6] = {b[0], b[1], z0, b[3], b[4], z1 - z0};
      p.rc = tsdf_hip_occupied(s, sb, &p.n);
      if (!p.rc && p.n) {
        p.idx.resize(p.n * 3);
        p.rc = tsdf_hip_occupied_fetch(s, p.idx.data(), nullptr, nullptr, nullptr);
      }
      if (p.rc) p.err = tsdf_hip_last_error();
    });
  }
  for (auto &t : th) t.join();
  uint64_t total = 0;
  st->m_n.assign(n, 0);
  st->m_used.assign(n, 0);
  for (int k = 0; k < n; ++k) {
    if (part[k].rc) {
      tsdf_set_error(part[k].err);
      return part[k].rc;
    }
    total += part[k].n;
    st->m_n[k] = part[k].n;
    st->m_used[k] = part[k].used ? 1 : 0;
  }
  st->m_idx.resize(total * 3);
  st->m_src.resize(total);
  std::vector<uint64_t> pos(n, 0), key(n, ~0ull);
  for (int k = 0; k < n; ++k)
    if (part[k].n) key[k] = occ_key_host(&part[k].idx[0]);
  for (uint64_t t = 0; t < total;) {
    int best = 0;
    for (int k = 1; k < n; ++k)
      if (key[k] < key[best]) best = k;
    uint64_t limit = ~0ull;
    for (int k = 0; k < n; ++k)
      if (k != best) limit = std::min(limit, key[k]);
    Part &p = part[best];
    uint64_t i = pos[best], j = i;
    while (j < p.n && occ_key_host(&p.idx[3 * j]) < limit) ++j;
    if (j == i) j = i + 1;  // (cannot happen: a voxel belongs to one slab)
    memcpy(&st->m_idx[3 * t], &p.idx[3 * i], (size_t)(j - i) * 12);
    for (uint64_t q = i; q < j; ++q) st->m_src[t + (q - i)] = ((uint64_t)best << 48) | q;
    t += j - i;
    pos[best] = j;
    key[best] = j < p.n ? occ_key_host(&p.idx[3 * j]) : ~0ull;
  }
  st->n = total;
  st->valid = true;
  if (n_out) *n_out = total;
  return TSDF_HIP_OK;
}

static int occ_multi_fetch(tsdf_handle h, int32_t *idx, float *d, float *w, uint8_t *rgb) {
  tsdf_occ_state *st = h->occ;
  if (!st || !st->valid) {
    tsdf_set_error("tsdf_hip_occupied_fetch: no tsdf_hip_occupied has completed on this handle");
    return TSDF_HIP_E_INVALID;
  }
  if (rgb)
    if (const int rc = occ_unsupported_rgb(tsdf_multi_first(h))) return rc;
  if (!st->n) return TSDF_HIP_OK;
  if (idx) memcpy(idx, st->m_idx.data(), (size_t)st->n * 12);
  if (!d && !w && !rgb) return TSDF_HIP_OK;
  const int n = (int)st->m_n.size();
  struct Part {
    std::vector<float> d, w;
    std::vector<uint8_t> rgb;
    int rc = 0;
    std::string err;
  };
  std::vector<Part> part(n);
  std::vector<std::thread> th;
  for (int k = 0; k < n; ++k) {
    const uint64_t nk = st->m_n[k];
    if (!nk) continue;
    th.emplace_back([&part, h, k, nk, d, w, rgb]() {
      Part &p = part[k];
      if (d) p.d.resize(nk);
      if (w) p.w.resize(nk);
      if (rgb) p.rgb.resize(nk * 3);
      p.rc = tsdf_hip_occupied_fetch(tsdf_multi_slab(h, k), nullptr, d ? p.d.data() : nullptr, w ? p.w.data() : nullptr,
                                     rgb ? p.rgb.data() : nullptr);
      if (p.rc) p.err = tsdf_hip_last_error();
    });
  }
  for (auto &t : th) t.join();
  for (int k = 0; k < n; ++k)
    if (part[k].rc) {
      tsdf_set_error(part[k].err);
      return part[k].rc;
    }
  for (uint64_t t = 0; t < st->n; ++t) {
    const Part &p = part[st->m_src[t] >> 48];
    const uint64_t i = st->m_src[t] & 0xffffffffffffull;
    if (d) d[t] = p.d[i];
    if (w) w[t] = p.w[i];
    if (rgb) memcpy(rgb + 3 * t, &p.rgb[3 * i], 3);
  }
  return TSDF_HIP_OK;
}
