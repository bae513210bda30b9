// libtsdf_hip.so -- computeDistanceField: the exact Euclidean distance transform of the volume's zero crossing
// (tsdf_hip_esdf; NOT in the reference, whose volumes only know the truncated distance).  The rule is in include/tsdf_hip.h.
//
// A separable exact transform in integer arithmetic, three streaming passes over a box of B voxels:
//   k_esdf_scan_x   one block per x row of the box, one lane per voxel, the block looping over segments of 256 voxels.
//                   Each lane classifies its own voxel (0 not valid, 1 valid and >= 0, 2 valid and negative: d and the weight
//                   through tsdf_load_w, any layout) and its +-y and +-z neighbours the same way; +-x come from the
//                   neighbouring lanes (a shuffle), the first and last lane of a wave read a one-voxel apron.  The site bit
//                   and the sign bit leave the wave as one 64-bit ballot each: the site words stay in LDS for the whole row,
//                   the sign words go to the sign plane (1 bit per voxel: the sign of the volume AT COMPUTE TIME, which the
//                   fetches need later).  Then every word looks up the last site before it and the first site after it (the
//                   carry across waves and segments, in LDS), and every lane takes the nearest site of its own word with a
//                   count-leading / count-trailing-zeros on the masked ballot: d2 = dx^2 in the row, or FAR.
//                   The "band seen" flags are NOT used to skip cells: a negative site's positive neighbour can be a
//                   never-in-band free-space voxel (d == 1) in a cell whose flag is 0, so the flags cannot decide a site.
//   k_esdf_axis<1>  y, then
//   k_esdf_axis<2>  z: one lane per line, lanes along x (every access to the field is coalesced), each lane sequential along
//                   its line: Meijster's lower envelope with the integer Sep (64-bit numerator, integer division; no float
//                   enters d2).  FAR entries are skipped, not pushed.  The envelope (g, s | t << 16: 8 bytes per parabola)
//                   lives in device scratch laid out [depth][line], so lanes at the same depth touch adjacent words; its
//                   top is kept in registers.  In place: a lane has read its whole line before it writes the first result.
//                   With r_max > 0 every pass writes FAR for d2 > r_max^2 at once: a final d2 <= r_max^2 bounds each of its
//                   per-axis terms by r_max^2, so nothing that survives ever looks at a truncated entry's value.
//   k_esdf_dist     (the fetches and tsdf_hip_esdf_sample) dist = sgn * voxel * sqrtf((float)d2) from d2 and the sign plane.
// Where the float is made: at the fetch.  Writing dist at the end of pass z would add 4 bytes written per voxel to every
// compute and 4 bytes held per voxel for good, whether or not anyone asks for floats (tsdf_hip_esdf_sample reads one word of
// d2 and one of the sign plane per point either way); made at the fetch it costs 4 1/8 bytes read per voxel FETCHED.
// Bytes per voxel of the box that the three passes move, by this file's own count:
//   pass x   reads d (4) and the weight (4 F32W, 4 PACKED with colour, 1 PACKED without) once -- the +-y / +-z rows are the
//            neighbouring blocks' own rows and are counted as cache hits --, writes d2 (4) and the sign bit (1/8)
//   pass y/z read 4, write 4, plus 8 written and 8 read per parabola that enters the envelope (at most one per voxel; counted
//            as 0, so the figure is a lower bound)
// -- 24 1/8 + the weight's bytes in all, which is the count tools/time_esdf.py divides by the measured time.
// No roofline claim until tools/time_esdf.py has run: the passes along y and z are sequential per lane and latency-bound.
// Compiled with -ffp-contract=off; no floating-point atomics: the only atomic is the 64-bit site count, one per block.
#include <math.h>

#include <algorithm>
#include <string>

#include "tsdf_common.h"
#include "tsdf_gridview.h"

#define ESDF_FAR TSDF_HIP_ESDF_FAR
#define ESDF_MAX_EXTENT 16384                 // per axis of the box: s and t of a parabola share a word, a row's site words fit LDS
#define ESDF_ROW_WORDS (ESDF_MAX_EXTENT / 64)
#define ESDF_STACK_CAP ((size_t)1 << 30)      // bytes of envelope scratch one launch of k_esdf_axis may use (lines are batched)

struct tsdf_esdf_state {
  bool valid = false;        // a tsdf_hip_esdf has completed on this handle and no tsdf_hip_shift has moved the indices since
  int box[6] = {0, 0, 0, 0, 0, 0};  // x0, y0, z0, nx, ny, nz
  int words = 0;             // 64-bit sign words per row
  DevBuf d2;                 // uint32_t [nz][ny][nx]
  DevBuf sign;               // uint64_t [nz][ny][words]: bit x & 63 of word x >> 6 = neg(v) at compute time
  DevBuf stack;              // uint2: the envelopes of one batch of lines
  DevBuf count;              // one unsigned long long: sites
  uint64_t sites = 0;
  EventSet<2> ev;
  float ms = 0.f;
};

void tsdf_esdf_release(tsdf_hip_volume *v) {
  if (!v->esdf) return;
  TsdfDeviceScope scope(v->device);
  delete v->esdf;
  v->esdf = nullptr;
}

void tsdf_esdf_invalidate(tsdf_hip_volume *v) {
  if (v->esdf) v->esdf->valid = false;
}

// tsdf_hip_reset: the field is dropped, memory included (the stream has been synchronised)
void tsdf_esdf_drop(tsdf_hip_volume *v) {
  if (!v->esdf) return;
  v->esdf->d2.release(), v->esdf->sign.release(), v->esdf->stack.release();
  v->esdf->valid = false;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
struct EsdfArgs {
  int x0, y0, z0, bx, by, bz;  // the box
  int nx, ny, nz;              // the grid (a whole-grid handle: plane index == z)
  int64_t pitch;
  const float *d;
  PlaneView pv;
  float min_weight;
  uint32_t r2;                 // r_max^2, 0 = unlimited
  int r;                       // r_max
  int words;
};

// 0 not valid, 1 valid and not negative, 2 valid and negative (-0.0 < 0 is false: not negative)
static __device__ __forceinline__ unsigned esdf_class(const EsdfArgs &a, int64_t i) {
  const float d = a.d[i];
  const float w = tsdf_load_w(a.pv, i);
  const bool valid = w > a.min_weight && d == d;
  return valid ? (d < 0.f ? 2u : 1u) : 0u;
}

static __global__ void __launch_bounds__(256)
k_esdf_scan_x(const EsdfArgs a, uint32_t *__restrict__ d2, uint64_t *__restrict__ sign, unsigned long long *__restrict__ n_sites) {
  __shared__ unsigned long long s_site[ESDF_ROW_WORDS];
  __shared__ int s_prev[ESDF_ROW_WORDS], s_next[ESDF_ROW_WORDS];  // last site in the words before / first site in the words after, box x
  __shared__ unsigned s_cnt[4];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int yl = (int)blockIdx.x, zl = (int)blockIdx.y;
  const int y = a.y0 + yl, z = a.z0 + zl;
  const int64_t row = ((int64_t)z * a.ny + y) * a.pitch;
  const int64_t sy = a.pitch, sz = (int64_t)a.ny * a.pitch;
  const int64_t out_row = (int64_t)zl * a.by + yl;
  unsigned sites = 0u;
  for (int seg = 0; seg < a.bx; seg += 256) {  // (block-uniform trip count)
    const int xl = seg + (int)tid, x = a.x0 + xl;
    const bool in_grid = x < a.nx, in_box = xl < a.bx;
    unsigned c = 0u;
    bool cross = false;
    if (in_grid) {
      const int64_t i = row + x;
      c = esdf_class(a, i);
      if (c && in_box) {  // a neighbour inside the GRID that is valid and of the other sign
        unsigned n;
        if (y > 0 && (n = esdf_class(a, i - sy)) != 0u && n != c) cross = true;
        if (y + 1 < a.ny && (n = esdf_class(a, i + sy)) != 0u && n != c) cross = true;
        if (z > 0 && (n = esdf_class(a, i - sz)) != 0u && n != c) cross = true;
        if (z + 1 < a.nz && (n = esdf_class(a, i + sz)) != 0u && n != c) cross = true;
      }
    }
    // +-x: the neighbouring lanes; the wave's first and last lane read the apron voxel (a lane past the grid's end has c == 0)
    unsigned cl = __shfl_up(c, 1), cr = __shfl_down(c, 1);
    if (lane == 0u) cl = (in_grid && x > 0) ? esdf_class(a, row + x - 1) : 0u;
    if (lane == 63u) cr = (x + 1 < a.nx) ? esdf_class(a, row + x + 1) : 0u;
    if (c && in_box && ((cl != 0u && cl != c) || (cr != 0u && cr != c))) cross = true;
    const bool site = in_box && c != 0u && cross;
    const unsigned long long m_site = __ballot(site), m_neg = __ballot(in_box && c == 2u);
    const int word = (seg >> 6) + (int)wave;
    if (lane == 0u && word < a.words) {
      s_site[word] = m_site;
      sign[out_row * a.words + word] = m_neg;
      sites += (unsigned)__popcll(m_site);
    }
  }
  if (lane == 0u) s_cnt[wave] = sites;
  __syncthreads();
  if (tid == 0u) {
    const unsigned n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (n) atomicAdd(n_sites, (unsigned long long)n);
  }
  // the carry across words: for word j, the last site before it and the first site after it (each thread walks until it
  // meets a word that holds a site)
  for (int j = (int)tid; j < a.words; j += 256) {
    int p = -1, q = -1;
    for (int k = j - 1; k >= 0; --k) {
      const unsigned long long m = s_site[k];
      if (m) {
        p = k * 64 + 63 - __clzll((long long)m);
        break;
      }
    }
    for (int k = j + 1; k < a.words; ++k) {
      const unsigned long long m = s_site[k];
      if (m) {
        q = k * 64 + (int)__builtin_ctzll(m);
        break;
      }
    }
    s_prev[j] = p;
    s_next[j] = q;
  }
  __syncthreads();
  for (int seg = 0; seg < a.bx; seg += 256) {
    const int xl = seg + (int)tid;
    if (xl >= a.bx) break;
    const int word = xl >> 6, bit = xl & 63;
    const unsigned long long m = s_site[word];
    const unsigned long long lo = m & (~0ull >> (63 - bit)), hi = m & (~0ull << bit);  // sites at or before / at or after this voxel
    const int p = lo ? word * 64 + 63 - __clzll((long long)lo) : s_prev[word];
    const int q = hi ? word * 64 + (int)__builtin_ctzll(hi) : s_next[word];
    int dx = -1;
    if (p >= 0) dx = xl - p;
    if (q >= 0 && (dx < 0 || q - xl < dx)) dx = q - xl;
    uint32_t v = ESDF_FAR;
    if (dx >= 0 && !(a.r2 && dx > a.r)) v = (uint32_t)dx * (uint32_t)dx;
    d2[out_row * a.bx + xl] = v;
  }
}

// Lines of one batch: AXIS 1 (y): line = (z, x), z in [o0, o0 + no); AXIS 2 (z): line = (y, x), y in [o0, o0 + no).
// Consecutive lanes take consecutive x of one outer index and then the next, so the field words a wave touches at one step are
// contiguous within a row (AXIS 2: across rows as well).
template <int AXIS>
static __global__ void __launch_bounds__(256)
k_esdf_axis(uint32_t *__restrict__ fld, uint2 *__restrict__ stack, const int bx, const int by, const int bz, const int o0, const int no,
            const uint32_t r2) {
  const int64_t lines = (int64_t)no * bx;
  const int64_t lid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (lid >= lines) return;
  const int n = AXIS == 1 ? by : bz;
  const int64_t stride = AXIS == 1 ? (int64_t)bx : (int64_t)bx * by;
  const int64_t base = AXIS == 1 ? ((int64_t)(o0 + lid / bx) * by) * bx + lid % bx : (int64_t)o0 * bx + lid;
  uint2 *__restrict__ st = stack + lid;  // entry k of this line: st[k * lines]
  // f(x; s, g) = (x - s)^2 + g; the top of the envelope in registers: parabola (ts, tg), lowest from tt on
  int q = -1;
  uint32_t ts = 0u, tg = 0u, tt = 0u;
  for (int u = 0; u < n; ++u) {
    const uint32_t g = fld[base + (int64_t)u * stride];
    if (g == ESDF_FAR) continue;
    while (q >= 0) {
      const uint32_t e = tt - ts, f = (uint32_t)u - tt;  // (either may wrap: the square is right modulo 2^32, and every f(x) < 2^32)
      if (e * e + tg <= f * f + g) break;                  // the top still wins at its own start: it stays
      if (--q >= 0) {
        const uint2 t = st[(int64_t)q * lines];
        tg = t.x, ts = t.y & 0xffffu, tt = t.y >> 16;
      }
    }
    if (q < 0) {
      q = 0, ts = (uint32_t)u, tg = g, tt = 0u;
      st[0] = make_uint2(tg, ts);
    } else {
      // Sep(ts, u) = floor((u^2 - ts^2 + g - tg) / (2 (u - ts))): the last x where the top is not above the new parabola.  The
      // numerator is >= 0 here (the top wins at tt >= 0, so tt <= Sep) and < 2^32 for every extent this file accepts.
      const int64_t num = (int64_t)u * u - (int64_t)ts * ts + (int64_t)g - (int64_t)tg;
      const uint32_t den = 2u * ((uint32_t)u - ts);
      const uint64_t sep = ((uint64_t)num >> 32) ? (uint64_t)num / den : (uint64_t)((uint32_t)num / den);
      if (sep + 1u < (uint64_t)n) {
        ++q, ts = (uint32_t)u, tg = g, tt = (uint32_t)sep + 1u;
        st[(int64_t)q * lines] = make_uint2(tg, ts | (tt << 16));
      }
    }
  }
  for (int u = n - 1; u >= 0; --u) {
    uint32_t v = ESDF_FAR;
    if (q >= 0) {
      const uint32_t e = (uint32_t)u > ts ? (uint32_t)u - ts : ts - (uint32_t)u;
      v = e * e + tg;
      if (r2 && v > r2) v = ESDF_FAR;
      if ((uint32_t)u == tt && --q >= 0) {
        const uint2 t = st[(int64_t)q * lines];
        tg = t.x, ts = t.y & 0xffffu, tt = t.y >> 16;
      }
    }
    fld[base + (int64_t)u * stride] = v;
  }
}

// dist = sgn * voxel * sqrtf((float)d2), FAR -> sgn * inf; sqrtf is the correctly rounded one (no fast-math in this build)
static __device__ __forceinline__ float esdf_dist(uint32_t v, bool neg, float voxel) {
  const float m = v == ESDF_FAR ? INFINITY : sqrtf((float)v) * voxel;
  return neg ? -m : m;
}

static __global__ void __launch_bounds__(256)
k_esdf_dist(const uint32_t *__restrict__ d2, const uint64_t *__restrict__ sign, int bx, int words, int64_t first, int64_t n, float voxel,
            float *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int64_t i = first + t, row = i / bx;
  const int xl = (int)(i - row * bx);
  const bool neg = (sign[row * words + (xl >> 6)] >> (xl & 63)) & 1ull;
  out[t] = esdf_dist(d2[i], neg, voxel);
}

static __global__ void __launch_bounds__(256)
k_esdf_sample(const GridView g, const uint32_t *__restrict__ d2, const uint64_t *__restrict__ sign, int x0, int y0, int z0, int bx, int by,
              int bz, int words, float voxel, const float *__restrict__ xyz, size_t n, float *__restrict__ dist,
              unsigned char *__restrict__ found) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  int64_t vi;
  bool local;
  int k;
  bool hit = containing(g, xyz[3 * t], xyz[3 * t + 1], xyz[3 * t + 2], vi, local, k);
  float v = NAN;
  if (hit) {  // (a whole-grid handle: vi = (k * ny + j) * pitch + i)
    const int i = (int)(vi % g.pitch) - x0, j = (int)((vi / g.pitch) % g.ny) - y0, kk = k - z0;
    hit = i >= 0 && i < bx && j >= 0 && j < by && kk >= 0 && kk < bz;
    if (hit) {
      const int64_t row = (int64_t)kk * by + j;
      const bool neg = (sign[row * words + (i >> 6)] >> (i & 63)) & 1ull;
      v = esdf_dist(d2[row * bx + i], neg, voxel);
    }
  }
  dist[t] = v;
  found[t] = hit ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static const char *esdf_refusal(const tsdf_hip_volume *h) {
  if (h->multi) return "tsdf_hip_esdf works on ONE handle; a multi-GPU set (tsdf_hip_create_multi) is not supported";
  if (h->z_first != 0 || h->nz_alloc != h->nz || h->z_begin != 0 || h->z_end != h->nz)
    return "tsdf_hip_esdf: a handle that owns part of its grid (z_begin / z_end) is not supported: distances cross slab borders";
  const tsdf_params &p = h->p;
  if (p.res[0] != p.res[1] || p.res[0] != p.res[2] || p.size[0] != p.size[1] || p.size[0] != p.size[2])
    return "tsdf_hip_esdf needs cubic voxels on a cubic grid (res and size equal on all axes): one voxel edge scales the distances";
  return nullptr;
}

static int esdf_nomem(size_t bytes) {
  tsdf_set_error("tsdf_hip_esdf: the field and its scratch need " + std::to_string(bytes) +
                 " bytes of device memory, which are not available; compute a smaller box");
  (void)hipGetLastError();
  return TSDF_HIP_E_NOMEM;
}

extern "C" int tsdf_hip_esdf(tsdf_handle h, const int32_t box[6], int32_t r_max, float min_weight, uint64_t *n_sites) {
  if (!h) return TSDF_HIP_E_INVALID;
  if (r_max < 0) {
    tsdf_set_error("tsdf_hip_esdf: r_max < 0");
    return TSDF_HIP_E_INVALID;
  }
  if (!(min_weight >= 0.f)) {
    tsdf_set_error("tsdf_hip_esdf: min_weight negative or NaN");
    return TSDF_HIP_E_INVALID;
  }
  if (const char *why = esdf_refusal(h)) {
    tsdf_set_error(why);
    return TSDF_HIP_E_UNSUPPORTED;
  }
  int b[6] = {0, 0, 0, h->nx, h->ny, h->nz};
  if (box) {
    for (int i = 0; i < 6; ++i) b[i] = box[i];
    if (b[3] <= 0 || b[4] <= 0 || b[5] <= 0 || b[0] < 0 || b[1] < 0 || b[2] < 0 || b[3] > h->nx - b[0] || b[4] > h->ny - b[1] ||
        b[5] > h->nz - b[2]) {
      tsdf_set_error("tsdf_hip_esdf: box outside the grid, or with an extent that is not positive");
      return TSDF_HIP_E_INVALID;
    }
  }
  if (b[3] > ESDF_MAX_EXTENT || b[4] > ESDF_MAX_EXTENT || b[5] > ESDF_MAX_EXTENT) {
    tsdf_set_error("tsdf_hip_esdf: a box of more than " + std::to_string(ESDF_MAX_EXTENT) + " voxels along an axis is not supported");
    return TSDF_HIP_E_UNSUPPORTED;
  }
  TSDF_ENTER(h);
  if (!h->esdf) h->esdf = new tsdf_esdf_state();
  tsdf_esdf_state *st = h->esdf;
  st->valid = false;  // the next tsdf_hip_esdf drops the field, whether or not it succeeds
  const int bx = b[3], by = b[4], bz = b[5];
  const size_t nvox = (size_t)bx * by * bz, rows = (size_t)by * bz;
  const int words = (bx + 63) / 64;
  // the envelopes of a batch of lines: whole outer indices (planes for y, rows for z), as many as the cap allows
  const size_t depth = (size_t)std::max(by, bz);
  const size_t per_outer = (size_t)bx * depth * sizeof(uint2);
  const size_t outer_max = (size_t)std::max(by, bz);
  const size_t batch = std::max<size_t>(1, std::min(outer_max, ESDF_STACK_CAP / per_outer));
  const size_t stack_entries = batch * bx * depth;
  // (a fetch_device may still be reading the buffers that are about to grow: reserve waits for the stream first)
  const size_t b_d2 = nvox * 4, b_sign = rows * words * 8, b_stack = stack_entries * sizeof(uint2);
  auto room = [&](DevBuf &buf, size_t bytes) {
    const int rc = buf.reserve(bytes, h->stream, "tsdf_hip_esdf");
    return rc == TSDF_HIP_E_NOMEM ? esdf_nomem(b_d2 + b_sign + b_stack) : rc;
  };
  if (const int rc = room(st->d2, b_d2)) return rc;
  if (const int rc = room(st->sign, b_sign)) return rc;
  if (const int rc = room(st->stack, b_stack)) return rc;
  if (const int rc = st->count.reserve(sizeof(unsigned long long), h->stream)) return rc;
  if (const int rc = st->ev.ensure(2)) return rc;
  uint32_t *const d2 = st->d2.as<uint32_t>();
  EsdfArgs a;
  a.x0 = b[0], a.y0 = b[1], a.z0 = b[2], a.bx = bx, a.by = by, a.bz = bz;
  a.nx = h->nx, a.ny = h->ny, a.nz = h->nz;
  a.pitch = h->pitch;
  a.d = h->d;
  a.pv = tsdf_plane_view(h);
  a.min_weight = min_weight;
  // (a box diagonal is below 2^15 voxels: a larger radius truncates nothing)
  a.r = r_max > 32767 ? 0 : r_max;
  a.r2 = (uint32_t)a.r * (uint32_t)a.r;
  a.words = words;
  TSDF_HIP_TRY(hipMemsetAsync(st->count.p, 0, sizeof(unsigned long long), h->stream));
  TSDF_HIP_TRY(hipEventRecord(st->ev[0], h->stream));
  hipLaunchKernelGGL(k_esdf_scan_x, dim3((unsigned)by, (unsigned)bz), dim3(256), 0, h->stream, a, d2, st->sign.as<uint64_t>(),
                     st->count.as<unsigned long long>());
  TSDF_HIP_TRY(hipGetLastError());
  for (int axis = 1; axis <= 2; ++axis) {
    const int outer = axis == 1 ? bz : by, n = axis == 1 ? by : bz;
    if (n == 1) continue;  // (a line of one voxel is its own transform)
    for (int o0 = 0; o0 < outer; o0 += (int)batch) {
      const int no = std::min((int)batch, outer - o0);
      const unsigned blocks = (unsigned)(((int64_t)no * bx + 255) / 256);
      if (axis == 1)
        hipLaunchKernelGGL(k_esdf_axis<1>, dim3(blocks), dim3(256), 0, h->stream, d2, st->stack.as<uint2>(), bx, by, bz, o0, no, a.r2);
      else
        hipLaunchKernelGGL(k_esdf_axis<2>, dim3(blocks), dim3(256), 0, h->stream, d2, st->stack.as<uint2>(), bx, by, bz, o0, no, a.r2);
      TSDF_HIP_TRY(hipGetLastError());
    }
  }
  TSDF_HIP_TRY(hipEventRecord(st->ev[1], h->stream));
  unsigned long long n = 0;
  TSDF_HIP_TRY(hipMemcpyAsync(&n, st->count.p, sizeof n, hipMemcpyDeviceToHost, h->stream));
  TSDF_HIP_TRY(hipStreamSynchronize(h->stream));
  st->ms = 0.f;
  (void)hipEventElapsedTime(&st->ms, st->ev[0], st->ev[1]);
  st->sites = n;
  for (int i = 0; i < 6; ++i) st->box[i] = b[i];
  st->words = words;
  st->valid = true;
  if (n_sites) *n_sites = n;
  return TSDF_HIP_OK;
}

static tsdf_esdf_state *esdf_ready(tsdf_handle h, const char *who) {
  tsdf_esdf_state *st = h->esdf;
  if (st && st->valid) return st;
  tsdf_set_error(std::string(who) + ": no distance field on this handle (none computed, or dropped by tsdf_hip_reset, or the indices moved in tsdf_hip_shift)");
  return nullptr;
}

extern "C" int tsdf_hip_esdf_fetch(tsdf_handle h, uint32_t *d2, float *dist) {
  if (!h) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_esdf_fetch");
  TSDF_ENTER(h);
  tsdf_esdf_state *st = esdf_ready(h, "tsdf_hip_esdf_fetch");
  if (!st) return TSDF_HIP_E_INVALID;
  const int64_t nvox = (int64_t)st->box[3] * st->box[4] * st->box[5];
  int rc = TSDF_HIP_OK;
  if (d2 && (rc = tsdf_to_host(h, d2, st->d2.p, (size_t)nvox * 4))) return rc;
  if (!dist) return TSDF_HIP_OK;
  const int64_t chunk = std::min<int64_t>(nvox, 16 << 20);  // staged through the handle's scratch
  if ((rc = tsdf_ensure_scratch(h, (size_t)chunk * 4))) return rc;
  const float voxel = tsdf_voxel_edge(h->p);
  for (int64_t off = 0; off < nvox; off += chunk) {
    const int64_t c = std::min(chunk, nvox - off);
    hipLaunchKernelGGL(k_esdf_dist, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, h->stream, st->d2.as<uint32_t>(), st->sign.as<uint64_t>(), st->box[3], st->words, off, c,
                       voxel, (float *)h->scratch.p);
    TSDF_HIP_TRY(hipGetLastError());
    if ((rc = tsdf_to_host(h, dist + off, h->scratch.p, (size_t)c * 4))) return rc;
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_esdf_fetch_device(tsdf_handle h, uint32_t *d_d2, float *d_dist) {
  if (!h) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_esdf_fetch_device");
  TSDF_ENTER(h);
  tsdf_esdf_state *st = esdf_ready(h, "tsdf_hip_esdf_fetch_device");
  if (!st) return TSDF_HIP_E_INVALID;
  const int64_t nvox = (int64_t)st->box[3] * st->box[4] * st->box[5];
  if (d_d2) TSDF_HIP_TRY(hipMemcpyAsync(d_d2, st->d2.p, (size_t)nvox * 4, hipMemcpyDeviceToDevice, h->stream));
  if (d_dist) {
    const int64_t chunk = (int64_t)1 << 30;
    for (int64_t off = 0; off < nvox; off += chunk) {
      const int64_t c = std::min(chunk, nvox - off);
      hipLaunchKernelGGL(k_esdf_dist, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, h->stream, st->d2.as<uint32_t>(), st->sign.as<uint64_t>(), st->box[3], st->words, off, c,
                         tsdf_voxel_edge(h->p), d_dist + off);
      TSDF_HIP_TRY(hipGetLastError());
    }
  }
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_esdf_sample(tsdf_handle h, const float *xyz, size_t n, float *dist, uint8_t *found) {
  if (!h || !xyz || !n || !dist || !found) return TSDF_HIP_E_INVALID;
  TSDF_NOT_ON_MULTI(h, "tsdf_hip_esdf_sample");
  TSDF_ENTER(h);
  tsdf_esdf_state *st = esdf_ready(h, "tsdf_hip_esdf_sample");
  if (!st) return TSDF_HIP_E_INVALID;
  int rc = tsdf_ensure_scratch(h, n * 17 + 16);
  if (rc) return rc;
  float *d_xyz = (float *)h->scratch.p, *d_dist = d_xyz + 3 * n;
  unsigned char *d_found = (unsigned char *)(d_dist + n);
  if ((rc = tsdf_to_device(h, d_xyz, xyz, n * 12))) return rc;
  hipLaunchKernelGGL(k_esdf_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, make_view(h), st->d2.as<uint32_t>(), st->sign.as<uint64_t>(), st->box[0],
                     st->box[1], st->box[2], st->box[3], st->box[4], st->box[5], st->words, tsdf_voxel_edge(h->p), d_xyz, n, d_dist, d_found);
  TSDF_HIP_TRY(hipGetLastError());
  if ((rc = tsdf_to_host(h, dist, d_dist, n * 4))) return rc;
  return tsdf_to_host(h, found, d_found, n);
}

extern "C" int tsdf_hip_esdf_stats(tsdf_handle h, uint64_t out[4]) {
  if (!h || !out) return TSDF_HIP_E_INVALID;
  out[0] = out[1] = out[2] = out[3] = 0;
  const tsdf_esdf_state *st = h->esdf;
  if (!st) return TSDF_HIP_OK;
  out[2] = st->d2.cap + st->sign.cap + st->stack.cap;
  if (!st->valid) return TSDF_HIP_OK;
  out[0] = (uint64_t)st->box[3] * st->box[4] * st->box[5];
  out[1] = st->sites;
  out[3] = (uint64_t)(st->ms * 1000.f);
  return TSDF_HIP_OK;
}
