// Micro-benchmark: the rate of k_integrate's frame gather on gfx950 -- per-lane indexed buffer loads from an L2-resident
// 640x480 frame, with the kernel's own access shape: a wave's 64 lanes x 4 voxels spread over a segment of ~80 consecutive
// pixels (a wave-row of 256 voxels projects to about that), a fresh segment per row, eight waves per SIMD.
//   (a) 8 x buffer_load_dword idxen    -- depth + bgra from the planar frame [depth | bgra], as k_integrate's colour instances did
//   (b) 4 x buffer_load_dwordx2 idxen  -- the same pixels from 8-byte records {depth, bgra}
//   (c) 4 x buffer_load_dword idxen    -- the colourless shape (depth only)
// Reported: ms, gather wave-instructions per clock per CU, bytes returned to lanes per clock per CU (engine clock as the
// runtime reports it).  Why: DESIGN.md 3.1 (round 7) -- whether the colour row is bound by vector-memory INSTRUCTIONS.
// build: hipcc --offload-arch=gfx950 -O3 tools/ubench/gather_rate.hip -o tools/ubench/gather_rate ; run: tools/ubench/gather_rate
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef int i4_rsrc __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));
__device__ unsigned struct_load_u32(i4_rsrc rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.i32");
__device__ u2 struct_load_u32x2(i4_rsrc rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.v2i32");

static __device__ __forceinline__ i4_rsrc make_rsrc_2d(const void *p, unsigned stride) {
  const unsigned long long a = (unsigned long long)p;
  i4_rsrc r;
  r.x = (int)(a & 0xffffffffull);
  r.y = (int)(((a >> 32) & 0xffffull) | ((unsigned long long)(stride & 0x3fffu) << 16));
  r.z = (int)0xffffffffu;  // no range check wanted: every index below is inside the frame by construction
  r.w = 0x00020000;
  return r;
}

constexpr int W = 640, H = 480, NPIX = W * H, SEG = 80;

// MODE 0: (a), 1: (b), 2: (c).  `frame`: planar [depth | bgra] for 0 and 2, records for 1.
template <int MODE>
__global__ void __launch_bounds__(256) k_gather(const uint32_t *frame, unsigned *out, int rows) {
  const i4_rsrc rs = make_rsrc_2d(frame, MODE == 1 ? 8u : 4u);
  const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  unsigned off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) off[j] = ((lane * 4u + (unsigned)j) * SEG) >> 8;  // 0 .. 79: four neighbouring lanes share a pixel
  unsigned base = (wave * 977u) % (unsigned)(NPIX - SEG);  // wave-uniform
  unsigned acc = 0;
  for (int r = 0; r < rows; ++r) {
    unsigned z[4], c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pix = (int)(base + off[j]);  // < NPIX
      if (MODE == 1) {
        const u2 v = struct_load_u32x2(rs, pix, 0, 0, 0);
        z[j] = v.x, c[j] = v.y;
      } else {
        z[j] = struct_load_u32(rs, pix, 0, 0, 0);
        if (MODE == 0) c[j] = struct_load_u32(rs, pix, 0, NPIX * 4, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += z[j] ^ c[j];
    base += W + 3u;  // the next voxel row's segment: about one image row on
    if (base >= (unsigned)(NPIX - SEG)) base -= (unsigned)(NPIX - SEG);
  }
  out[blockIdx.x * 256u + threadIdx.x] = acc;
}

int main() {
  const int blocks = 256 * 8 * 2, rows = 4000;  // 8 resident blocks of 4 waves per CU = 8 waves per SIMD, two rounds
  std::vector<uint32_t> planar(2 * NPIX), rec(2 * NPIX);
  for (int i = 0; i < NPIX; ++i) {
    planar[i] = 0x3f800000u + (unsigned)i, planar[NPIX + i] = (unsigned)i * 2654435761u;
    rec[2 * i] = planar[i], rec[2 * i + 1] = planar[NPIX + i];
  }
  uint32_t *d_planar = nullptr, *d_rec = nullptr;
  unsigned *d_out = nullptr;
  hipMalloc(&d_planar, planar.size() * 4);
  hipMalloc(&d_rec, rec.size() * 4);
  hipMalloc(&d_out, (size_t)blocks * 256 * 4);
  hipMemcpy(d_planar, planar.data(), planar.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(d_rec, rec.data(), rec.size() * 4, hipMemcpyHostToDevice);
  hipDeviceProp_t prop;
  hipGetDeviceProperties(&prop, 0);
  const double clock_hz = prop.clockRate * 1e3;
  const int cus = prop.multiProcessorCount;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  printf("# engine clock reported: %.0f MHz, %d CUs; %d blocks x 4 waves x %d rows; frame %d x %d (%.1f MB)\n", clock_hz * 1e-6, cus, blocks, rows,
         W, H, NPIX * 8 / 1e6);
  struct V {
    const char *name;
    void (*k)(const uint32_t *, unsigned *, int);
    const uint32_t *frame;
    int instr, bytes_per_lane;  // gather instructions per wave-row; bytes one lane receives per row
  } list[] = {{"(a) 8 x dword idxen, planar [depth | bgra]", k_gather<0>, d_planar, 8, 32},
              {"(b) 4 x dwordx2 idxen, 8-byte records", k_gather<1>, d_rec, 4, 32},
              {"(c) 4 x dword idxen, depth only", k_gather<2>, d_planar, 4, 16}};
  std::vector<unsigned> sums[3];
  for (int rep = 0; rep < 3; ++rep) {
    int vi = 0;
    for (const V &v : list) {
      hipLaunchKernelGGL(v.k, dim3(blocks), dim3(256), 0, 0, v.frame, d_out, rows);  // warm: code object, L2
      hipEventRecord(e0);
      hipLaunchKernelGGL(v.k, dim3(blocks), dim3(256), 0, 0, v.frame, d_out, rows);
      hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) {
        printf("kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
      }
      float ms = 0;
      hipEventElapsedTime(&ms, e0, e1);
      const double wave_rows = (double)blocks * 4 * rows, clocks = ms * 1e-3 * clock_hz;
      printf("rep %d %-44s %8.3f ms  %6.3f gather wave-instr / clk / CU  %7.1f B / clk / CU  %6.1f clk per wave-row per CU\n", rep, v.name, ms,
             wave_rows * v.instr / clocks / cus, wave_rows * 64 * v.bytes_per_lane / clocks / cus, clocks * cus / wave_rows);
      if (rep == 0) {
        sums[vi].resize((size_t)blocks * 256);
        hipMemcpy(sums[vi].data(), d_out, sums[vi].size() * 4, hipMemcpyDeviceToHost);
      }
      ++vi;
    }
  }
  // (a) and (b) fetch the same bits
  printf("# (a) and (b) return the same values: %s\n", sums[0] == sums[1] ? "yes" : "NO");
  return sums[0] == sums[1] ? 0 : 1;
}
