// Test harness (tests/test_castrays_admit.py): ray_admit of cpu_tsdf_amd/csrc/tsdf_ray_admit.h -- the admission rule of
// tsdf_hip_cast_rays, the very function the kernels call -- compiled with the host compiler alone and run over a table of rays.
//
//   castrays_admit <table.txt>
// table.txt: one ray per line, 9 float32 bit patterns in hex: ox oy oz ux uy uz tmin tmax leaf.
// stdout:    one line per ray: "<admitted 0|1> <cap>".
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "tsdf_ray_admit.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 3;
  unsigned w[9];
  while (fscanf(f, "%x %x %x %x %x %x %x %x %x", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8]) == 9) {
    float v[9];
    for (int k = 0; k < 9; ++k) {
      const uint32_t bits = w[k];
      memcpy(&v[k], &bits, 4);
    }
    uint32_t cap = 12345u;
    const bool ok = ray_admit(v, v + 3, v[6], v[7], v[8], &cap);
    printf("%d %u\n", ok ? 1 : 0, (unsigned)cap);
  }
  fclose(f);
  return 0;
}
