// Test harness (tests/test_align_abi.py): the host arithmetic of tsdf_hip_align -- cpu_tsdf_amd/csrc/tsdf_se3.h, the very
// header tsdf_align.hip includes -- on inputs from a file; no device, no library.
//
//   se3 exp   <in.bin> <out.bin>    in: k x 6 doubles (omega, v);           out: k x 12 doubles, the rows of [R | t]
//   se3 solve <in.bin> <out.bin>    in: k x 29 doubles (tsdf_hip_align_system); out: k x 7 doubles: status, then the step
#include <cstdio>
#include <cstring>
#include <vector>

#include "tsdf_se3.h"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const bool solve = !strcmp(argv[1], "solve");
  if (!solve && strcmp(argv[1], "exp")) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double v;
  while (fread(&v, sizeof v, 1, f) == 1) in.push_back(v);
  fclose(f);
  const size_t per = solve ? 29 : 6;
  if (in.empty() || in.size() % per) return 4;
  FILE *o = fopen(argv[3], "wb");
  if (!o) return 5;
  for (size_t k = 0; k < in.size() / per; ++k) {
    if (solve) {
      double out[7] = {0, 0, 0, 0, 0, 0, 0};
      out[0] = tsdf_solve_step(&in[per * k], out + 1);
      fwrite(out, sizeof out, 1, o);
    } else {
      double T[12];
      tsdf_se3_exp(&in[per * k], T);
      fwrite(T, sizeof T, 1, o);
    }
  }
  fclose(o);
  return 0;
}
