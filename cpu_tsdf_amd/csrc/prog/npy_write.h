// A float32 array as a NumPy .npy file, format version 1.0: the magic string, the version, a little-endian uint16 header
// length, a Python dict literal padded with spaces so that the data starts on a 64-byte boundary, then the raw
// little-endian values in C order.  What numpy.load reads; no dependency.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>

static inline bool npy_write_f32(const char *path, const float *data, size_t nz, size_t ny, size_t nx) {
  std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(nz) + ", " + std::to_string(ny) + ", " +
                     std::to_string(nx) + "), }";
  while ((10 + dict.size() + 1) % 64) dict += ' ';
  dict += '\n';
  const uint16_t len = (uint16_t)dict.size();
  const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(len & 255), (unsigned char)(len >> 8)};
  FILE *f = fopen(path, "wb");
  if (!f) return false;
  const size_t n = nz * ny * nx;
  bool ok = fwrite(head, 1, 10, f) == 10 && fwrite(dict.data(), 1, dict.size(), f) == dict.size() && fwrite(data, 4, n, f) == n;
  return (fclose(f) == 0) && ok;
}
