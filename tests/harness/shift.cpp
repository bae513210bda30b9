// Test harness (tests/test_shift_dropin_gpu.py): cpu_tsdf::TSDFVolumeOctree::shiftVolume of the C++ drop-in on a volume the
// harness fuses itself, results dumped for a byte comparison with the Python binding.
//
//   shift <in.bin> <out.bin>
// in.bin:  int64 res, width, height, n_frames, sx, sy, sz; double size, fx, fy, cx, cy; 16 doubles: the global transform set
//          before the shift (row-major); per frame 16 doubles (camera -> volume, row-major) and width x height floats of depth.
// out.bin: int64 ok (shiftVolume's return value); int64: 1 if shiftVolume on a volume before reset() returned false;
//          3 doubles (moved); 16 doubles (getGlobalTransform().matrix(), row-major); res^3 floats d; res^3 floats w
//          (downloadBlock of the whole grid).
#include <cpu_tsdf/tsdf_volume_octree.h>

#include <cstdint>
#include <cstdio>
#include <vector>

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static Eigen::Affine3d to_affine(const double *m16) {
  Eigen::Affine3d t = Eigen::Affine3d::Identity();
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) t.matrix()(r, c) = m16[4 * r + c];
  return t;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n[7];
  double g[5], pose[16];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g) || !rd(f, pose, sizeof pose)) return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  cpu_tsdf::TSDFVolumeOctree early;
  Eigen::Vector3d untouched(7., 8., 9.);
  const int64_t refused = (!early.shiftVolume(1, 0, 0, &untouched) && untouched[0] == 7. && untouched[1] == 8. && untouched[2] == 9.) ? 1 : 0;
  cpu_tsdf::TSDFVolumeOctree vol;
  vol.setResolution(res, res, res);
  vol.setGridSize((float)g[0], (float)g[0], (float)g[0]);
  vol.setImageSize(W, H);
  vol.setCameraIntrinsics(g[1], g[2], g[3], g[4]);
  vol.setSensorDistanceBounds(0.f, 3.f * (float)g[0]);
  vol.setDepthTruncationLimits(0.03f, 0.03f);
  vol.setWeightTruncationLimit(100.f);
  vol.setIntegrateColor(false);
  vol.reset();
  vol.setGlobalTransform(to_affine(pose));
  std::vector<float> depth((size_t)W * H);
  for (int64_t k = 0; k < n[3]; ++k) {
    if (!rd(f, pose, sizeof pose) || !rd(f, depth.data(), depth.size() * 4)) return 5;
    if (!vol.integratePlanar(depth.data(), nullptr, W, H, to_affine(pose))) return 6;
  }
  fclose(f);
  Eigen::Vector3d moved(0., 0., 0.);
  const int64_t ok = vol.shiftVolume((int)n[4], (int)n[5], (int)n[6], &moved) ? 1 : 0;
  const Eigen::Affine3d gt = vol.getGlobalTransform();
  double m3[3] = {moved[0], moved[1], moved[2]}, out16[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out16[4 * r + c] = gt.matrix()(r, c);
  const size_t nv = (size_t)res * res * res;
  std::vector<float> d(nv), w(nv);
  if (!vol.downloadBlock(0, 0, 0, res, res, res, d.data(), w.data(), nullptr)) return 7;
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 8;
  fwrite(&ok, sizeof ok, 1, o);
  fwrite(&refused, sizeof refused, 1, o);
  fwrite(m3, sizeof m3, 1, o);
  fwrite(out16, sizeof out16, 1, o);
  fwrite(d.data(), 4, nv, o);
  fwrite(w.data(), 4, nv, o);
  fclose(o);
  return 0;
}
