// Test harness (tests/test_align_dropin_gpu.py): cpu_tsdf::TSDFVolumeOctree::getAlignmentSystem and alignCloud of the C++
// drop-in on a volume the harness fuses itself, results dumped for a byte comparison with the Python binding.
//
//   align <in.bin> <out.bin>
// in.bin:  int64 res, width, height, n_frames, n_points, max_iterations; double size, fx, fy, cx, cy;
//          per frame 16 doubles (camera -> volume, row-major) and width x height floats of depth;
//          n_points x 3 floats; 16 doubles: the pose of the system and the guess.
// out.bin: 29 doubles (getAlignmentSystem at the guess); int64 ok; 16 doubles (alignCloud's refined pose);
//          int64: 1 if BOTH calls refused on a volume whose setGridSize is not a cube.
#include <cpu_tsdf/tsdf_volume_octree.h>

#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static Eigen::Affine3d to_affine(const double *m16) {
  Eigen::Affine3d t = Eigen::Affine3d::Identity();
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) t.matrix()(r, c) = m16[4 * r + c];
  return t;
}

static void configure(cpu_tsdf::TSDFVolumeOctree &vol, int res, int W, int H, const double *g, float sx, float sy, float sz) {
  vol.setResolution(res, res, res);
  vol.setGridSize(sx, sy, sz);
  vol.setImageSize(W, H);
  vol.setCameraIntrinsics(g[1], g[2], g[3], g[4]);
  vol.setSensorDistanceBounds(0.f, 3.f * (float)g[0]);
  vol.setDepthTruncationLimits(0.03f, 0.03f);
  vol.setWeightTruncationLimit(100.f);
  vol.setIntegrateColor(false);
  vol.reset();
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n[6];
  double g[5], pose[16];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g)) return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  cpu_tsdf::TSDFVolumeOctree vol;
  configure(vol, res, W, H, g, (float)g[0], (float)g[0], (float)g[0]);
  std::vector<float> depth((size_t)W * H);
  for (int64_t k = 0; k < n[3]; ++k) {
    if (!rd(f, pose, sizeof pose) || !rd(f, depth.data(), depth.size() * 4)) return 5;
    if (!vol.integratePlanar(depth.data(), nullptr, W, H, to_affine(pose))) return 6;
  }
  std::vector<float> xyz((size_t)n[4] * 3);
  if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, pose, sizeof pose)) return 5;
  fclose(f);
  const Eigen::Affine3d guess = to_affine(pose);
  // the template strips points without a finite z: put some in, the result must not notice
  pcl::PointCloud<pcl::PointXYZ> cloud;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int64_t i = 0; i < n[4]; ++i) {
    if (i % 1000 == 0) cloud.push_back(pcl::PointXYZ(0.f, 0.f, i % 2000 ? nan : std::numeric_limits<float>::infinity()));
    cloud.push_back(pcl::PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
  }
  double sys[29];
  if (!vol.getAlignmentSystem(xyz.data(), (size_t)n[4], guess, sys)) return 7;
  Eigen::Affine3d refined = Eigen::Affine3d::Identity();
  const int64_t ok = vol.alignCloud(cloud, guess, refined, (int)n[5], 0.f, 0.9f, 0.0) ? 1 : 0;
  double out16[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out16[4 * r + c] = refined.matrix()(r, c);
  cpu_tsdf::TSDFVolumeOctree flat;
  configure(flat, res, W, H, g, (float)g[0], (float)g[0], (float)g[0] / 2);
  double sys2[29];
  Eigen::Affine3d r2 = Eigen::Affine3d::Identity();
  const int64_t refused = (!flat.getAlignmentSystem(xyz.data(), (size_t)n[4], guess, sys2) && !flat.alignCloud(cloud, guess, r2)) ? 1 : 0;
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 8;
  fwrite(sys, sizeof sys, 1, o);
  fwrite(&ok, sizeof ok, 1, o);
  fwrite(out16, sizeof out16, 1, o);
  fwrite(&refused, sizeof refused, 1, o);
  fclose(o);
  return 0;
}
