// Timing program of tools/time_align.py: what a caller of the C++ drop-in paid per Gauss-Newton iteration before alignCloud --
// one getFxnAndGradient call (one launch, one device round trip) per point -- against alignCloud itself, on a volume the
// program fuses from the frames in its input.  Wall clock, one JSON line.
//
//   time_align <in.bin> <n_loop_points>
// in.bin: the format of tests/harness/align.cpp (int64 res, width, height, n_frames, n_points, max_iterations; double size,
//         fx, fy, cx, cy; per frame a pose and a depth image; the cloud; the guess).
#include <cpu_tsdf/tsdf_volume_octree.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
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
  int64_t n[6];
  double g[5], pose[16];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g)) return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  cpu_tsdf::TSDFVolumeOctree vol;
  vol.setResolution(res, res, res);
  vol.setGridSize((float)g[0], (float)g[0], (float)g[0]);
  vol.setImageSize(W, H);
  vol.setCameraIntrinsics(g[1], g[2], g[3], g[4]);
  vol.setSensorDistanceBounds(0.f, 3.f * (float)g[0]);
  vol.setIntegrateColor(false);
  vol.reset();
  std::vector<float> depth((size_t)W * H);
  for (int64_t k = 0; k < n[3]; ++k) {
    if (!rd(f, pose, sizeof pose) || !rd(f, depth.data(), depth.size() * 4)) return 5;
    if (!vol.integratePlanar(depth.data(), nullptr, W, H, to_affine(pose))) return 6;
  }
  std::vector<float> xyz((size_t)n[4] * 3);
  if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, pose, sizeof pose)) return 5;
  fclose(f);
  const Eigen::Affine3d guess = to_affine(pose);
  float M[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) M[4 * r + c] = (float)guess.matrix()(r, c);
  const size_t m = std::min<size_t>((size_t)atoll(argv[2]), (size_t)n[4]);
  float val;
  Eigen::Vector3f grad;
  // the per-point loop: transform on the host, one call per point, the 29 sums on the host
  double acc[29] = {0};
  size_t ok = 0;
  for (int rep = 0; rep < 2; ++rep) {  // the first pass warms the runtime up
    const double t0 = now_ms();
    ok = 0;
    for (size_t i = 0; i < m; ++i) {
      float q[3];
      for (int r = 0; r < 3; ++r) q[r] = ((M[4 * r] * xyz[3 * i] + M[4 * r + 1] * xyz[3 * i + 1]) + M[4 * r + 2] * xyz[3 * i + 2]) + M[4 * r + 3];
      if (!vol.getFxnAndGradient(pcl::PointXYZ(q[0], q[1], q[2]), val, grad)) continue;
      const double J[6] = {(double)q[1] * grad(2) - (double)q[2] * grad(1), (double)q[2] * grad(0) - (double)q[0] * grad(2),
                           (double)q[0] * grad(1) - (double)q[1] * grad(0), grad(0), grad(1), grad(2)};
      int k = 0;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) acc[k++] += J[a] * J[b];
      ++ok;
    }
    acc[28] = now_ms() - t0;
  }
  const double loop_ms = acc[28];
  pcl::PointCloud<pcl::PointXYZ> cloud;
  for (int64_t i = 0; i < n[4]; ++i) cloud.push_back(pcl::PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
  Eigen::Affine3d refined;
  double best = 1e300;
  bool aligned = false;
  for (int rep = 0; rep < 4; ++rep) {  // best of three after one warm-up
    const double t0 = now_ms();
    aligned = vol.alignCloud(cloud, guess, refined, (int)n[5], 0.f, 0.9f, 0.0);
    const double ms = now_ms() - t0;
    if (rep && ms < best) best = ms;
  }
  printf("{\"loop_points\": %zu, \"loop_points_ok\": %zu, \"per_point_loop_wall_ms\": %.3f, \"per_point_us\": %.2f, "
         "\"align_cloud_points\": %lld, \"align_cloud_iterations\": %lld, \"align_cloud_wall_ms\": %.3f, \"align_cloud_ok\": %d}\n",
         m, ok, loop_ms, 1000. * loop_ms / (double)m, (long long)n[4], (long long)n[5], best, aligned ? 1 : 0);
  return 0;
}
