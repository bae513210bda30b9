// Test harness (tests/test_castrays_dropin_gpu.py): cpu_tsdf::TSDFVolumeOctree::castRays of the C++ drop-in on a volume fused
// from organised host clouds, results dumped for a byte comparison with the Python binding.
//
//   castrays <in.bin> <out.bin>
// in.bin:  int64 res, width, height, n_frames, n_rays, with_range; double size, fx, fy, cx, cy; n_frames frames, each 16
//          doubles (camera -> volume, row-major), width x height floats of depth and width x height x 4 bytes b, g, r, a;
//          then n_rays x 3 floats of origins, n_rays x 3 floats of directions, n_rays x 2 floats tmin, tmax.
// out.bin: int64: 1 if castRays before reset() returned false and left the cloud and the status alone; int64 ok of castRays
//          after all frames were integrated (t_range passed iff with_range); int64 width, height, is_dense of the cloud; per
//          point 6 floats x, y, z, normal_x, normal_y, normal_z; per point 3 bytes r, g, b; n_rays status bytes.
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
  int64_t n[6];
  double g[5];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g)) return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  const size_t n_frames = (size_t)n[3], n_rays = (size_t)n[4];
  const bool with_range = n[5] != 0;
  std::vector<Eigen::Affine3d> poses;
  std::vector<pcl::PointCloud<pcl::PointXYZRGBA>> clouds;
  std::vector<float> depth((size_t)W * H);
  std::vector<unsigned char> bgra((size_t)W * H * 4);
  for (size_t k = 0; k < n_frames; ++k) {
    double pose[16];
    if (!rd(f, pose, sizeof pose) || !rd(f, depth.data(), depth.size() * 4) || !rd(f, bgra.data(), bgra.size())) return 5;
    poses.push_back(to_affine(pose));
    pcl::PointCloud<pcl::PointXYZRGBA> cloud(W, H);
    for (size_t i = 0; i < depth.size(); ++i) {
      pcl::PointXYZRGBA &pt = cloud.points[i];
      pt.x = pt.y = 0.f;  // (only z and the colour are read)
      pt.z = depth[i];
      pt.b = bgra[4 * i], pt.g = bgra[4 * i + 1], pt.r = bgra[4 * i + 2], pt.a = 255;
    }
    clouds.push_back(cloud);
  }
  std::vector<float> org(3 * n_rays), dir(3 * n_rays), range(2 * n_rays);
  if (!rd(f, org.data(), org.size() * 4) || !rd(f, dir.data(), dir.size() * 4) || !rd(f, range.data(), range.size() * 4)) return 5;
  fclose(f);
  const pcl::PointCloud<pcl::Normal> no_normals;
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 8;
  cpu_tsdf::TSDFVolumeOctree vol;
  vol.setResolution(res, res, res);
  vol.setGridSize((float)g[0], (float)g[0], (float)g[0]);
  vol.setImageSize(W, H);
  vol.setCameraIntrinsics(g[1], g[2], g[3], g[4]);
  vol.setSensorDistanceBounds(0.f, 3.f * (float)g[0]);
  vol.setDepthTruncationLimits(0.03f, 0.03f);
  vol.setWeightTruncationLimit(100.f);
  vol.setIntegrateColor(true);
  {
    pcl::PointCloud<pcl::PointXYZRGBNormal> untouched(3, 1);
    std::vector<uint8_t> st(2, 9);
    const int64_t refused = (!vol.castRays(org.data(), dir.data(), n_rays, untouched, &st) && untouched.size() == 3 && st.size() == 2 &&
                             st[0] == 9 && st[1] == 9) ? 1 : 0;
    fwrite(&refused, sizeof refused, 1, o);
  }
  vol.reset();
  for (size_t k = 0; k < n_frames; ++k)
    if (!vol.integrateCloud(clouds[k], no_normals, poses[k])) return 6;
  pcl::PointCloud<pcl::PointXYZRGBNormal> hits;
  std::vector<uint8_t> status;
  const int64_t ok = vol.castRays(org.data(), dir.data(), n_rays, hits, &status, with_range ? range.data() : nullptr) ? 1 : 0;
  const int64_t shape[3] = {(int64_t)hits.width, (int64_t)hits.height, hits.is_dense ? 1 : 0};
  fwrite(&ok, sizeof ok, 1, o);
  fwrite(shape, sizeof shape, 1, o);
  for (size_t i = 0; i < hits.size(); ++i) {
    const pcl::PointXYZRGBNormal &pt = hits.points[i];
    const float v[6] = {pt.x, pt.y, pt.z, pt.normal_x, pt.normal_y, pt.normal_z};
    fwrite(v, sizeof v, 1, o);
  }
  for (size_t i = 0; i < hits.size(); ++i) {
    const pcl::PointXYZRGBNormal &pt = hits.points[i];
    const unsigned char c[3] = {pt.r, pt.g, pt.b};
    fwrite(c, 1, 3, o);
  }
  fwrite(status.data(), 1, status.size(), o);
  fclose(o);
  return 0;
}
