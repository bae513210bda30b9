// Test harness (tests/test_reintegrate_dropin_gpu.py): cpu_tsdf::TSDFVolumeOctree::reintegrateCloud of the C++ drop-in on
// organised host clouds, results dumped for a byte comparison with the Python binding.
//
//   reintegrate <in.bin> <out.bin>
// in.bin:  int64 res, width, height, n_frames, repose; double size, fx, fy, cx, cy; 16 doubles: the corrected pose of frame
//          `repose`; then n_frames frames, each 16 doubles (camera -> volume, row-major), width x height floats of depth and
//          width x height x 4 bytes b, g, r, a.
// out.bin: int64: 1 if reintegrateCloud before reset() returned false and left *lowered / *observed alone; then int64 ok,
//          uint64 lowered, uint64 observed of reintegrateCloud(frame `repose`, its pose, the corrected pose) after all frames
//          were integrated; res^3 floats d, res^3 floats w, 3 res^3 bytes rgb (downloadBlock of the whole grid).
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
  int64_t n[5];
  double g[5];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g)) return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  const size_t n_frames = (size_t)n[3], repose = (size_t)n[4];
  if (repose >= n_frames) return 4;
  double corrected[16];
  if (!rd(f, corrected, sizeof corrected)) return 4;
  const Eigen::Affine3d new_pose = to_affine(corrected);
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
    uint64_t untouched[2] = {7, 9};
    const int64_t refused = (!vol.reintegrateCloud(clouds[repose], no_normals, poses[repose], new_pose, &untouched[0], &untouched[1]) &&
                             untouched[0] == 7 && untouched[1] == 9) ? 1 : 0;
    fwrite(&refused, sizeof refused, 1, o);
  }
  vol.reset();
  for (size_t k = 0; k < n_frames; ++k)
    if (!vol.integrateCloud(clouds[k], no_normals, poses[k])) return 6;
  uint64_t lowered = 0, observed = 0;
  const int64_t ok = vol.reintegrateCloud(clouds[repose], no_normals, poses[repose], new_pose, &lowered, &observed) ? 1 : 0;
  const size_t nv = (size_t)res * res * res;
  std::vector<float> d(nv), w(nv);
  std::vector<unsigned char> rgb(3 * nv);
  if (!vol.downloadBlock(0, 0, 0, res, res, res, d.data(), w.data(), rgb.data())) return 7;
  fwrite(&ok, sizeof ok, 1, o);
  fwrite(&lowered, sizeof lowered, 1, o);
  fwrite(&observed, sizeof observed, 1, o);
  fwrite(d.data(), 4, nv, o);
  fwrite(w.data(), 4, nv, o);
  fwrite(rgb.data(), 1, 3 * nv, o);
  fclose(o);
  return 0;
}
