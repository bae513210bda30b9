// Test harness (tests/test_esdf_dropin_gpu.py): computeDistanceField / getDistanceField / getDistance of the C++ drop-in on a
// volume the harness fuses itself, results dumped for a byte comparison with the Python binding.
//
//   esdf <in.bin> <out.bin>
// in.bin:  int64 res, width, height, n_frames, n_points; double size, fx, fy, cx, cy; n_frames frames, each 16 doubles
//          (camera -> volume, row-major) and width x height floats of depth; then n_points x 3 floats.
// out.bin: int64: 1 if all three members returned false on a volume before reset() and left their outputs alone; then twice --
//          r_max 0, then r_max 2 -- int64 ok, uint64 sites, res^3 uint32 d2, res^3 floats dist, n_points int64 (getDistance's
//          return value), n_points floats (its dist; 7 where it returned false).
#include <cpu_tsdf/tsdf_volume_octree.h>

#include <cstdint>
#include <cstdio>
#include <vector>

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n[5];
  double g[5];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g)) return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  cpu_tsdf::TSDFVolumeOctree vol, early;
  vol.setResolution(res, res, res);
  vol.setGridSize((float)g[0], (float)g[0], (float)g[0]);
  vol.setImageSize(W, H);
  vol.setCameraIntrinsics(g[1], g[2], g[3], g[4]);
  vol.setSensorDistanceBounds(0.f, 3.f * (float)g[0]);
  vol.setDepthTruncationLimits(0.03f, 0.03f);
  vol.setWeightTruncationLimit(100.f);
  vol.setIntegrateColor(false);
  vol.reset();
  std::vector<float> depth((size_t)W * H);
  for (int64_t k = 0; k < n[3]; ++k) {
    double pose[16];
    if (!rd(f, pose, sizeof pose) || !rd(f, depth.data(), depth.size() * 4)) return 5;
    Eigen::Affine3d t = Eigen::Affine3d::Identity();
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) t.matrix()(r, c) = pose[4 * r + c];
    if (!vol.integratePlanar(depth.data(), nullptr, W, H, t)) return 6;
  }
  std::vector<float> pts((size_t)n[4] * 3);
  if (!rd(f, pts.data(), pts.size() * 4)) return 5;
  fclose(f);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 8;
  {
    uint64_t sites = 7;
    std::vector<float> dist(3, 7.f);
    float one = 7.f;
    const bool a = early.computeDistanceField(0, 0.f, &sites), b = early.getDistanceField(dist), c = early.getDistance(pcl::PointXYZ(0.f, 0.f, 0.f), one);
    // (and on a volume that is ready but holds no field yet)
    const bool d = vol.getDistanceField(dist), e = vol.getDistance(pcl::PointXYZ(0.f, 0.f, 0.f), one);
    const int64_t refused = (!a && !b && !c && !d && !e && sites == 7 && one == 7.f) ? 1 : 0;
    fwrite(&refused, sizeof refused, 1, o);
  }
  const size_t nv = (size_t)res * res * res;
  for (int r_max : {0, 2}) {
    uint64_t sites = 0;
    std::vector<float> dist;
    std::vector<uint32_t> d2;
    const int64_t ok = (vol.computeDistanceField(r_max, 0.f, &sites) && vol.getDistanceField(dist, &d2) && dist.size() == nv && d2.size() == nv) ? 1 : 0;
    if (!ok) return 7;
    fwrite(&ok, sizeof ok, 1, o);
    fwrite(&sites, sizeof sites, 1, o);
    fwrite(d2.data(), 4, nv, o);
    fwrite(dist.data(), 4, nv, o);
    std::vector<int64_t> found((size_t)n[4]);
    std::vector<float> val((size_t)n[4], 7.f);
    for (size_t k = 0; k < found.size(); ++k)
      found[k] = vol.getDistance(pcl::PointXYZ(pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]), val[k]) ? 1 : 0;
    fwrite(found.data(), 8, found.size(), o);
    fwrite(val.data(), 4, val.size(), o);
  }
  fclose(o);
  return 0;
}
