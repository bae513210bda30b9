// Test harness (tests/test_merge_dropin_gpu.py): cpu_tsdf::TSDFVolumeOctree::mergeVolume of the C++ drop-in on volumes the
// harness fuses itself, results dumped for a byte comparison with the Python binding.
//
//   merge <in.bin> <out.bin>
// in.bin:  int64 res, width, height, n_a, n_b; double size, fx, fy, cx, cy; 16 doubles each (row-major): the global transform
//          of dst, the global transform of src, dst_from_src; then n_a frames for dst and n_b frames for src, each 16 doubles
//          (camera -> volume, row-major) and width x height floats of depth.
// out.bin: int64: 1 if mergeVolume with a volume before reset() on either side returned false; then twice -- mergeVolume with
//          the explicit transform, mergeVolume through the two global transforms, each into a freshly fused dst -- int64 ok,
//          uint64 merged, res^3 floats d, res^3 floats w (downloadBlock of the whole grid).
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

struct Frame {
  double pose[16];
  std::vector<float> depth;
};

static bool fuse(cpu_tsdf::TSDFVolumeOctree &vol, int res, int W, int H, const double *g, const double *global, const std::vector<Frame> &frames) {
  vol.setResolution(res, res, res);
  vol.setGridSize((float)g[0], (float)g[0], (float)g[0]);
  vol.setImageSize(W, H);
  vol.setCameraIntrinsics(g[1], g[2], g[3], g[4]);
  vol.setSensorDistanceBounds(0.f, 3.f * (float)g[0]);
  vol.setDepthTruncationLimits(0.03f, 0.03f);
  vol.setWeightTruncationLimit(100.f);
  vol.setIntegrateColor(false);
  vol.reset();
  vol.setGlobalTransform(to_affine(global));
  for (const Frame &fr : frames)
    if (!vol.integratePlanar(fr.depth.data(), nullptr, W, H, to_affine(fr.pose))) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n[5];
  double g[5], g_dst[16], g_src[16], d_from_s[16];
  if (!rd(f, n, sizeof n) || !rd(f, g, sizeof g) || !rd(f, g_dst, sizeof g_dst) || !rd(f, g_src, sizeof g_src) || !rd(f, d_from_s, sizeof d_from_s))
    return 4;
  const int res = (int)n[0], W = (int)n[1], H = (int)n[2];
  std::vector<Frame> fa((size_t)n[3]), fb((size_t)n[4]);
  for (std::vector<Frame> *fs : {&fa, &fb})
    for (Frame &fr : *fs) {
      fr.depth.resize((size_t)W * H);
      if (!rd(f, fr.pose, sizeof fr.pose) || !rd(f, fr.depth.data(), fr.depth.size() * 4)) return 5;
    }
  fclose(f);
  cpu_tsdf::TSDFVolumeOctree src;
  if (!fuse(src, res, W, H, g, g_src, fb)) return 6;
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 8;
  {
    cpu_tsdf::TSDFVolumeOctree early, ready;
    if (!fuse(ready, res, W, H, g, g_dst, fa)) return 6;
    uint64_t untouched = 7;
    const int64_t refused = (!early.mergeVolume(src, nullptr, 0.f, &untouched) && !ready.mergeVolume(early, nullptr, 0.f, &untouched) && untouched == 7) ? 1 : 0;
    fwrite(&refused, sizeof refused, 1, o);
  }
  const size_t nv = (size_t)res * res * res;
  std::vector<float> d(nv), w(nv);
  for (int mode = 0; mode < 2; ++mode) {
    cpu_tsdf::TSDFVolumeOctree dst;
    if (!fuse(dst, res, W, H, g, g_dst, fa)) return 6;
    const Eigen::Affine3d explicit_t = to_affine(d_from_s);
    uint64_t merged = 0;
    const int64_t ok = dst.mergeVolume(src, mode == 0 ? &explicit_t : nullptr, 0.f, &merged) ? 1 : 0;
    if (!dst.downloadBlock(0, 0, 0, res, res, res, d.data(), w.data(), nullptr)) return 7;
    fwrite(&ok, sizeof ok, 1, o);
    fwrite(&merged, sizeof merged, 1, o);
    fwrite(d.data(), 4, nv, o);
    fwrite(w.data(), 4, nv, o);
  }
  fclose(o);
  return 0;
}
