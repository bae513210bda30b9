// Test harness of the smoothMesh tests.
//
//   meshsmooth arrays <mesh.bin> <out.bin> <lambda> <mu> <iterations> <keep_boundary>
// The host pass that defines the result, cpu_tsdf::mesh_post::smoothArrays, on raw arrays; touches no device
// (tests/test_smooth_oracle.py).
// mesh.bin: int64 n_verts, n_faces (-1: faces == NULL), has_rgb; n_verts x 3 float; n_verts x 3 bytes when has_rgb;
//           n_faces x 3 uint32.
// out.bin:  int64 rc; when rc == 0: int64 n, unique edges; vertices n x 3 float; fixed n bytes; degree n x uint32.  Otherwise:
//           the reason as text, then one byte: 1 when the pass left its output untouched.
//
//   meshsmooth mesh <mesh.bin> <out.bin> <lambda> <mu> <iterations> <keep_boundary>
// The two --smooth passes of the programs on copies of one PolygonMesh (with an rgb field when has_rgb): the host's
// cpu_tsdf::mesh_post::smoothMesh and smoothMeshGpu (tests/test_smooth_dropin_gpu.py).
// out.bin:  for the host pass, then for the GPU-backed pass: int64 point_step, blob bytes, n_polygons; the cloud blob; per
//           polygon int64 size and its uint32 indices.
//
//   meshsmooth volume <volume file> <out.bin> <lambda> <mu> <iterations> <keep_boundary> <min weight> <colour 0|1> <decimate cell_size, 0: none>
// cpu_tsdf::MarchingCubesTSDFOctree with setSmooth on a volume saved by TSDFVolumeOctree::save
// (tests/test_smooth_dropin_gpu.py).  out.bin: one mesh, as above.
#include <cpu_tsdf/marching_cubes_tsdf_octree.h>
#include <cpu_tsdf/tsdf_volume_octree.h>
#include <pcl/PolygonMesh.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mesh_post.h"

struct Args {
  float lambda, mu;
  int iterations, keep_boundary;
};

struct Mesh {
  bool null_faces = false;
  std::vector<float> xyz;
  std::vector<uint8_t> rgb;
  std::vector<uint32_t> idx;
};

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int read_mesh(const char *src, Mesh &m) {
  FILE *f = fopen(src, "rb");
  if (!f) return 3;
  int64_t n[3];
  if (!rd(f, n, sizeof n) || n[0] < 0) return 4;
  m.null_faces = n[1] < 0;
  m.xyz.resize((size_t)n[0] * 3);
  m.rgb.resize(n[2] ? (size_t)n[0] * 3 : 0);
  m.idx.resize(m.null_faces ? 0 : (size_t)n[1] * 3);
  if (!rd(f, m.xyz.data(), m.xyz.size() * 4) || !rd(f, m.rgb.data(), m.rgb.size()) || !rd(f, m.idx.data(), m.idx.size() * 4)) return 5;
  fclose(f);
  return 0;
}

static int run_arrays(const char *src, const char *dst, const Args &a) {
  Mesh m;
  if (const int rc = read_mesh(src, m)) return rc;
  static const uint32_t none[3] = {0, 0, 0};
  cpu_tsdf::mesh_post::Smoothed s;
  s.verts.assign(1, 42.f);  // a refusal must leave this alone
  std::string why;
  const int64_t rc = cpu_tsdf::mesh_post::smoothArrays(m.xyz.data(), m.xyz.size() / 3, m.null_faces ? nullptr : (m.idx.empty() ? none : m.idx.data()),
                                                       m.idx.size() / 3, a.lambda, a.mu, a.iterations, a.keep_boundary, s, &why);
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  fwrite(&rc, sizeof rc, 1, o);
  if (rc) {
    const char untouched = s.verts.size() == 1 && s.verts[0] == 42.f && s.fixed.empty() && s.degree.empty();
    fwrite(why.data(), 1, why.size(), o);
    fwrite(&untouched, 1, 1, o);
  } else {
    const int64_t hdr[2] = {(int64_t)s.fixed.size(), (int64_t)s.edges};
    fwrite(hdr, sizeof hdr, 1, o);
    fwrite(s.verts.data(), 4, s.verts.size(), o);
    fwrite(s.fixed.data(), 1, s.fixed.size(), o);
    fwrite(s.degree.data(), 4, s.degree.size(), o);
  }
  fclose(o);
  return 0;
}

static void dump(FILE *o, const pcl::PolygonMesh &m) {
  const int64_t hdr[3] = {(int64_t)m.cloud.point_step, (int64_t)m.cloud.data.size(), (int64_t)m.polygons.size()};
  fwrite(hdr, sizeof hdr, 1, o);
  fwrite(m.cloud.data.data(), 1, m.cloud.data.size(), o);
  for (const pcl::Vertices &p : m.polygons) {
    const int64_t k = (int64_t)p.vertices.size();
    fwrite(&k, sizeof k, 1, o);
    for (size_t j = 0; j < p.vertices.size(); ++j) {
      const uint32_t v = (uint32_t)p.vertices[j];
      fwrite(&v, sizeof v, 1, o);
    }
  }
}

static int run_mesh(const char *src, const char *dst, const Args &a) {
  Mesh m;
  if (const int rc = read_mesh(src, m)) return rc;
  if (m.null_faces) return 4;
  pcl::PolygonMesh host;
  cpu_tsdf::mesh_post::storeDecimated(m.xyz, m.rgb, m.xyz.size() / 3, m.idx.data(), m.idx.size() / 3, host);  // (a mesh from arrays)
  pcl::PolygonMesh gpu = host;
  std::string why;
  if (cpu_tsdf::mesh_post::smoothMesh(host, a.iterations, a.lambda, a.mu, a.keep_boundary != 0, &why)) {
    fprintf(stderr, "smoothMesh: %s\n", why.c_str());
    return 6;
  }
  if (cpu_tsdf::mesh_post::smoothMeshGpu(gpu, a.iterations, a.lambda, a.mu, a.keep_boundary != 0, 0, &why)) {
    fprintf(stderr, "smoothMeshGpu: %s\n", why.c_str());
    return 6;
  }
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  dump(o, host);
  dump(o, gpu);
  fclose(o);
  return 0;
}

static int run_volume(const char *src, const char *dst, const Args &a, char **more) {
  cpu_tsdf::TSDFVolumeOctree::Ptr tsdf(new cpu_tsdf::TSDFVolumeOctree);
  tsdf->load(src);
  if (!tsdf->handle()) return 3;
  cpu_tsdf::MarchingCubesTSDFOctree mc;
  mc.setInputTSDF(tsdf);
  mc.setMinWeight((float)atof(more[0]));
  mc.setColorByRGB(atoi(more[1]) != 0);
  if (atof(more[2]) > 0) mc.setDecimate((float)atof(more[2]));
  mc.setSmooth(999);  // (a second call replaces the first)
  mc.setSmooth(a.iterations, a.lambda, a.mu, a.keep_boundary != 0);
  pcl::PolygonMesh m;
  mc.reconstruct(m);
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  dump(o, m);
  fclose(o);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 8) return 2;
  const Args a{(float)atof(argv[4]), (float)atof(argv[5]), atoi(argv[6]), atoi(argv[7])};
  if (argc == 8 && !strcmp(argv[1], "arrays")) return run_arrays(argv[2], argv[3], a);
  if (argc == 8 && !strcmp(argv[1], "mesh")) return run_mesh(argv[2], argv[3], a);
  if (argc == 11 && !strcmp(argv[1], "volume")) return run_volume(argv[2], argv[3], a, argv + 8);
  return 2;
}
