// Test harness of the decimateMesh tests.
//
//   meshdec arrays <mesh.bin> <out.bin> <cell_size>
// The host pass that defines the result, cpu_tsdf::mesh_post::decimateArrays, on raw arrays; touches no device
// (tests/test_decimate_oracle.py).
// mesh.bin: int64 n_verts, n_faces (-1: a soup of n_verts / 3 faces), has_rgb; n_verts x 3 float; n_verts x 3 bytes when
//           has_rgb; n_faces x 3 uint32 unless a soup.
// out.bin:  int64 rc; when rc == 0: int64 n, m, k, has_rgb, duplicates; remap n x uint32; vertices m x 3 float; rgb m x 3 bytes
//           when has_rgb; counts m x uint32; faces k x 3 uint32.  Otherwise: the reason as text.
//
//   meshdec mesh <mesh.bin> <out.bin> <cell_size>
// The two --decimate passes of the programs on copies of one PolygonMesh (with an rgb field when has_rgb): the host's
// cpu_tsdf::mesh_post::decimateMesh and decimateMeshGpu (tests/test_decimate_dropin_gpu.py).  mesh.bin as above, indexed.
// out.bin:  for the host pass, then for the GPU-backed pass: int64 point_step, blob bytes, n_polygons; the cloud blob; per
//           polygon int64 size and its uint32 indices.
//
//   meshdec volume <volume file> <out.bin> <cell_size> <min weight> <colour 0|1> <cleanup face_dist> <cleanup min_neighbors, -1: none>
//           <flatten min_dist, 0: none>
// cpu_tsdf::MarchingCubesTSDFOctree with setDecimate on a volume saved by TSDFVolumeOctree::save
// (tests/test_decimate_dropin_gpu.py).
// out.bin:  int64 point_step, blob bytes, n_polygons; the cloud blob; per polygon int64 size and its uint32 indices.
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

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int run_arrays(const char *src, const char *dst, float cell_size) {
  FILE *f = fopen(src, "rb");
  if (!f) return 3;
  int64_t n[3];
  if (!rd(f, n, sizeof n) || n[0] < 0) return 4;
  const bool soup = n[1] < 0;
  const size_t nv = (size_t)n[0], nf = soup ? nv / 3 : (size_t)n[1];
  std::vector<float> xyz(nv * 3);
  std::vector<uint8_t> rgb(n[2] ? nv * 3 : 0);
  std::vector<uint32_t> idx(soup ? 0 : nf * 3);
  if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, rgb.data(), rgb.size()) || !rd(f, idx.data(), idx.size() * 4)) return 5;
  fclose(f);
  cpu_tsdf::mesh_post::Decimated d;
  std::string why;
  const int64_t rc = cpu_tsdf::mesh_post::decimateArrays(xyz.data(), n[2] ? rgb.data() : nullptr, nv, soup ? nullptr : idx.data(), nf, cell_size, d, &why);
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  fwrite(&rc, sizeof rc, 1, o);
  if (rc) {
    fwrite(why.data(), 1, why.size(), o);
  } else {
    const int64_t hdr[5] = {(int64_t)nv, (int64_t)d.counts.size(), (int64_t)(d.faces.size() / 3), n[2] ? 1 : 0, (int64_t)d.duplicates};
    fwrite(hdr, sizeof hdr, 1, o);
    fwrite(d.remap.data(), 4, d.remap.size(), o);
    fwrite(d.verts.data(), 4, d.verts.size(), o);
    fwrite(d.rgb.data(), 1, d.rgb.size(), o);
    fwrite(d.counts.data(), 4, d.counts.size(), o);
    fwrite(d.faces.data(), 4, d.faces.size(), o);
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

static int run_mesh(const char *src, const char *dst, float cell_size) {
  FILE *f = fopen(src, "rb");
  if (!f) return 3;
  int64_t n[3];
  if (!rd(f, n, sizeof n) || n[0] < 0 || n[1] < 0) return 4;
  const size_t nv = (size_t)n[0], nf = (size_t)n[1];
  std::vector<float> xyz(nv * 3);
  std::vector<uint8_t> rgb(n[2] ? nv * 3 : 0);
  std::vector<uint32_t> idx(nf * 3);
  if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, rgb.data(), rgb.size()) || !rd(f, idx.data(), idx.size() * 4)) return 5;
  fclose(f);
  pcl::PolygonMesh host;
  cpu_tsdf::mesh_post::storeDecimated(xyz, rgb, nv, idx.data(), nf, host);  // (the tail builds a mesh from arrays: any arrays)
  pcl::PolygonMesh gpu = host;
  std::string why;
  if (const int rc = cpu_tsdf::mesh_post::decimateMesh(host, cell_size, &why)) {
    fprintf(stderr, "decimateMesh: %s\n", why.c_str());
    return 6;
  }
  if (const int rc = cpu_tsdf::mesh_post::decimateMeshGpu(gpu, cell_size)) {
    fprintf(stderr, "decimateMeshGpu: %s: %s\n", tsdf_hip_error_string(rc), tsdf_hip_last_error());
    return 6;
  }
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  dump(o, host);
  dump(o, gpu);
  fclose(o);
  return 0;
}

static int run_volume(char **a) {
  cpu_tsdf::TSDFVolumeOctree::Ptr tsdf(new cpu_tsdf::TSDFVolumeOctree);
  tsdf->load(a[0]);
  if (!tsdf->handle()) return 3;
  cpu_tsdf::MarchingCubesTSDFOctree mc;
  mc.setInputTSDF(tsdf);
  mc.setMinWeight((float)atof(a[3]));
  mc.setColorByRGB(atoi(a[4]) != 0);
  if (atoi(a[6]) >= 0) mc.setCleanup((float)atof(a[5]), atoi(a[6]));
  if (atof(a[7]) > 0) mc.setFlatten((float)atof(a[7]));
  mc.setDecimate(1e9f);  // (a second call replaces the first)
  mc.setDecimate((float)atof(a[2]));
  pcl::PolygonMesh m;
  mc.reconstruct(m);
  FILE *o = fopen(a[1], "wb");
  if (!o) return 7;
  dump(o, m);
  fclose(o);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "arrays")) return run_arrays(argv[2], argv[3], (float)atof(argv[4]));
  if (argc == 5 && !strcmp(argv[1], "mesh")) return run_mesh(argv[2], argv[3], (float)atof(argv[4]));
  if (argc == 10 && !strcmp(argv[1], "volume")) return run_volume(argv + 2);
  return 2;
}
