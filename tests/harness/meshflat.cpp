// Test harness (tests/test_flatten_oracle.py, tests/test_flatten_dropin_gpu.py): the two --flatten passes of the `integrate`
// program on one mesh -- the host's cpu_tsdf::mesh_post::flattenVertices, which defines the result, and flattenVerticesGpu,
// which asks the library (tsdf_hip_mesh_flatten) for the seeds and the faces -- each on its own copy, both results dumped for
// a byte comparison.
//
//   meshflat <mesh.bin> <out.bin> <min_dist> [--host-only]
// mesh.bin: int64 n_verts, n_faces; n_verts x 3 float; n_faces x 3 uint32.
// out.bin:  for the host pass, then (without --host-only, which touches no device) for the GPU-backed pass: int64
//           point_step, blob bytes, n_polygons; the cloud blob; per polygon int64 size and its uint32 indices.
#include <pcl/PolygonMesh.h>
#include <pcl/conversions.h>
#include <pcl/point_types.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mesh_post.h"

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

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

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const bool host_only = argc > 4 && !strcmp(argv[4], "--host-only");
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n[2];
  if (!rd(f, n, sizeof n) || n[0] < 0 || n[1] < 0) return 4;
  std::vector<float> xyz((size_t)n[0] * 3);
  std::vector<uint32_t> idx((size_t)n[1] * 3);
  if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, idx.data(), idx.size() * 4)) return 5;
  fclose(f);
  const float min_dist = (float)atof(argv[3]);
  pcl::PointCloud<pcl::PointXYZ> cloud;
  for (int64_t i = 0; i < n[0]; ++i) {
    pcl::PointXYZ p;
    p.x = xyz[3 * i], p.y = xyz[3 * i + 1], p.z = xyz[3 * i + 2];
    cloud.push_back(p);
  }
  pcl::PolygonMesh host;
  pcl::toPCLPointCloud2(cloud, host.cloud);
  host.polygons.resize((size_t)n[1]);
  for (int64_t t = 0; t < n[1]; ++t) {
    host.polygons[t].vertices.resize(3);
    for (int j = 0; j < 3; ++j) host.polygons[t].vertices[j] = idx[3 * t + j];
  }
  pcl::PolygonMesh gpu = host;
  cpu_tsdf::mesh_post::flattenVertices(host, min_dist);
  if (!host_only)
    if (const int rc = cpu_tsdf::mesh_post::flattenVerticesGpu(gpu, min_dist)) {
      fprintf(stderr, "flattenVerticesGpu: %s: %s\n", tsdf_hip_error_string(rc), tsdf_hip_last_error());
      return 6;
    }
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 7;
  dump(o, host);
  if (!host_only) dump(o, gpu);
  fclose(o);
  return 0;
}
