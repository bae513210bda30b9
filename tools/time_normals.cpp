// Timing program of tools/time_normals.py: the two --normals passes of the programs -- the host's
// cpu_tsdf::mesh_post::meshNormals and meshNormalsGpu (tsdf_hip_mesh_normals: upload, device pass, download) -- on prefixes of
// one indexed mesh, wall clock, one JSON line per prefix.
//
//   time_normals <mesh.bin> <n_verts> [<n_verts> ...]
// mesh.bin: int64 n_verts, n_faces; n_verts x 3 float; n_faces x 3 uint32 (as tsdf_hip_march_fetch_indexed returns them).
// A prefix of n vertices keeps the faces whose three corners lie below n.
#include <pcl/PolygonMesh.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mesh_post.h"

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static pcl::PolygonMesh prefix_mesh(const std::vector<float> &xyz, const std::vector<uint32_t> &idx, size_t n) {
  std::vector<uint32_t> faces;
  for (size_t f = 0; f < idx.size() / 3; ++f)
    if (idx[3 * f] < n && idx[3 * f + 1] < n && idx[3 * f + 2] < n) faces.insert(faces.end(), &idx[3 * f], &idx[3 * f] + 3);
  pcl::PolygonMesh m;
  cpu_tsdf::mesh_post::storeDecimated(xyz, std::vector<uint8_t>(), n, faces.data(), faces.size() / 3, m);
  return m;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n_all[2] = {0, 0};
  if (fread(n_all, sizeof n_all, 1, f) != 1 || n_all[0] < 0 || n_all[1] < 0) return 4;
  std::vector<float> xyz((size_t)n_all[0] * 3);
  std::vector<uint32_t> idx((size_t)n_all[1] * 3);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || fread(idx.data(), 4, idx.size(), f) != idx.size()) return 5;
  fclose(f);
  {  // the first GPU call of a process pays for the runtime's start: not part of any figure
    pcl::PolygonMesh warm = prefix_mesh(xyz, idx, (size_t)(n_all[0] < 64 ? n_all[0] : 64));
    if (cpu_tsdf::mesh_post::meshNormalsGpu(warm)) return 6;
  }
  for (int a = 2; a < argc; ++a) {
    const size_t n = (size_t)std::min<long long>(atoll(argv[a]), n_all[0]);
    const pcl::PolygonMesh in = prefix_mesh(xyz, idx, n);
    double host_ms = 1e300, gpu_ms = 1e300;
    uint64_t st[4] = {0, 0, 0, 0};
    pcl::PolygonMesh host;
    for (int rep = 0; rep < 3; ++rep) {  // the best of three, for both
      host = in;
      const double t0 = now_ms();
      if (cpu_tsdf::mesh_post::meshNormals(host)) return 8;
      const double ms = now_ms() - t0;
      if (ms < host_ms) host_ms = ms;
    }
    for (int rep = 0; rep < 3; ++rep) {
      pcl::PolygonMesh m = in;
      const double t1 = now_ms();
      if (const int rc = cpu_tsdf::mesh_post::meshNormalsGpu(m)) {
        fprintf(stderr, "meshNormalsGpu: %s: %s\n", tsdf_hip_error_string(rc), tsdf_hip_last_error());
        return 6;
      }
      const double ms = now_ms() - t1;
      if (ms < gpu_ms) gpu_ms = ms;
      tsdf_hip_mesh_normals_stats(st);
      if (m.cloud.data != host.cloud.data) {
        fprintf(stderr, "the passes disagree at %zu vertices\n", n);
        return 7;
      }
    }
    printf("{\"vertices\": %zu, \"faces\": %zu, \"skipped_faces\": %llu, \"zero_normals\": %llu, \"host_pass_wall_ms\": %.3f, "
           "\"gpu_backed_pass_wall_ms\": %.3f, \"gpu_device_ms\": %.3f}\n",
           n, in.polygons.size(), (unsigned long long)st[1], (unsigned long long)st[2], host_ms, gpu_ms, (double)st[3] / 1000.);
    fflush(stdout);
  }
  return 0;
}
