// Timing program of tools/time_decimate.py: the two --decimate passes of the programs -- the host's
// cpu_tsdf::mesh_post::decimateMesh and decimateMeshGpu (tsdf_hip_mesh_decimate + the host's vertex blob) -- on prefixes of
// one mesh, wall clock, one JSON line per prefix.
//
//   time_decimate <mesh.bin> <cell_size> <max_host_faces> <n_faces> [<n_faces> ...]
// mesh.bin: int64 n_tri; n_tri x 9 float (triangle soup, as tsdf_hip_march_fetch returns it).
// The host pass is skipped for prefixes of more than max_host_faces faces (it is one thread).
#include <pcl/PolygonMesh.h>
#include <pcl/conversions.h>
#include <pcl/point_types.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mesh_post.h"

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static pcl::PolygonMesh soup_mesh(const std::vector<float> &xyz, size_t n_tri) {
  pcl::PointCloud<pcl::PointXYZ> cloud;
  cloud.points.resize(3 * n_tri);
  cloud.width = (uint32_t)(3 * n_tri), cloud.height = 1;
  for (size_t i = 0; i < 3 * n_tri; ++i) cloud.points[i].x = xyz[3 * i], cloud.points[i].y = xyz[3 * i + 1], cloud.points[i].z = xyz[3 * i + 2];
  pcl::PolygonMesh m;
  pcl::toPCLPointCloud2(cloud, m.cloud);
  m.polygons.resize(n_tri);
  for (size_t t = 0; t < n_tri; ++t) {
    m.polygons[t].vertices.resize(3);
    for (int j = 0; j < 3; ++j) m.polygons[t].vertices[j] = (uint32_t)(3 * t + j);
  }
  return m;
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n_all = 0;
  if (fread(&n_all, sizeof n_all, 1, f) != 1 || n_all < 0) return 4;
  std::vector<float> xyz((size_t)n_all * 9);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size()) return 5;
  fclose(f);
  const float cell_size = (float)atof(argv[2]);
  const long long max_host = atoll(argv[3]);
  {  // the first GPU call of a process pays for the runtime's start: not part of any figure
    pcl::PolygonMesh warm = soup_mesh(xyz, (size_t)(n_all < 64 ? n_all : 64));
    if (cpu_tsdf::mesh_post::decimateMeshGpu(warm, cell_size)) return 6;
  }
  for (int a = 4; a < argc; ++a) {
    const size_t n = (size_t)std::min<long long>(atoll(argv[a]), n_all);
    double host_ms = -1.;
    long long host_kept = -1, host_verts = -1;
    if ((long long)n <= max_host) {
      pcl::PolygonMesh m = soup_mesh(xyz, n);
      const double t0 = now_ms();
      if (cpu_tsdf::mesh_post::decimateMesh(m, cell_size)) return 8;
      host_ms = now_ms() - t0;
      host_kept = (long long)m.polygons.size();
      host_verts = (long long)m.cloud.width * m.cloud.height;
    }
    double gpu_ms = 1e300;
    uint64_t st[4] = {0, 0, 0, 0};
    long long gpu_kept = -1, gpu_verts = -1;
    for (int rep = 0; rep < 3; ++rep) {  // the best of three
      pcl::PolygonMesh m = soup_mesh(xyz, n);
      const double t0 = now_ms();
      if (const int rc = cpu_tsdf::mesh_post::decimateMeshGpu(m, cell_size)) {
        fprintf(stderr, "decimateMeshGpu: %s: %s\n", tsdf_hip_error_string(rc), tsdf_hip_last_error());
        return 6;
      }
      const double ms = now_ms() - t0;
      if (ms < gpu_ms) gpu_ms = ms;
      tsdf_hip_mesh_decimate_stats(st);
      gpu_kept = (long long)m.polygons.size();
      gpu_verts = (long long)m.cloud.width * m.cloud.height;
    }
    if (host_kept >= 0 && (host_kept != gpu_kept || host_verts != gpu_verts)) {
      fprintf(stderr, "the passes disagree at %zu faces: host keeps %lld faces and %lld vertices, GPU %lld and %lld\n", n, host_kept, host_verts,
              gpu_kept, gpu_verts);
      return 7;
    }
    printf("{\"faces\": %zu, \"vertices\": %zu, \"vertices_out\": %lld, \"faces_out\": %lld, \"host_pass_wall_ms\": %.3f, "
           "\"gpu_backed_pass_wall_ms\": %.3f, \"gpu_device_ms\": %.3f, \"duplicate_faces\": %llu}\n",
           n, 3 * n, gpu_verts, gpu_kept, host_ms, gpu_ms, (double)st[3] / 1000., (unsigned long long)st[2]);
    fflush(stdout);
  }
  return 0;
}
