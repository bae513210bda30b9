// Test harness of the meshNormals tests.
//
//   meshnormals arrays <mesh.bin> <out.bin>
// The host pass that defines the result, cpu_tsdf::mesh_post::normalArrays, on raw arrays; touches no device
// (tests/test_normals_oracle.py).
// mesh.bin: int64 n_verts, n_faces, null_faces (1: faces == NULL, a soup), has_rgb; n_verts x 3 float; n_verts x 3 bytes when
//           has_rgb; n_faces x 3 uint32 unless null_faces.
// out.bin:  int64 rc; when rc == 0: int64 n, skipped faces, zero normals; normals n x 3 float; flags n bytes.  Otherwise: the
//           reason as text, then one byte: 1 when the pass left its output untouched.
//
//   meshnormals ply <mesh.bin> <prefix> <normals 0|1|2>
// A PolygonMesh from the arrays (with an rgb field when has_rgb); with normals != 0 cpu_tsdf::mesh_post::meshNormals on it (2:
// twice -- the second call rewrites the fields); then pcl::io::savePLYFile -> <prefix>.ascii.ply and savePLYFileBinary ->
// <prefix>.binary.ply.  Touches no device.  Exit status 6 when the pass refuses (its reason on stderr).
//
//   meshnormals mesh <mesh.bin> <out.bin>
// The two --normals passes of the programs on copies of one PolygonMesh: the host's meshNormals and meshNormalsGpu
// (tests/test_normals_dropin_gpu.py).  out.bin: for the host pass, then for the GPU-backed pass, one mesh: int64 point_step,
// blob bytes, n_polygons, n_fields; per field 16 bytes of name and int64 offset; the cloud blob; per polygon int64 size and
// its uint32 indices.
//
//   meshnormals volume <volume file> <out.bin> <min weight> <colour 0|1> <flatten 0|1> <decimate cell_size, 0: none> <smooth iterations, 0: none>
// cpu_tsdf::MarchingCubesTSDFOctree with setNormals on a volume saved by TSDFVolumeOctree::save
// (tests/test_normals_dropin_gpu.py).  out.bin: one mesh, as above.
#include <cpu_tsdf/marching_cubes_tsdf_octree.h>
#include <cpu_tsdf/tsdf_volume_octree.h>
#include <pcl/PolygonMesh.h>
#include <pcl/io/ply_io.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mesh_post.h"

struct Mesh {
  bool null_faces = false;
  size_t n_faces = 0;
  std::vector<float> xyz;
  std::vector<uint8_t> rgb;
  std::vector<uint32_t> idx;
};

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int read_mesh(const char *src, Mesh &m) {
  FILE *f = fopen(src, "rb");
  if (!f) return 3;
  int64_t n[4];
  if (!rd(f, n, sizeof n) || n[0] < 0 || n[1] < 0) return 4;
  m.null_faces = n[2] != 0;
  m.n_faces = (size_t)n[1];
  m.xyz.resize((size_t)n[0] * 3);
  m.rgb.resize(n[3] ? (size_t)n[0] * 3 : 0);
  m.idx.resize(m.null_faces ? 0 : (size_t)n[1] * 3);
  if (!rd(f, m.xyz.data(), m.xyz.size() * 4) || !rd(f, m.rgb.data(), m.rgb.size()) || !rd(f, m.idx.data(), m.idx.size() * 4)) return 5;
  fclose(f);
  return 0;
}

static int run_arrays(const char *src, const char *dst) {
  Mesh m;
  if (const int rc = read_mesh(src, m)) return rc;
  static const uint32_t none[3] = {0, 0, 0};
  cpu_tsdf::mesh_post::Normals r;
  r.normals.assign(1, 42.f);  // a refusal must leave this alone
  std::string why;
  const int64_t rc = cpu_tsdf::mesh_post::normalArrays(m.xyz.data(), m.xyz.size() / 3, m.null_faces ? nullptr : (m.idx.empty() ? none : m.idx.data()),
                                                       m.n_faces, r, &why);
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  fwrite(&rc, sizeof rc, 1, o);
  if (rc) {
    const char untouched = r.normals.size() == 1 && r.normals[0] == 42.f && r.flags.empty() && r.skipped == 0 && r.zero == 0;
    fwrite(why.data(), 1, why.size(), o);
    fwrite(&untouched, 1, 1, o);
  } else {
    const int64_t hdr[3] = {(int64_t)r.flags.size(), (int64_t)r.skipped, (int64_t)r.zero};
    fwrite(hdr, sizeof hdr, 1, o);
    fwrite(r.normals.data(), 4, r.normals.size(), o);
    fwrite(r.flags.data(), 1, r.flags.size(), o);
  }
  fclose(o);
  return 0;
}

static void dump(FILE *o, const pcl::PolygonMesh &m) {
  const int64_t hdr[4] = {(int64_t)m.cloud.point_step, (int64_t)m.cloud.data.size(), (int64_t)m.polygons.size(), (int64_t)m.cloud.fields.size()};
  fwrite(hdr, sizeof hdr, 1, o);
  for (const auto &f : m.cloud.fields) {
    char name[16] = {0};
    strncpy(name, f.name.c_str(), 15);
    const int64_t off = (int64_t)f.offset;
    fwrite(name, 1, 16, o);
    fwrite(&off, sizeof off, 1, o);
  }
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

// a PolygonMesh from the arrays; a soup gets the polygons (3f, 3f + 1, 3f + 2)
static void to_mesh(Mesh &m, pcl::PolygonMesh &mesh) {
  if (m.null_faces) {
    m.idx.resize(m.n_faces * 3);
    for (size_t e = 0; e < m.idx.size(); ++e) m.idx[e] = (uint32_t)e;
  }
  cpu_tsdf::mesh_post::storeDecimated(m.xyz, m.rgb, m.xyz.size() / 3, m.idx.data(), m.idx.size() / 3, mesh);
}

static int run_ply(const char *src, const char *prefix, int normals) {
  Mesh m;
  if (const int rc = read_mesh(src, m)) return rc;
  pcl::PolygonMesh mesh;
  to_mesh(m, mesh);
  for (int k = 0; k < normals; ++k) {
    std::string why;
    if (cpu_tsdf::mesh_post::meshNormals(mesh, &why)) {
      fprintf(stderr, "meshNormals: %s\n", why.c_str());
      return 6;
    }
  }
  if (pcl::io::savePLYFile(std::string(prefix) + ".ascii.ply", mesh)) return 7;
  if (pcl::io::savePLYFileBinary(std::string(prefix) + ".binary.ply", mesh)) return 7;
  return 0;
}

static int run_mesh(const char *src, const char *dst) {
  Mesh m;
  if (const int rc = read_mesh(src, m)) return rc;
  pcl::PolygonMesh host;
  to_mesh(m, host);
  pcl::PolygonMesh gpu = host;
  std::string why;
  if (cpu_tsdf::mesh_post::meshNormals(host, &why)) {
    fprintf(stderr, "meshNormals: %s\n", why.c_str());
    return 6;
  }
  if (cpu_tsdf::mesh_post::meshNormalsGpu(gpu, 0, &why)) {
    fprintf(stderr, "meshNormalsGpu: %s\n", why.c_str());
    return 6;
  }
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  dump(o, host);
  dump(o, gpu);
  fclose(o);
  return 0;
}

static int run_volume(const char *src, const char *dst, char **more) {
  cpu_tsdf::TSDFVolumeOctree::Ptr tsdf(new cpu_tsdf::TSDFVolumeOctree);
  tsdf->load(src);
  if (!tsdf->handle()) return 3;
  cpu_tsdf::MarchingCubesTSDFOctree mc;
  mc.setInputTSDF(tsdf);
  mc.setMinWeight((float)atof(more[0]));
  mc.setColorByRGB(atoi(more[1]) != 0);
  if (atoi(more[2])) mc.setFlatten();
  if (atof(more[3]) > 0) mc.setDecimate((float)atof(more[3]));
  if (atoi(more[4]) > 0) mc.setSmooth(atoi(more[4]));
  mc.setNormals(false);  // (a later call replaces an earlier one)
  mc.setNormals();
  pcl::PolygonMesh m;
  mc.reconstruct(m);
  FILE *o = fopen(dst, "wb");
  if (!o) return 7;
  dump(o, m);
  fclose(o);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  if (argc == 4 && !strcmp(argv[1], "arrays")) return run_arrays(argv[2], argv[3]);
  if (argc == 5 && !strcmp(argv[1], "ply")) return run_ply(argv[2], argv[3], atoi(argv[4]));
  if (argc == 4 && !strcmp(argv[1], "mesh")) return run_mesh(argv[2], argv[3]);
  if (argc == 9 && !strcmp(argv[1], "volume")) return run_volume(argv[2], argv[3], argv + 4);
  return 2;
}
