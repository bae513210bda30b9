// Mesh post-processing of the `integrate` program (--flatten / --cleanup), re-implemented without a
// kd-tree library: both passes only ever ask "which points lie strictly within r of this one", which a
// uniform hash grid of cell r answers from the 27 surrounding cells.
//
// Contracts reproduced (src/prog/integrate.cpp):
//   flattenVertices (:103-158): vertices are visited in index order; an unassigned vertex opens a new output
//     vertex and EVERY vertex strictly within min_dist of it -- assigned or not -- is (re)mapped to it; faces
//     are re-indexed, a face with two equal corners is dropped, face order is kept.  Colours are lost (the
//     reference converts the cloud to PointXYZ).  flattenVerticesGpu gets the same seeds and faces from the GPU
//     (tsdf_hip_mesh_flatten: the loop's result is a function of the input); the host pass stays: it
//     defines the result.
//   cleanupMesh (:160-237): faces whose centroids form a connected group (links: centroid distance strictly
//     below face_dist) of at most min_neighbors faces are removed; vertices no face uses are removed; vertex
//     and face order are kept.  Colours are lost likewise.  cleanupMeshGpu gets the same face set from the GPU
//     (tsdf_hip_mesh_cleanup); the host pass stays: it defines the result.
// An extension with no counterpart in the reference:
//   decimateMesh: vertex clustering (Rossignac-Borrel) on a grid of edge cell_size -- every occupied cell keeps one vertex,
//     the mean of its members; faces are re-indexed, degenerate and duplicate faces dropped.  decimateArrays below states the
//     rules; decimateMeshGpu gets the same arrays from the GPU (tsdf_hip_mesh_decimate); the host pass stays: it defines the
//     result.
//   smoothMesh: Taubin's lambda | mu smoothing of an indexed mesh over the neighbours its faces define -- only the vertices
//     move.  smoothArrays below states the rules; smoothMeshGpu gets the same vertices from the GPU (tsdf_hip_mesh_smooth);
//     the host pass stays: it defines the result.
//   meshNormals: area-weighted vertex normals of the final mesh, appended to the cloud as normal_x, normal_y, normal_z.
//     normalArrays below states the rules; meshNormalsGpu gets the same normals from the GPU (tsdf_hip_mesh_normals); the host
//     pass stays: it defines the result.
#pragma once

#include <pcl/PolygonMesh.h>
#include <pcl/conversions.h>
#include <pcl/point_types.h>

#include <tsdf_hip.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace cpu_tsdf {
namespace mesh_post {

class PointGrid {
 public:
  PointGrid(const std::vector<float> &xyz, double cell) : xyz_(xyz), cell_(cell) {
    for (size_t i = 0; i < xyz.size() / 3; ++i)
      if (finite(i)) cells_[key(c(xyz[3 * i]), c(xyz[3 * i + 1]), c(xyz[3 * i + 2]))].push_back((int)i);
  }
  // calls f(j) for every j (including i) with |p_j - p_i|^2 < r2, computed in float like a kd-tree would
  template <typename F>
  void forNeighbours(size_t i, float r2, F f) const {
    if (!finite(i)) return;
    const float x = xyz_[3 * i], y = xyz_[3 * i + 1], z = xyz_[3 * i + 2];
    const long cx = c(x), cy = c(y), cz = c(z);
    for (long dz = -1; dz <= 1; ++dz)
      for (long dy = -1; dy <= 1; ++dy)
        for (long dx = -1; dx <= 1; ++dx) {
          const auto it = cells_.find(key(cx + dx, cy + dy, cz + dz));
          if (it == cells_.end()) continue;
          for (int j : it->second) {
            const float ex = xyz_[3 * j] - x, ey = xyz_[3 * j + 1] - y, ez = xyz_[3 * j + 2] - z;
            if (ex * ex + ey * ey + ez * ez < r2) f(j);
          }
        }
  }

 private:
  bool finite(size_t i) const {
    return std::isfinite(xyz_[3 * i]) && std::isfinite(xyz_[3 * i + 1]) && std::isfinite(xyz_[3 * i + 2]);
  }
  long c(float v) const { return (long)std::floor((double)v / cell_); }
  static std::uint64_t key(long x, long y, long z) {
    return ((std::uint64_t)(x & 0x1fffff) << 42) | ((std::uint64_t)(y & 0x1fffff) << 21) | (std::uint64_t)(z & 0x1fffff);
  }
  const std::vector<float> &xyz_;
  double cell_;
  std::unordered_map<std::uint64_t, std::vector<int> > cells_;
};

inline std::vector<float> vertexPositions(const pcl::PolygonMesh &mesh) {
  pcl::PointCloud<pcl::PointXYZ> v;
  pcl::fromPCLPointCloud2(mesh.cloud, v);
  std::vector<float> xyz(3 * v.points.size());
  for (size_t i = 0; i < v.points.size(); ++i) {
    xyz[3 * i] = v.points[i].x;
    xyz[3 * i + 1] = v.points[i].y;
    xyz[3 * i + 2] = v.points[i].z;
  }
  return xyz;
}

inline void storeVertices(const std::vector<float> &xyz, const std::vector<int> &keep, pcl::PolygonMesh &mesh) {
  pcl::PointCloud<pcl::PointXYZ> out;
  for (int i : keep) {
    pcl::PointXYZ p;
    p.x = xyz[3 * i];
    p.y = xyz[3 * i + 1];
    p.z = xyz[3 * i + 2];
    out.push_back(p);
  }
  pcl::toPCLPointCloud2(out, mesh.cloud);
}

inline void flattenVertices(pcl::PolygonMesh &mesh, float min_dist = 0.0001f) {
  const std::vector<float> xyz = vertexPositions(mesh);
  const size_t n = xyz.size() / 3;
  const PointGrid grid(xyz, min_dist);
  const float r2 = (float)((double)min_dist * (double)min_dist);
  std::vector<int> remap(n, -1), seeds;
  for (size_t i = 0; i < n; ++i) {
    if (remap[i] >= 0) continue;
    const int idx = (int)seeds.size();
    remap[i] = idx;
    // the reference additionally requires the SQUARED distance to be below min_dist itself (:128)
    grid.forNeighbours(i, r2 < min_dist ? r2 : min_dist, [&](int j) { if ((size_t)j != i) remap[j] = idx; });
    seeds.push_back((int)i);
  }
  size_t kept = 0;
  for (size_t f = 0; f < mesh.polygons.size(); ++f) {
    pcl::Vertices &v = mesh.polygons[f];
    for (auto &k : v.vertices) k = (std::uint32_t)remap[k];
    if (v.vertices.size() >= 3 &&
        (v.vertices[0] == v.vertices[1] || v.vertices[1] == v.vertices[2] || v.vertices[2] == v.vertices[0]))
      continue;
    if (kept != f) mesh.polygons[kept] = mesh.polygons[f];
    ++kept;
  }
  mesh.polygons.resize(kept);
  storeVertices(xyz, seeds, mesh);
}

// The same result with the seeds and the re-indexed faces computed on the GPU (tsdf_hip_mesh_flatten, which reproduces the
// pass above vertex for vertex and face for face); the vertex blob is built here, as above.  A mesh with a polygon that is
// not a triangle keeps the host pass.  0, or the library's error code (its text in tsdf_hip_last_error) with the mesh
// untouched.
inline int flattenVerticesGpu(pcl::PolygonMesh &mesh, float min_dist = 0.0001f, int device = 0) {
  for (const auto &p : mesh.polygons)
    if (p.vertices.size() != 3) {
      flattenVertices(mesh, min_dist);
      return 0;
    }
  const std::vector<float> xyz = vertexPositions(mesh);
  const size_t n = xyz.size() / 3, nf = mesh.polygons.size();
  std::vector<std::uint32_t> faces(3 * nf), seeds(n);
  for (size_t f = 0; f < nf; ++f)
    for (int k = 0; k < 3; ++k) faces[3 * f + k] = mesh.polygons[f].vertices[k];
  std::uint64_t n_out = 0, n_kept = 0;
  // (the re-indexed faces come back in place of the ones handed over: the library has read those before it writes)
  const int rc = tsdf_hip_mesh_flatten(device, xyz.data(), n, faces.data(), nf, min_dist, nullptr, seeds.data(), &n_out, faces.data(), &n_kept);
  if (rc) return rc;
  mesh.polygons.resize((size_t)n_kept);
  for (size_t f = 0; f < (size_t)n_kept; ++f)
    for (int k = 0; k < 3; ++k) mesh.polygons[f].vertices[k] = faces[3 * f + k];
  storeVertices(xyz, std::vector<int>(seeds.begin(), seeds.begin() + (size_t)n_out), mesh);
  return 0;
}

// The tail of cleanupMesh (:208-237): the polygons with drop[f] set go, then the vertices no face uses; vertex and face
// order are kept, faces are re-indexed.
inline void dropFaces(pcl::PolygonMesh &mesh, const std::vector<float> &xyz, const std::vector<char> &drop) {
  size_t kept = 0;
  for (size_t f = 0; f < mesh.polygons.size(); ++f) {
    if (drop[f]) continue;
    if (kept != f) mesh.polygons[kept] = mesh.polygons[f];
    ++kept;
  }
  mesh.polygons.resize(kept);
  const size_t n = xyz.size() / 3;
  std::vector<int> new_index(n, -1), keep;
  std::vector<char> used(n, 0);
  for (const auto &p : mesh.polygons)
    for (int k = 0; k < 3; ++k) used[p.vertices[k]] = 1;
  for (size_t i = 0; i < n; ++i)
    if (used[i]) {
      new_index[i] = (int)keep.size();
      keep.push_back((int)i);
    }
  for (auto &p : mesh.polygons)
    for (int k = 0; k < 3; ++k) p.vertices[k] = (std::uint32_t)new_index[p.vertices[k]];
  storeVertices(xyz, keep, mesh);
}

inline void cleanupMesh(pcl::PolygonMesh &mesh, float face_dist = 0.02f, int min_neighbors = 5) {
  const std::vector<float> xyz = vertexPositions(mesh);
  // centroids of the triangles (:78-92: (v0 + v1 + v2) / 3 in float)
  std::vector<float> cen;
  std::vector<size_t> tri;  // polygon index of each centroid
  for (size_t f = 0; f < mesh.polygons.size(); ++f) {
    const auto &v = mesh.polygons[f].vertices;
    if (v.size() != 3) continue;
    for (int k = 0; k < 3; ++k) cen.push_back(((xyz[3 * v[0] + k] + xyz[3 * v[1] + k]) + xyz[3 * v[2] + k]) / 3.f);
    tri.push_back(f);
  }
  const size_t nf = tri.size();
  const PointGrid grid(cen, face_dist);
  const float r2 = (float)((double)face_dist * (double)face_dist);
  std::vector<char> seen(nf, 0), drop(mesh.polygons.size(), 0);
  std::vector<int> group;
  for (size_t i = 0; i < nf; ++i) {
    if (seen[i]) continue;
    group.assign(1, (int)i);
    seen[i] = 1;
    for (size_t q = 0; q < group.size(); ++q)
      grid.forNeighbours((size_t)group[q], r2, [&](int j) {
        if (!seen[j]) {
          seen[j] = 1;
          group.push_back(j);
        }
      });
    if ((int)group.size() <= min_neighbors)
      for (int g : group) drop[tri[g]] = 1;
  }
  dropFaces(mesh, xyz, drop);
}

// The same result with the groups found on the GPU (tsdf_hip_mesh_cleanup, which reproduces the pass above face for face):
// the triangles' keep mask comes from the library, the tail is the host's.  0, or the library's error code (its text in
// tsdf_hip_last_error) with the mesh untouched.
inline int cleanupMeshGpu(pcl::PolygonMesh &mesh, float face_dist = 0.02f, int min_neighbors = 5, int device = 0) {
  const std::vector<float> xyz = vertexPositions(mesh);
  std::vector<std::uint32_t> faces;
  std::vector<size_t> tri;  // polygon index of each face handed over (as above: only triangles take part)
  for (size_t f = 0; f < mesh.polygons.size(); ++f) {
    const auto &v = mesh.polygons[f].vertices;
    if (v.size() != 3) continue;
    for (int k = 0; k < 3; ++k) faces.push_back(v[k]);
    tri.push_back(f);
  }
  std::vector<std::uint8_t> keep(tri.size(), 1);
  std::uint64_t n_kept = 0;
  const int rc = tsdf_hip_mesh_cleanup(device, xyz.data(), xyz.size() / 3, faces.data(), tri.size(), face_dist, min_neighbors,
                                       keep.data(), &n_kept);
  if (rc) return rc;
  std::vector<char> drop(mesh.polygons.size(), 0);
  for (size_t i = 0; i < tri.size(); ++i)
    if (!keep[i]) drop[tri[i]] = 1;
  dropFaces(mesh, xyz, drop);
  return 0;
}

// Triangles below which --cleanup keeps the host pass: the largest prefix at which tools/time_cleanup.py measured the
// GPU-backed pass (upload, device pass, mask download, this file's tail) slower than cleanupMesh
// (profiles/cleanup_timing.json, "gpu_backed_pass_loses_up_to_faces": 3000 at 512^3 and at 2048^3, the next prefix, 5000,
// wins).
constexpr size_t kCleanupHostBelowFaces = 3000;

// --cleanup of the `integrate` program: the GPU pass from the crossover up, the host pass below it, or always with
// TSDF_HIP_HOST_MESH_POST=1 (A/B runs, tools/time_cleanup.py).  The result does not depend on the choice.
inline int cleanupMeshAuto(pcl::PolygonMesh &mesh, float face_dist = 0.02f, int min_neighbors = 5) {
  const char *host = std::getenv("TSDF_HIP_HOST_MESH_POST");
  if ((host && host[0] == '1') || mesh.polygons.size() <= kCleanupHostBelowFaces) {
    cleanupMesh(mesh, face_dist, min_neighbors);
    return 0;
  }
  return cleanupMeshGpu(mesh, face_dist, min_neighbors);
}

// Vertices up to which --flatten keeps the host pass: the largest prefix at which tools/time_flatten.py measured the
// GPU-backed pass (upload, device pass, download, this file's tail) slower than flattenVertices
// (profiles/flatten_timing.json, "gpu_backed_pass_loses_up_to_vertices": 30000 at 512^3 -- 7.6 ms against 2.6 ms; the next
// prefix, 90000, wins).
constexpr size_t kFlattenHostBelowVertices = 30000;

// --flatten of the `integrate` program: the GPU pass from the crossover up, the host pass below it, or always with
// TSDF_HIP_HOST_MESH_POST=1 (A/B runs, tools/time_flatten.py).  The result does not depend on the choice.
inline int flattenVerticesAuto(pcl::PolygonMesh &mesh, float min_dist = 0.0001f) {
  const char *host = std::getenv("TSDF_HIP_HOST_MESH_POST");
  if ((host && host[0] == '1') || (size_t)mesh.cloud.width * mesh.cloud.height <= kFlattenHostBelowVertices) {
    flattenVertices(mesh, min_dist);
    return 0;
  }
  return flattenVerticesGpu(mesh, min_dist);
}

// ---- decimateMesh: vertex clustering -------------------------------------------------------------------------------------------
struct Decimated {
  std::vector<std::uint32_t> remap;   // n: the output vertex of each input vertex
  std::vector<float> verts;           // m x 3
  std::vector<std::uint8_t> rgb;      // m x 3, or empty without colours
  std::vector<std::uint32_t> counts;  // m: members of each output vertex
  std::vector<std::uint32_t> faces;   // k x 3
  std::uint64_t duplicates = 0;       // faces dropped by the duplicate rule (the degenerate ones went before)
};

// The definition, as one sequential pass over the vertices in index order and one over the faces.
//   1. A finite vertex belongs to the cell floor((double)v / (double)cell_size) per axis (PointGrid::c); the vertices of one
//      cell are one cluster.  A vertex with a component that is not finite is a cluster of its own.  A cell index outside
//      [-2^20, 2^20) would alias under PointGrid::key's 21-bit masks: the call is refused and nothing is written.
//   2. Clusters are numbered by their lowest member: the first vertex of a new cell opens the next output vertex.
//   3. A cluster of one member keeps that vertex bit for bit.  Otherwise, per component, a double sum that starts at +0.0 takes
//      the members one add at a time in ascending index, is divided by (double)count and rounded to float once.  The order
//      is part of the definition: double addition is not associative, and the GPU pass performs exactly these adds.
//   4. The colour is the rounded integer mean per channel, (2 * sum + count) / (2 * count).
//   5. Faces go through remap; a face with two equal corners is dropped; of the remaining faces with the same three corners,
//      in whatever orientation, the one with the lowest index survives, as it is.  Face order is kept.
// xyz n x 3, rgb n x 3 or NULL, faces nf x 3 or NULL for a soup (face f = vertices 3f, 3f + 1, 3f + 2).  0, or
// TSDF_HIP_E_INVALID with the reason in *error.
inline int decimateArrays(const float *xyz, const std::uint8_t *rgb, size_t n, const std::uint32_t *faces, size_t nf, float cell_size,
                          Decimated &out, std::string *error = nullptr) {
  const auto refuse = [&](const std::string &why) {
    if (error) *error = why;
    return (int)TSDF_HIP_E_INVALID;
  };
  if (!(cell_size > 0.f) || !std::isfinite(cell_size)) return refuse("decimateMesh: cell_size must be finite and positive");
  if (n > ((size_t)1 << 31) || nf > ((size_t)1 << 31)) return refuse("decimateMesh: more than 2^31 vertices or faces");
  if (!faces && n / 3 < nf) return refuse("decimateMesh: a triangle soup needs 3 vertices per face");
  if (faces)
    for (size_t e = 0; e < 3 * nf; ++e)
      if (faces[e] >= n) return refuse("decimateMesh: a face names a vertex index >= n_verts");
  const double cell = (double)cell_size;
  std::vector<std::uint64_t> key(n);
  for (size_t i = 0; i < n; ++i) {
    key[i] = ~(std::uint64_t)0;  // not finite: in no cell
    if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2])) continue;
    std::uint64_t k = 0;
    for (int a = 0; a < 3; ++a) {
      const double c = std::floor((double)xyz[3 * i + a] / cell);
      if (!(c >= -1048576.0 && c < 1048576.0))
        return refuse("decimateMesh: a vertex lies outside the 2^21 cells per axis the cell key holds: |coordinate| must stay below 2^20 * "
                      "cell_size = " + std::to_string(1048576.0 * cell));
      k = (k << 21) | (std::uint64_t)((long)c & 0x1fffff);
    }
    key[i] = k;
  }
  struct Acc {
    double s[3];
    std::uint64_t c[3];
    std::uint32_t count, first;
  };
  std::vector<Acc> acc;
  std::unordered_map<std::uint64_t, std::uint32_t> cluster_of;
  out = Decimated();
  out.remap.resize(n);
  for (size_t i = 0; i < n; ++i) {
    std::uint32_t o = (std::uint32_t)acc.size();
    if (key[i] != ~(std::uint64_t)0) {
      const auto it = cluster_of.emplace(key[i], o);
      o = it.first->second;
    }
    if (o == acc.size()) acc.push_back(Acc{{0.0, 0.0, 0.0}, {0, 0, 0}, 0u, (std::uint32_t)i});
    Acc &a = acc[o];
    for (int k = 0; k < 3; ++k) {
      a.s[k] += (double)xyz[3 * i + k];
      if (rgb) a.c[k] += rgb[3 * i + k];
    }
    ++a.count;
    out.remap[i] = o;
  }
  const size_t m = acc.size();
  out.verts.resize(3 * m);
  out.counts.resize(m);
  if (rgb) out.rgb.resize(3 * m);
  for (size_t o = 0; o < m; ++o) {
    const Acc &a = acc[o];
    out.counts[o] = a.count;
    if (a.count == 1)
      std::memcpy(&out.verts[3 * o], xyz + 3 * (size_t)a.first, 3 * sizeof(float));
    else
      for (int k = 0; k < 3; ++k) out.verts[3 * o + k] = (float)(a.s[k] / (double)a.count);
    if (rgb)
      for (int k = 0; k < 3; ++k) out.rgb[3 * o + k] = (std::uint8_t)((2 * a.c[k] + a.count) / (2 * (std::uint64_t)a.count));
  }
  struct Triple {
    std::uint32_t v[3];
    bool operator==(const Triple &t) const { return v[0] == t.v[0] && v[1] == t.v[1] && v[2] == t.v[2]; }
  };
  struct TripleHash {
    size_t operator()(const Triple &t) const {
      std::uint64_t h = 0x9e3779b97f4a7c15ull;
      for (int k = 0; k < 3; ++k) h = (h ^ t.v[k]) * 0xff51afd7ed558ccdull, h ^= h >> 32;
      return (size_t)h;
    }
  };
  std::unordered_set<Triple, TripleHash> seen;
  for (size_t f = 0; f < nf; ++f) {
    std::uint32_t r[3];
    for (int k = 0; k < 3; ++k) r[k] = out.remap[faces ? faces[3 * f + k] : 3 * f + k];
    if (r[0] == r[1] || r[1] == r[2] || r[2] == r[0]) continue;
    Triple t{{r[0], r[1], r[2]}};
    if (t.v[0] > t.v[1]) std::swap(t.v[0], t.v[1]);
    if (t.v[1] > t.v[2]) std::swap(t.v[1], t.v[2]);
    if (t.v[0] > t.v[1]) std::swap(t.v[0], t.v[1]);
    if (!seen.insert(t).second) {
      ++out.duplicates;
      continue;
    }
    out.faces.insert(out.faces.end(), r, r + 3);
  }
  return 0;
}

inline bool hasColourField(const pcl::PolygonMesh &mesh) {
  for (const auto &f : mesh.cloud.fields)
    if (f.name == "rgb" || f.name == "rgba") return true;
  return false;
}

// positions and, when the cloud has an rgb field, colours (r, g, b) of the mesh's vertices
inline void vertexArrays(const pcl::PolygonMesh &mesh, std::vector<float> &xyz, std::vector<std::uint8_t> &rgb) {
  rgb.clear();
  if (!hasColourField(mesh)) {
    xyz = vertexPositions(mesh);
    return;
  }
  pcl::PointCloud<pcl::PointXYZRGB> v;
  pcl::fromPCLPointCloud2(mesh.cloud, v);
  xyz.resize(3 * v.points.size());
  rgb.resize(3 * v.points.size());
  for (size_t i = 0; i < v.points.size(); ++i) {
    xyz[3 * i] = v.points[i].x, xyz[3 * i + 1] = v.points[i].y, xyz[3 * i + 2] = v.points[i].z;
    rgb[3 * i] = v.points[i].r, rgb[3 * i + 1] = v.points[i].g, rgb[3 * i + 2] = v.points[i].b;
  }
}

// the tail both decimate passes share: the vertex blob (with an rgb field when colours came along) and the polygons
inline void storeDecimated(const std::vector<float> &xyz, const std::vector<std::uint8_t> &rgb, size_t m, const std::uint32_t *faces, size_t k,
                           pcl::PolygonMesh &mesh) {
  if (!rgb.empty()) {
    pcl::PointCloud<pcl::PointXYZRGB> out;
    for (size_t o = 0; o < m; ++o) {
      pcl::PointXYZRGB p;
      p.x = xyz[3 * o], p.y = xyz[3 * o + 1], p.z = xyz[3 * o + 2];
      p.r = rgb[3 * o], p.g = rgb[3 * o + 1], p.b = rgb[3 * o + 2];
      out.push_back(p);
    }
    pcl::toPCLPointCloud2(out, mesh.cloud);
  } else {
    pcl::PointCloud<pcl::PointXYZ> out;
    for (size_t o = 0; o < m; ++o) {
      pcl::PointXYZ p;
      p.x = xyz[3 * o], p.y = xyz[3 * o + 1], p.z = xyz[3 * o + 2];
      out.push_back(p);
    }
    pcl::toPCLPointCloud2(out, mesh.cloud);
  }
  mesh.polygons.resize(k);
  for (size_t f = 0; f < k; ++f) {
    mesh.polygons[f].vertices.resize(3);
    for (int j = 0; j < 3; ++j) mesh.polygons[f].vertices[j] = faces[3 * f + j];
  }
}

// false: a polygon is not a triangle (such a mesh is left alone by both decimate passes: the rules speak of triangles)
inline bool triangleIndices(const pcl::PolygonMesh &mesh, std::vector<std::uint32_t> &faces) {
  faces.resize(3 * mesh.polygons.size());
  for (size_t f = 0; f < mesh.polygons.size(); ++f) {
    if (mesh.polygons[f].vertices.size() != 3) return false;
    for (int k = 0; k < 3; ++k) faces[3 * f + k] = mesh.polygons[f].vertices[k];
  }
  return true;
}

// The host pass on a PolygonMesh; it keeps an rgb field when the cloud has one.  0, or TSDF_HIP_E_INVALID (the reason in
// *error) with the mesh untouched.
inline int decimateMesh(pcl::PolygonMesh &mesh, float cell_size, std::string *error = nullptr) {
  std::vector<float> xyz;
  std::vector<std::uint8_t> rgb;
  std::vector<std::uint32_t> faces;
  if (!triangleIndices(mesh, faces)) {
    if (error) *error = "decimateMesh: a polygon is not a triangle";
    return (int)TSDF_HIP_E_INVALID;
  }
  vertexArrays(mesh, xyz, rgb);
  Decimated d;
  const int rc = decimateArrays(xyz.data(), rgb.empty() ? nullptr : rgb.data(), xyz.size() / 3, faces.data(), faces.size() / 3, cell_size, d, error);
  if (rc) return rc;
  storeDecimated(d.verts, d.rgb, d.counts.size(), d.faces.data(), d.faces.size() / 3, mesh);
  return 0;
}

// The same result from the GPU (tsdf_hip_mesh_decimate, which reproduces the pass above bit for bit); the blob is built by
// the same tail.  0, or the library's error code (its text in tsdf_hip_last_error) with the mesh untouched.
inline int decimateMeshGpu(pcl::PolygonMesh &mesh, float cell_size, int device = 0) {
  std::vector<float> xyz;
  std::vector<std::uint8_t> rgb;
  std::vector<std::uint32_t> faces;
  if (!triangleIndices(mesh, faces)) return (int)TSDF_HIP_E_INVALID;
  vertexArrays(mesh, xyz, rgb);
  const size_t n = xyz.size() / 3, nf = faces.size() / 3;
  std::vector<float> out_xyz(3 * n);
  std::vector<std::uint8_t> out_rgb(rgb.empty() ? 0 : 3 * n);
  std::uint64_t m = 0, k = 0;
  // (the re-indexed faces come back in place of the ones handed over: the library has read those before it writes)
  const int rc = tsdf_hip_mesh_decimate(device, xyz.data(), rgb.empty() ? nullptr : rgb.data(), n, faces.data(), nf, cell_size, nullptr,
                                        out_xyz.data(), rgb.empty() ? nullptr : out_rgb.data(), nullptr, &m, faces.data(), &k);
  if (rc) return rc;
  if (!rgb.empty()) out_rgb.resize(3 * (size_t)m);
  storeDecimated(out_xyz, out_rgb, (size_t)m, faces.data(), (size_t)k, mesh);
  return 0;
}

// Vertices up to which --decimate keeps the host pass: the largest prefix at which tools/time_decimate.py measured the
// GPU-backed pass (upload, device pass, download, this file's tail) slower than decimateMesh
// (profiles/decimate_timing.json, "gpu_backed_pass_loses_up_to_vertices": 300000 at 512^3 with a cell of 2 voxels -- 11.4 ms
// against 9.4 ms; the next prefix, 3000000, wins with 58.9 ms against 124.8 ms).
constexpr size_t kDecimateHostBelowVertices = 300000;

// --decimate of the programs: the GPU pass from the crossover up, the host pass below it, or always with
// TSDF_HIP_HOST_MESH_POST=1 (A/B runs, tools/time_decimate.py).  The result does not depend on the choice.
inline int decimateMeshAuto(pcl::PolygonMesh &mesh, float cell_size, std::string *error = nullptr) {
  const char *host = std::getenv("TSDF_HIP_HOST_MESH_POST");
  if ((host && host[0] == '1') || (size_t)mesh.cloud.width * mesh.cloud.height <= kDecimateHostBelowVertices) return decimateMesh(mesh, cell_size, error);
  const int rc = decimateMeshGpu(mesh, cell_size);
  if (rc && error) *error = tsdf_hip_last_error();
  return rc;
}

// ---- smoothMesh: Taubin's lambda | mu -------------------------------------------------------------------------------------------
struct Smoothed {
  std::vector<float> verts;           // n x 3
  std::vector<std::uint8_t> fixed;    // n: rule 3's bits
  std::vector<std::uint32_t> degree;  // n
  std::uint64_t edges = 0;            // unique undirected edges
};

// The definition (umbrella operator, uniform weights, Jacobi steps), as one sequential pass.
//   1. N(i) is the set of j != i such that some face has both i and j among its corners, ordered by ascending index;
//      deg(i) = |N(i)|.  A degenerate face (a, a, b) still contributes a-b; duplicate faces contribute once.
//   2. The multiplicity of the undirected edge {a, b}, a != b, is the number of corner pairs (0,1), (1,2), (2,0) of all faces
//      that name it; a BOUNDARY edge has multiplicity exactly 1.
//   3. fixed[i], decided once from the input positions, is the OR of 1 (a component of i or of some j in N(i) is not finite),
//      2 (deg(i) == 0) and 4 (keep_boundary != 0 and i is an endpoint of a boundary edge).  A fixed vertex keeps its three
//      words bit for bit through every step.
//   4. One step with factor f, the float widened to double, every vertex reading the positions of the step before: per
//      component s = +0.0; for j in N(i) ascending s += (double)x_j; m = s / (double)deg(i); p = (double)x_i;
//      x'_i = (float)(p + f * (m - p)).  Each operation is rounded once (the programs are built with -ffp-contract=off), and the
//      order of the adds is part of the definition: the GPU pass performs exactly these.
//   5. One iteration is a step with lambda and then, iff mu != 0, a step with mu.  iterations == 0 returns the input.
// xyz n x 3, faces nf x 3 (required: a soup shares no vertices).  0, or TSDF_HIP_E_INVALID with the reason in *error and `out`
// untouched.
inline int smoothArrays(const float *xyz, size_t n, const std::uint32_t *faces, size_t nf, float lambda, float mu, int iterations, int keep_boundary,
                        Smoothed &out, std::string *error = nullptr) {
  const auto refuse = [&](const std::string &why) {
    if (error) *error = why;
    return (int)TSDF_HIP_E_INVALID;
  };
  if (!std::isfinite(lambda) || !(lambda > 0.f && lambda <= 1.f)) return refuse("smoothMesh: lambda must be finite and in (0, 1]");
  if (!std::isfinite(mu) || !(mu >= -1.f && mu <= 0.f)) return refuse("smoothMesh: mu must be finite and in [-1, 0]");
  if (iterations < 0 || iterations > 1000) return refuse("smoothMesh: iterations must be in [0, 1000]");
  if (n > ((size_t)1 << 31) || nf > ((size_t)1 << 31)) return refuse("smoothMesh: more than 2^31 vertices or faces");
  if (!faces && (n || nf)) return refuse("smoothMesh: a triangle soup shares no vertices, so it has no neighbours to smooth with: flatten or decimate first");
  if (n && !xyz) return refuse("smoothMesh: verts must not be NULL");
  for (size_t e = 0; e < 3 * nf; ++e)
    if (faces[e] >= n) return refuse("smoothMesh: a face names a vertex index >= n_verts");
  // rules 1 and 2: every corner pair in both directions; after sorting, a run of equal (a, b) is as long as the multiplicity
  std::vector<std::uint64_t> key;
  key.reserve(6 * nf);
  for (size_t f = 0; f < nf; ++f)
    for (int k = 0; k < 3; ++k) {
      const std::uint64_t a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3];
      if (a == b) continue;
      key.push_back(a << 32 | b);
      key.push_back(b << 32 | a);
    }
  std::sort(key.begin(), key.end());
  std::vector<std::uint32_t> row(n + 1, 0), col;
  std::vector<char> boundary(n, 0);
  for (size_t i = 0; i < key.size();) {
    size_t j = i + 1;
    while (j < key.size() && key[j] == key[i]) ++j;
    const std::uint32_t a = (std::uint32_t)(key[i] >> 32);
    if (j - i == 1) boundary[a] = 1;
    ++row[a + 1];
    col.push_back((std::uint32_t)key[i]);
    i = j;
  }
  for (size_t i = 0; i < n; ++i) row[i + 1] += row[i];
  const auto finite = [&](size_t i) { return std::isfinite(xyz[3 * i]) && std::isfinite(xyz[3 * i + 1]) && std::isfinite(xyz[3 * i + 2]); };
  Smoothed r;
  r.edges = col.size() / 2;
  r.fixed.resize(n);
  r.degree.resize(n);
  for (size_t i = 0; i < n; ++i) {
    bool fin = finite(i);
    for (std::uint32_t e = row[i]; e < row[i + 1] && fin; ++e) fin = finite(col[e]);
    r.degree[i] = row[i + 1] - row[i];
    r.fixed[i] = (std::uint8_t)((fin ? 0 : 1) | (r.degree[i] == 0 ? 2 : 0) | (keep_boundary && boundary[i] ? 4 : 0));
  }
  r.verts.assign(xyz, xyz + 3 * n);
  std::vector<float> next(3 * n);
  for (int it = 0; it < iterations; ++it)
    for (int half = 0; half < (mu != 0.f ? 2 : 1); ++half) {
      const double f = (double)(half ? mu : lambda);
      for (size_t i = 0; i < n; ++i) {
        if (r.fixed[i]) {
          std::memcpy(&next[3 * i], &r.verts[3 * i], 3 * sizeof(float));
          continue;
        }
        for (int c = 0; c < 3; ++c) {
          double s = 0.0;
          for (std::uint32_t e = row[i]; e < row[i + 1]; ++e) s += (double)r.verts[3 * (size_t)col[e] + c];
          const double m = s / (double)r.degree[i], p = (double)r.verts[3 * i + c];
          next[3 * i + c] = (float)(p + f * (m - p));
        }
      }
      r.verts.swap(next);
    }
  out = std::move(r);
  return 0;
}

// the offsets of the x, y, z fields (FLOAT32) in the cloud blob; false: the cloud has no such fields
inline bool positionOffsets(const pcl::PolygonMesh &mesh, std::uint32_t off[3]) {
  int found = 0;
  for (const auto &f : mesh.cloud.fields)
    for (int k = 0; k < 3; ++k)
      if (f.name == std::string(1, "xyz"[k]) && f.datatype == pcl::PCLPointField::FLOAT32) off[k] = f.offset, found |= 1 << k;
  return found == 7;
}

// both smooth passes on a PolygonMesh: the positions out of the blob, pass(xyz, faces, out), and the x, y, z fields of the blob
// rewritten -- every other field (rgb) survives.  A polygon that is not a triangle refuses the mesh.
template <typename Pass>
inline int smoothBlob(pcl::PolygonMesh &mesh, std::string *error, Pass pass) {
  std::vector<std::uint32_t> faces;
  std::uint32_t off[3];
  const size_t n = (size_t)mesh.cloud.width * mesh.cloud.height, step = mesh.cloud.point_step;
  if (!triangleIndices(mesh, faces) || (n && !positionOffsets(mesh, off))) {
    if (error) *error = "smoothMesh: a polygon is not a triangle, or the cloud has no float x, y, z fields";
    return (int)TSDF_HIP_E_INVALID;
  }
  std::vector<float> xyz(3 * n), out;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) std::memcpy(&xyz[3 * i + k], mesh.cloud.data.data() + i * step + off[k], 4);
  const int rc = pass(xyz, faces, out);
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) std::memcpy(mesh.cloud.data.data() + i * step + off[k], &out[3 * i + k], 4);
  return 0;
}

// The host pass on a PolygonMesh.  0, or TSDF_HIP_E_INVALID (the reason in *error) with the mesh untouched.
inline int smoothMesh(pcl::PolygonMesh &mesh, int iterations, float lambda = 0.5f, float mu = -0.53f, bool keep_boundary = true,
                      std::string *error = nullptr) {
  return smoothBlob(mesh, error, [&](const std::vector<float> &xyz, const std::vector<std::uint32_t> &faces, std::vector<float> &out) {
    Smoothed s;
    // (an empty vector's data() may be NULL: an empty mesh is not a soup)
    static const std::uint32_t none[3] = {0, 0, 0};
    const int rc = smoothArrays(xyz.data(), xyz.size() / 3, faces.empty() ? none : faces.data(), faces.size() / 3, lambda, mu, iterations,
                                keep_boundary ? 1 : 0, s, error);
    out.swap(s.verts);
    return rc;
  });
}

// The same result from the GPU (tsdf_hip_mesh_smooth, which reproduces the pass above bit for bit).  0, or the library's
// error code (its text in tsdf_hip_last_error, or in *error for what this function refuses itself) with the mesh untouched.
inline int smoothMeshGpu(pcl::PolygonMesh &mesh, int iterations, float lambda = 0.5f, float mu = -0.53f, bool keep_boundary = true, int device = 0,
                         std::string *error = nullptr) {
  bool own = false;  // the refusal is smoothBlob's own, not the library's
  std::string why;
  const int rc = smoothBlob(mesh, &why, [&](const std::vector<float> &xyz, const std::vector<std::uint32_t> &faces, std::vector<float> &out) {
    own = true;
    static const std::uint32_t none[3] = {0, 0, 0};
    out.resize(xyz.size());
    return tsdf_hip_mesh_smooth(device, xyz.data(), xyz.size() / 3, faces.empty() ? none : faces.data(), faces.size() / 3, lambda, mu, iterations,
                                keep_boundary ? 1 : 0, out.data(), nullptr, nullptr);
  });
  if (rc && error) *error = own ? std::string(tsdf_hip_last_error()) : why;
  return rc;
}

// Vertices up to which --smooth keeps the host pass: the largest prefix at which tools/time_smooth.py measured the GPU-backed
// pass (upload, device pass, download) slower than smoothMesh (profiles/smooth_timing.json,
// "gpu_backed_pass_loses_up_to_vertices": 10000 at 512^3 and 10 iterations -- 5.9 ms against 4.8 ms; the next prefix, 30000,
// wins with 6.5 ms against 15.9 ms).
constexpr size_t kSmoothHostBelowVertices = 10000;

// --smooth of the programs: the GPU pass from the crossover up, the host pass below it, or always with
// TSDF_HIP_HOST_MESH_POST=1 (A/B runs, tools/time_smooth.py).  The result does not depend on the choice.
inline int smoothMeshAuto(pcl::PolygonMesh &mesh, int iterations, float lambda = 0.5f, float mu = -0.53f, bool keep_boundary = true,
                          std::string *error = nullptr) {
  const char *host = std::getenv("TSDF_HIP_HOST_MESH_POST");
  if ((host && host[0] == '1') || (size_t)mesh.cloud.width * mesh.cloud.height <= kSmoothHostBelowVertices)
    return smoothMesh(mesh, iterations, lambda, mu, keep_boundary, error);
  return smoothMeshGpu(mesh, iterations, lambda, mu, keep_boundary, 0, error);
}

// --smooth of the programs, applied last.  still_soup: neither --flatten nor --decimate has run, so no two faces share a vertex
// yet: flattenVerticesAuto at its default distance comes first.  0, or the error code with its text in *error.
inline int smoothProgramMesh(pcl::PolygonMesh &mesh, bool still_soup, int iterations, float lambda, float mu, std::string *error) {
  if (still_soup)
    if (const int rc = flattenVerticesAuto(mesh)) {
      if (error) *error = tsdf_hip_last_error();
      return rc;
    }
  return smoothMeshAuto(mesh, iterations, lambda, mu, true, error);
}

// ---- meshNormals: area-weighted vertex normals ---------------------------------------------------------------------------------
struct Normals {
  std::vector<float> normals;       // n x 3
  std::vector<std::uint8_t> flags;  // n: rule 4's bits
  std::uint64_t skipped = 0;        // faces with a coordinate that is not finite
  std::uint64_t zero = 0;           // vertices whose normal is zero
};

// The definition, as one sequential pass over the faces in index order and one over the vertices.
//   1. The face vector of f = (a, b, c): e1 = (double)p_b - (double)p_a, e2 = (double)p_c - (double)p_a componentwise,
//      g_f = (e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x); every difference, product and subtraction is
//      rounded once (the programs are built with -ffp-contract=off: a contracted fma(e1y, e2z, -(e1z * e2y)) would make the
//      zero vector of a face with two corners at one position nonzero).  |g_f| is twice the area.  A face with a coordinate
//      that is not finite at any corner is skipped: it adds nothing and is counted.
//   2. Per component s_i = +0.0; over the faces that name i in ascending face index, s_i += g_f once per corner that names i.
//      The order of the adds is part of the definition: the GPU pass performs exactly these.
//   3. l2 = (sx * sx + sy * sy) + sz * sz, l = sqrt(l2); l2 == 0: three +0.0f; else ((float)(sx / l), (float)(sy / l),
//      (float)(sz / l)), by division.
//   4. flags[i] = 1 (no face names i) | 2 (rule 3 wrote zero) | 4 (a face that names i was skipped).
//   5. Orientation: the normal points to the side from which a -> b -> c appear counter-clockwise, along
//      (p_b - p_a) x (p_c - p_a); on a marched mesh that is out of the surface, into observed free space.
// xyz n x 3, faces nf x 3 or NULL for a soup (n a multiple of 3, face f = vertices 3f, 3f + 1, 3f + 2, nf = n / 3 or 0).  0, or
// TSDF_HIP_E_INVALID with the reason in *error and `out` untouched.
inline int normalArrays(const float *xyz, size_t n, const std::uint32_t *faces, size_t nf, Normals &out, std::string *error = nullptr) {
  const auto refuse = [&](const std::string &why) {
    if (error) *error = why;
    return (int)TSDF_HIP_E_INVALID;
  };
  if (n > ((size_t)1 << 31) || nf > (size_t)1431655765) return refuse("meshNormals: more than 2^31 vertices or 1431655765 faces");
  if (n && !xyz) return refuse("meshNormals: verts must not be NULL");
  if (!faces && (n % 3 || (nf && nf != n / 3)))
    return refuse("meshNormals: a triangle soup has 3 vertices per face: n_verts must be a multiple of 3 and n_faces 0 or n_verts / 3");
  if (faces)
    for (size_t e = 0; e < 3 * nf; ++e)
      if (faces[e] >= n) return refuse("meshNormals: a face names a vertex index >= n_verts");
  Normals r;
  r.normals.assign(3 * n, 0.f);
  r.flags.assign(n, 0);
  std::vector<double> s(3 * n, 0.0);
  std::vector<char> named(n, 0);
  for (size_t f = 0; f < nf; ++f) {
    size_t v[3];
    for (int k = 0; k < 3; ++k) v[k] = faces ? faces[3 * f + k] : 3 * f + k;
    const float *a = xyz + 3 * v[0], *b = xyz + 3 * v[1], *c = xyz + 3 * v[2];
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(a[k]) && std::isfinite(b[k]) && std::isfinite(c[k]);
    double g[3] = {0.0, 0.0, 0.0};
    if (fin) {
      const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
      const double e2x = (double)c[0] - (double)a[0], e2y = (double)c[1] - (double)a[1], e2z = (double)c[2] - (double)a[2];
      g[0] = e1y * e2z - e1z * e2y;
      g[1] = e1z * e2x - e1x * e2z;
      g[2] = e1x * e2y - e1y * e2x;
    } else {
      ++r.skipped;
    }
    for (int k = 0; k < 3; ++k) {
      named[v[k]] = 1;
      if (!fin) {
        r.flags[v[k]] |= 4;
        continue;
      }
      for (int j = 0; j < 3; ++j) s[3 * v[k] + j] += g[j];
    }
  }
  for (size_t i = 0; i < n; ++i) {
    const double sx = s[3 * i], sy = s[3 * i + 1], sz = s[3 * i + 2];
    const double l2 = (sx * sx + sy * sy) + sz * sz;
    if (!named[i]) r.flags[i] |= 1;
    if (l2 == 0.0) {
      r.flags[i] |= 2;
      ++r.zero;
      continue;
    }
    const double l = std::sqrt(l2);
    r.normals[3 * i] = (float)(sx / l), r.normals[3 * i + 1] = (float)(sy / l), r.normals[3 * i + 2] = (float)(sz / l);
  }
  out = std::move(r);
  return 0;
}

// the offsets of the FLOAT32 fields normal_x, normal_y, normal_z in the cloud blob; false: the cloud does not have all three
inline bool normalOffsets(const pcl::PolygonMesh &mesh, std::uint32_t off[3]) {
  int found = 0;
  for (const auto &f : mesh.cloud.fields)
    for (int k = 0; k < 3; ++k)
      if (f.name == std::string("normal_") + "xyz"[k] && f.datatype == pcl::PCLPointField::FLOAT32) off[k] = f.offset, found |= 1 << k;
  return found == 7;
}

// both normal passes on a PolygonMesh: the positions out of the blob, pass(xyz, faces or NULL for a soup, n_faces, out), and
// three FLOAT32 fields normal_x, normal_y, normal_z APPENDED to the blob after the fields it has (rewritten if they are
// there already); every other field and the polygons stay.  A mesh whose polygon f is (3f, 3f + 1, 3f + 2) throughout is
// handed over as a soup: the result is the same and the GPU pass needs no sort.  A polygon that is not a triangle refuses
// the mesh.
template <typename Pass>
inline int normalsBlob(pcl::PolygonMesh &mesh, std::string *error, Pass pass) {
  std::vector<std::uint32_t> faces;
  std::uint32_t off[3];
  const size_t n = (size_t)mesh.cloud.width * mesh.cloud.height, step = mesh.cloud.point_step;
  if (!triangleIndices(mesh, faces) || (n && !positionOffsets(mesh, off))) {
    if (error) *error = "meshNormals: a polygon is not a triangle, or the cloud has no float x, y, z fields";
    return (int)TSDF_HIP_E_INVALID;
  }
  const size_t nf = faces.size() / 3;
  bool soup = nf && n == 3 * nf;
  for (size_t e = 0; e < faces.size() && soup; ++e) soup = faces[e] == e;
  std::vector<float> xyz(3 * n), out;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) std::memcpy(&xyz[3 * i + k], mesh.cloud.data.data() + i * step + off[k], 4);
  static const std::uint32_t none[3] = {0, 0, 0};  // (an empty vector's data() may be NULL: a mesh without faces is no soup)
  const int rc = pass(xyz, soup ? nullptr : (nf ? faces.data() : none), nf, out);
  if (rc) return rc;
  std::uint32_t at[3];
  if (!normalOffsets(mesh, at)) {
    const size_t wide = step + 12;
    std::vector<std::uint8_t> data(n * wide);
    for (size_t i = 0; i < n; ++i) std::memcpy(data.data() + i * wide, mesh.cloud.data.data() + i * step, step);
    mesh.cloud.data.swap(data);
    for (int k = 0; k < 3; ++k) {
      pcl::PCLPointField f;
      f.name = std::string("normal_") + "xyz"[k];
      f.offset = at[k] = (std::uint32_t)(step + 4 * k);
      f.datatype = pcl::PCLPointField::FLOAT32;
      f.count = 1;
      mesh.cloud.fields.push_back(f);
    }
    mesh.cloud.point_step = (std::uint32_t)wide;
    mesh.cloud.row_step = (std::uint32_t)(wide * mesh.cloud.width);
  }
  const size_t now = mesh.cloud.point_step;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) std::memcpy(mesh.cloud.data.data() + i * now + at[k], &out[3 * i + k], 4);
  return 0;
}

// The host pass on a PolygonMesh.  0, or TSDF_HIP_E_INVALID (the reason in *error) with the mesh untouched.
inline int meshNormals(pcl::PolygonMesh &mesh, std::string *error = nullptr) {
  return normalsBlob(mesh, error, [&](const std::vector<float> &xyz, const std::uint32_t *faces, size_t nf, std::vector<float> &out) {
    Normals r;
    const int rc = normalArrays(xyz.data(), xyz.size() / 3, faces, nf, r, error);
    out.swap(r.normals);
    return rc;
  });
}

// The same result from the GPU (tsdf_hip_mesh_normals, which reproduces the pass above word for word).  0, or the library's
// error code (its text in tsdf_hip_last_error, or in *error for what this function refuses itself) with the mesh untouched.
inline int meshNormalsGpu(pcl::PolygonMesh &mesh, int device = 0, std::string *error = nullptr) {
  bool own = false;  // the refusal is normalsBlob's own, not the library's
  std::string why;
  const int rc = normalsBlob(mesh, &why, [&](const std::vector<float> &xyz, const std::uint32_t *faces, size_t nf, std::vector<float> &out) {
    own = true;
    out.resize(xyz.size());
    return tsdf_hip_mesh_normals(device, xyz.data(), xyz.size() / 3, faces, nf, out.data(), nullptr);
  });
  if (rc && error) *error = own ? std::string(tsdf_hip_last_error()) : why;
  return rc;
}

// Vertices up to which --normals keeps the host pass: the largest prefix at which tools/time_normals.py measured the
// GPU-backed pass (upload, device pass, download) slower than meshNormals (profiles/normals_timing.json,
// "gpu_backed_pass_loses_up_to_vertices": 300000 at 512^3 -- 11.4 ms against 7.8 ms; the full mesh, 946378 vertices, wins with
// 22.4 ms against 35.5 ms).  The host pass is one cheap loop: the device pass itself takes 0.5 ms there, and
// the transfers and allocations around it decide.
constexpr size_t kNormalsHostBelowVertices = 300000;

// --normals of the programs: the GPU pass from the crossover up, the host pass below it, or always with
// TSDF_HIP_HOST_MESH_POST=1 (A/B runs, tools/time_normals.py).  The result does not depend on the choice.
inline int meshNormalsAuto(pcl::PolygonMesh &mesh, std::string *error = nullptr) {
  const char *host = std::getenv("TSDF_HIP_HOST_MESH_POST");
  if ((host && host[0] == '1') || (size_t)mesh.cloud.width * mesh.cloud.height <= kNormalsHostBelowVertices) return meshNormals(mesh, error);
  return meshNormalsGpu(mesh, 0, error);
}

}  // namespace mesh_post
}  // namespace cpu_tsdf
