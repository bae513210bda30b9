// Host shell of the MI355X drop-in: cpu_tsdf::MarchingCubesTSDFOctree on top of the C ABI.
// Mirrors performReconstruction of the reference (src/lib/marching_cubes_tsdf_octree.cpp:108-143): build
// the vertex cloud (3 vertices per triangle, no sharing), move it by the volume's global transform,
// pack it into the PolygonMesh blob, polygons = {3i, 3i+1, 3i+2}.  With setFlatten (an extension) the vertex cloud and the
// polygons are the indexed mesh of tsdf_hip_march_flatten instead, with setDecimate that of tsdf_hip_march_decimate; setSmooth
// moves that mesh's vertices (tsdf_hip_march_smooth) before they are fetched.
#include <cpu_tsdf/marching_cubes_tsdf_octree.h>
#include <pcl/common/transforms.h>
#include <pcl/console/print.h>
#include <pcl/conversions.h>

#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace cpu_tsdf {

// setInputTSDF (reference: src/lib/marching_cubes_tsdf_octree.cpp:44-83) leaves the pcl::MarchingCubes base in the
// state the reference leaves it in, so that code reading it back (getGridResolution, getIsoLevel, the input cloud's
// bounding box) sees the same values.  What that state IS: the "input cloud" is the eight corners of the box spanned by
// the centres of voxel (0, 0, 0) and of voxel (res_x, res_y, res_z) -- the reference adds a half-voxel offset to each
// centre and subtracts the same number again (:64-66), which leaves the centres themselves; getVoxelCenter is separable
// per axis, so the eight points are the combinations of those two -- no grid extension, iso level 0, and size_voxel_
// the box divided by the resolution.  The kernels derive the same lower boundary / voxel size from the volume's
// parameters (tsdf_march.hip).
void MarchingCubesTSDFOctree::setInputTSDF(TSDFVolumeOctree::ConstPtr tsdf_volume) {
  tsdf_volume_ = tsdf_volume;
  if (!tsdf_volume_) return;
  int res[3];
  tsdf_volume_->getResolution(res[0], res[1], res[2]);
  setGridResolution(res[0], res[1], res[2]);
  const pcl::PointXYZ first = tsdf_volume_->getVoxelCenter(0, 0, 0);
  const pcl::PointXYZ beyond = tsdf_volume_->getVoxelCenter(res[0], res[1], res[2]);
  pcl::PointCloud<pcl::PointXYZ>::Ptr corners(new pcl::PointCloud<pcl::PointXYZ>);
  for (int c = 0; c < 8; ++c)  // x slowest, z fastest, like the reference's three loops
    corners->points.push_back(pcl::PointXYZ((c & 4) ? beyond.x : first.x, (c & 2) ? beyond.y : first.y, (c & 1) ? beyond.z : first.z));
  corners->width = (uint32_t)corners->points.size();
  corners->height = 1;
  setInputCloud(corners);
  setPercentageExtendGrid(0);
  setIsoLevel(0.f);
  getBoundingBox();
  size_voxel_ = (upper_boundary_ - lower_boundary_) * Eigen::Array3f(res_x_, res_y_, res_z_).inverse();
}

// setCleanup's arguments per object (the header says why they are not members).  cleanup_of: false = no cleanup asked for.
struct CleanupArgs {
  float face_dist;
  int min_neighbors;
};
static std::mutex g_cleanup_mutex;
static std::map<const MarchingCubesTSDFOctree *, CleanupArgs> g_cleanup;

void MarchingCubesTSDFOctree::setCleanup(float face_dist, int min_neighbors) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_cleanup[this] = CleanupArgs{face_dist, min_neighbors};
}

void MarchingCubesTSDFOctree::clearCleanup() {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_cleanup.erase(this);
}

// setFlatten's argument per object, kept like setCleanup's
static std::map<const MarchingCubesTSDFOctree *, float> g_flatten;

void MarchingCubesTSDFOctree::setFlatten(float min_dist) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_flatten[this] = min_dist;
}

void MarchingCubesTSDFOctree::clearFlatten() {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_flatten.erase(this);
}

// setDecimate's argument per object, kept likewise
static std::map<const MarchingCubesTSDFOctree *, float> g_decimate;

void MarchingCubesTSDFOctree::setDecimate(float cell_size) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_decimate[this] = cell_size;
}

void MarchingCubesTSDFOctree::clearDecimate() {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_decimate.erase(this);
}

// setSmooth's arguments per object, kept likewise
struct SmoothArgs {
  int iterations;
  float lambda, mu;
  bool keep_boundary;
};
static std::map<const MarchingCubesTSDFOctree *, SmoothArgs> g_smooth;

void MarchingCubesTSDFOctree::setSmooth(int iterations, float lambda, float mu, bool keep_boundary) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_smooth[this] = SmoothArgs{iterations, lambda, mu, keep_boundary};
}

void MarchingCubesTSDFOctree::clearSmooth() {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  g_smooth.erase(this);
}

// setNormals' argument per object, kept likewise: the objects that asked for normals
static std::set<const MarchingCubesTSDFOctree *> g_normals;

void MarchingCubesTSDFOctree::setNormals(bool on) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  if (on)
    g_normals.insert(this);
  else
    g_normals.erase(this);
}

static bool normals_of(const MarchingCubesTSDFOctree *mc) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  return g_normals.count(mc) != 0;
}

MarchingCubesTSDFOctree::~MarchingCubesTSDFOctree() {
  clearCleanup();
  clearFlatten();
  clearDecimate();
  clearSmooth();
  setNormals(false);
}

static bool smooth_of(const MarchingCubesTSDFOctree *mc, SmoothArgs &out) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  const auto it = g_smooth.find(mc);
  if (it == g_smooth.end()) return false;
  out = it->second;
  return true;
}

static bool decimate_of(const MarchingCubesTSDFOctree *mc, float &out) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  const auto it = g_decimate.find(mc);
  if (it == g_decimate.end()) return false;
  out = it->second;
  return true;
}

static bool flatten_of(const MarchingCubesTSDFOctree *mc, float &out) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  const auto it = g_flatten.find(mc);
  if (it == g_flatten.end()) return false;
  out = it->second;
  return true;
}

static bool cleanup_of(const MarchingCubesTSDFOctree *mc, CleanupArgs &out) {
  std::lock_guard<std::mutex> lock(g_cleanup_mutex);
  const auto it = g_cleanup.find(mc);
  if (it == g_cleanup.end()) return false;
  out = it->second;
  return true;
}

// cleanup: NULL, or the arguments of setCleanup -- tsdf_hip_march_cleanup between the march and the fetch.  flatten: NULL,
// or setFlatten's min_dist -- tsdf_hip_march_flatten after that, and the INDEXED mesh is fetched: `indexed` is set and
// `faces` holds its polygons (otherwise the soup: polygon i = {3i, 3i + 1, 3i + 2}).  decimate: NULL, or setDecimate's
// cell_size -- tsdf_hip_march_decimate in flatten's place (with both set, flatten is skipped), fetched the same way.  smooth:
// NULL, or the arguments of setSmooth -- tsdf_hip_march_smooth last, on the indexed mesh; with neither flatten nor decimate,
// flatten runs first at its default min_dist.  normals: NULL, or where setNormals' normals go -- tsdf_hip_march_normals last of
// all, on the mesh that is fetched (the indexed one, or the soup), one row per vertex.
static bool run_march(const TSDFVolumeOctree::ConstPtr &vol, float w_min, int mode, const CleanupArgs *cleanup, const float *flatten, const float *decimate,
                      const SmoothArgs *smooth, std::vector<float> *normals, std::vector<float> &verts, std::vector<unsigned char> &rgb, std::vector<uint32_t> &faces, bool &indexed) {
  verts.clear();
  rgb.clear();
  faces.clear();
  indexed = false;
  if (normals) normals->clear();
  if (!vol || !vol->handle()) {
    PCL_ERROR("[cpu_tsdf::MarchingCubesTSDFOctree::reconstruct] no TSDF volume set (or reset() not called)\n");
    return false;
  }
  if (!vol->cubicForQueries("MarchingCubesTSDFOctree::reconstruct")) return false;
  uint64_t n_tri = 0;
  int rc = tsdf_hip_march(vol->handle(), w_min, mode, &n_tri);
  if (rc == 0 && cleanup) rc = tsdf_hip_march_cleanup(vol->handle(), cleanup->face_dist, cleanup->min_neighbors, &n_tri);
  if (rc == 0 && (flatten || decimate || smooth)) {
    uint64_t n_verts = 0, n_faces = 0;
    rc = decimate ? tsdf_hip_march_decimate(vol->handle(), *decimate, &n_verts, &n_faces)
                  : tsdf_hip_march_flatten(vol->handle(), flatten ? *flatten : 0.0001f, &n_verts, &n_faces);
    if (rc == 0 && smooth)
      rc = tsdf_hip_march_smooth(vol->handle(), smooth->lambda, smooth->mu, smooth->iterations, smooth->keep_boundary ? 1 : 0, nullptr);
    if (rc == 0) {
      indexed = true;
      verts.resize((size_t)n_verts * 3);
      if (mode) rgb.resize((size_t)n_verts * 3);
      faces.resize((size_t)n_faces * 3);
      if (n_verts) rc = tsdf_hip_march_fetch_indexed(vol->handle(), verts.data(), mode ? rgb.data() : nullptr, faces.data(), nullptr);
    }
  } else if (rc == 0 && n_tri) {
    verts.resize((size_t)n_tri * 9);
    if (mode) rgb.resize((size_t)n_tri * 9);
    rc = tsdf_hip_march_fetch(vol->handle(), verts.data(), mode ? rgb.data() : nullptr, nullptr);
  }
  if (rc == 0 && normals) {
    uint64_t n_verts = 0;
    rc = tsdf_hip_march_normals(vol->handle(), &n_verts, nullptr);
    if (rc == 0 && n_verts * 3 != verts.size()) {
      PCL_ERROR("[cpu_tsdf::MarchingCubesTSDFOctree::reconstruct] the normals describe %llu vertices, the mesh has %llu\n",
                (unsigned long long)n_verts, (unsigned long long)(verts.size() / 3));
      rc = TSDF_HIP_E_INVALID;
    }
    normals->resize(verts.size());
    if (rc == 0 && n_verts) rc = tsdf_hip_march_fetch_normals(vol->handle(), normals->data());
  }
  if (rc) {
    PCL_ERROR("[cpu_tsdf::MarchingCubesTSDFOctree::reconstruct] %s: %s\n", tsdf_hip_error_string(rc),
              tsdf_hip_last_error());
    verts.clear();
    rgb.clear();
    faces.clear();
    indexed = false;
    if (normals) normals->clear();
    return false;
  }
  return true;
}

static void fill_polygons(size_t n_vertices, bool indexed, const std::vector<uint32_t> &faces, std::vector<pcl::Vertices> &polygons) {
  polygons.resize(indexed ? faces.size() / 3 : n_vertices / 3);
  for (size_t i = 0; i < polygons.size(); ++i) {
    pcl::Vertices v;
    v.vertices.resize(3);
    for (int j = 0; j < 3; ++j) v.vertices[j] = indexed ? faces[3 * i + j] : static_cast<int>(i) * 3 + j;
    polygons[i] = v;
  }
}

// setNormals: three FLOAT32 fields normal_x, normal_y, normal_z appended to the blob, after the fields it has.  The normals are
// those of the mesh in the VOLUME frame (tsdf_hip_march_normals) word for word while the global transform's linear part is the
// identity; otherwise they are turned by it like the vertices (a rotation: the global transform is rigid).
static void append_normals(const std::vector<float> &normals, const Eigen::Affine3d &g, pcl::PCLPointCloud2 &cloud) {
  const size_t n = normals.size() / 3, step = cloud.point_step, wide = step + 12;
  const Eigen::Matrix4d m = g.matrix();
  bool identity = true;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) identity = identity && m(r, c) == (r == c ? 1.0 : 0.0);
  std::vector<std::uint8_t> data(n * wide);
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(data.data() + i * wide, cloud.data.data() + i * step, step);
    float v[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    if (!identity) {
      const double x = v[0], y = v[1], z = v[2];
      for (int r = 0; r < 3; ++r) v[r] = static_cast<float>(x * m(r, 0) + (y * m(r, 1) + z * m(r, 2)));
    }
    std::memcpy(data.data() + i * wide + step, v, 12);
  }
  cloud.data.swap(data);
  for (int k = 0; k < 3; ++k) {
    pcl::PCLPointField f;
    f.name = std::string("normal_") + "xyz"[k];
    f.offset = (uint32_t)(step + 4 * k);
    f.datatype = pcl::PCLPointField::FLOAT32;
    f.count = 1;
    cloud.fields.push_back(f);
  }
  cloud.point_step = (uint32_t)wide;
  cloud.row_step = (uint32_t)(wide * cloud.width);
}

void MarchingCubesTSDFOctree::performReconstruction(pcl::PolygonMesh &output) {
  output.polygons.clear();
  // color_by_confidence_ wins over color_by_rgb_ (marching_cubes_tsdf_octree.cpp:215-231)
  const int mode = color_by_confidence_ ? 2 : (color_by_rgb_ ? 1 : 0);
  std::vector<float> verts;
  std::vector<unsigned char> rgb;
  std::vector<uint32_t> faces;
  bool indexed = false;
  CleanupArgs cleanup;
  SmoothArgs smooth;
  float flatten = 0.f, decimate = 0.f;
  std::vector<float> normals;
  const bool want_normals = normals_of(this);
  const bool ok = run_march(tsdf_volume_, w_min_, mode, cleanup_of(this, cleanup) ? &cleanup : nullptr, flatten_of(this, flatten) ? &flatten : nullptr,
                            decimate_of(this, decimate) ? &decimate : nullptr, smooth_of(this, smooth) ? &smooth : nullptr,
                            want_normals ? &normals : nullptr, verts, rgb, faces, indexed);
  const size_t n = verts.size() / 3;
  const Eigen::Affine3d g = tsdf_volume_ ? tsdf_volume_->getGlobalTransform() : Eigen::Affine3d::Identity();
  if (mode) {
    pcl::PointCloud<pcl::PointXYZRGB> cloud;
    cloud.points.resize(n);
    cloud.width = (uint32_t)n;
    cloud.height = 1;
    for (size_t i = 0; i < n; ++i) {
      pcl::PointXYZRGB &p = cloud.points[i];
      p.x = verts[3 * i];
      p.y = verts[3 * i + 1];
      p.z = verts[3 * i + 2];
      p.r = rgb[3 * i];
      p.g = rgb[3 * i + 1];
      p.b = rgb[3 * i + 2];
    }
    pcl::transformPointCloud(cloud, cloud, g);
    pcl::toPCLPointCloud2(cloud, output.cloud);
  } else {
    pcl::PointCloud<pcl::PointXYZ> cloud;
    cloud.points.resize(n);
    cloud.width = (uint32_t)n;
    cloud.height = 1;
    for (size_t i = 0; i < n; ++i) {
      pcl::PointXYZ &p = cloud.points[i];
      p.x = verts[3 * i];
      p.y = verts[3 * i + 1];
      p.z = verts[3 * i + 2];
    }
    pcl::transformPointCloud(cloud, cloud, g);
    pcl::toPCLPointCloud2(cloud, output.cloud);
  }
  fill_polygons(n, indexed, faces, output.polygons);
  if (want_normals && ok) append_normals(normals, g, output.cloud);
}

void MarchingCubesTSDFOctree::performReconstruction(pcl::PointCloud<pcl::PointXYZ> &points,
                                                    std::vector<pcl::Vertices> &polygons) {
  std::vector<float> verts;
  std::vector<unsigned char> rgb;
  std::vector<uint32_t> faces;
  bool indexed = false;
  CleanupArgs cleanup;
  SmoothArgs smooth;
  float flatten = 0.f, decimate = 0.f;
  run_march(tsdf_volume_, w_min_, 0, cleanup_of(this, cleanup) ? &cleanup : nullptr, flatten_of(this, flatten) ? &flatten : nullptr,
            decimate_of(this, decimate) ? &decimate : nullptr, smooth_of(this, smooth) ? &smooth : nullptr, nullptr, verts, rgb, faces, indexed);
  const size_t n = verts.size() / 3;
  points.points.resize(n);
  points.width = (uint32_t)n;
  points.height = 1;
  for (size_t i = 0; i < n; ++i) {
    points.points[i].x = verts[3 * i];
    points.points[i].y = verts[3 * i + 1];
    points.points[i].z = verts[3 * i + 2];
  }
  if (tsdf_volume_) pcl::transformPointCloud(points, points, tsdf_volume_->getGlobalTransform());
  fill_polygons(n, indexed, faces, polygons);
}

}  // namespace cpu_tsdf
