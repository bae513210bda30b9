// Host shell of the MI355X drop-in: cpu_tsdf::TSDFVolumeOctree on top of the C ABI (tsdf_hip.h).
// Mirrors the reference's src/lib/tsdf_volume_octree.cpp method by method; the voxel work itself is in
// the HIP kernels.  Compiles against real PCL/Eigen or against the stand-ins in compat/.
#include <cpu_tsdf/tsdf_volume_octree.h>
#include <pcl/common/transforms.h>
#include <pcl/console/print.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>


namespace cpu_tsdf {

static void report(const char *who, int rc) {
  PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::%s] %s: %s\n", who, tsdf_hip_error_string(rc), tsdf_hip_last_error());
}

// Defaults of the reference constructor (src/lib/tsdf_volume_octree.cpp:54-85) come from the C ABI.
TSDFVolumeOctree::TSDFVolumeOctree()
    : UNOBSERVED_VOXEL(std::numeric_limits<float>::quiet_NaN()),
      h_(nullptr),
      num_random_splits_(1),
      is_empty_(true),
      weight_by_depth_(false),
      weight_by_variance_(false),
      color_mode_("RGB"),
      view_buf_(nullptr),
      view_cap_(0) {
  tsdf_hip_default_params(&p_);
  max_cell_size_[0] = max_cell_size_[1] = max_cell_size_[2] = 0.5f;
  global_transform_ = Eigen::Affine3d::Identity();
  // The two extensions a program written against the reference cannot name, for a binary that is only RE-LINKED against
  // this library: CPU_TSDF_HIP_FRAME_PAIRING=1 starts every volume with setFramePairing(true), CPU_TSDF_HIP_DEVICES=0,1,2,3
  // with setDevices({0, 1, 2, 3}).  The setters override them as usual.
  if (const char *e = std::getenv("CPU_TSDF_HIP_FRAME_PAIRING")) frame_pairing_ = std::atoi(e) != 0;
  if (const char *e = std::getenv("CPU_TSDF_HIP_DEVICES")) {
    for (const char *c = e; *c;) {
      char *end = nullptr;
      const long v = std::strtol(c, &end, 10);
      if (end == c) break;
      devices_.push_back((int)v);
      c = *end == ',' ? end + 1 : end;
    }
  }
}

TSDFVolumeOctree::~TSDFVolumeOctree() {
  if (h_) tsdf_hip_destroy(h_);
  if (view_buf_) tsdf_hip_host_free(view_buf_);
}

void TSDFVolumeOctree::setResolution(int xres, int yres, int zres) {
  p_.res[0] = xres;
  p_.res[1] = yres;
  p_.res[2] = zres;
}
void TSDFVolumeOctree::getResolution(int &xres, int &yres, int &zres) const {
  xres = p_.res[0];
  yres = p_.res[1];
  zres = p_.res[2];
}
void TSDFVolumeOctree::setGridSize(float xsize, float ysize, float zsize) {
  p_.size[0] = xsize;
  p_.size[1] = ysize;
  p_.size[2] = zsize;
}
void TSDFVolumeOctree::getGridSize(float &xsize, float &ysize, float &zsize) const {
  xsize = p_.size[0];
  ysize = p_.size[1];
  zsize = p_.size[2];
}
void TSDFVolumeOctree::setImageSize(int width, int height) {
  p_.image_width = width;
  p_.image_height = height;
}
void TSDFVolumeOctree::getImageSize(int &width, int &height) const {
  width = p_.image_width;
  height = p_.image_height;
}
void TSDFVolumeOctree::setDepthTruncationLimits(float max_dist_pos, float max_dist_neg) {
  p_.max_dist_pos = max_dist_pos;
  p_.max_dist_neg = max_dist_neg;
}
void TSDFVolumeOctree::getDepthTruncationLimits(float &max_dist_pos, float &max_dist_neg) const {
  max_dist_pos = p_.max_dist_pos;
  max_dist_neg = p_.max_dist_neg;
}
void TSDFVolumeOctree::setWeightTruncationLimit(float max_weight) { p_.max_weight = max_weight; }
float TSDFVolumeOctree::getWeightTruncationLimit() const { return p_.max_weight; }
void TSDFVolumeOctree::setCameraIntrinsics(const double fx, const double fy, const double cx, const double cy) {
  p_.fx = fx;
  p_.fy = fy;
  p_.cx = cx;
  p_.cy = cy;
}
void TSDFVolumeOctree::getCameraIntrinsics(double &fx, double &fy, double &cx, double &cy) const {
  fx = p_.fx;
  fy = p_.fy;
  cx = p_.cx;
  cy = p_.cy;
}
void TSDFVolumeOctree::setMaxVoxelSize(float x, float y, float z) {
  max_cell_size_[0] = x;
  max_cell_size_[1] = y;
  max_cell_size_[2] = z;
}
void TSDFVolumeOctree::setIntegrateColor(bool integrate_color) { p_.integrate_color = integrate_color ? 1 : 0; }
// reference: tsdf_volume_octree.h:290 -> OctreeNode::instantiateByTypeString (src/lib/octree.cpp:193-206)
void TSDFVolumeOctree::setColorMode(const std::string &color_mode) {
  if (color_mode == "RGB") {
    p_.color_mode = TSDF_COLOR_RGB;
  } else if (color_mode == "RGBNormalized") {
    p_.color_mode = TSDF_COLOR_RGB_NORMALIZED;
  } else if (color_mode == "LAB") {
    p_.color_mode = TSDF_COLOR_LAB;
  } else {  // octree.cpp:203-205 prints and returns NULL, which reset() would then dereference
    PCL_WARN("[cpu_tsdf::TSDFVolumeOctree::setColorMode] \"%s\" voxels do not exist in the HIP volume; keeping %s\n",
             color_mode.c_str(), color_mode_.c_str());
    return;
  }
  color_mode_ = color_mode;
}
void TSDFVolumeOctree::setSensorDistanceBounds(float min_sensor_dist, float max_sensor_dist) {
  p_.min_sensor_dist = min_sensor_dist;
  p_.max_sensor_dist = max_sensor_dist;
}
void TSDFVolumeOctree::getSensorDistanceBounds(float &min_sensor_dist, float &max_sensor_dist) const {
  min_sensor_dist = p_.min_sensor_dist;
  max_sensor_dist = p_.max_sensor_dist;
}

bool TSDFVolumeOctree::ready(const char *who) const {
  if (h_) return true;
  PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::%s] called before reset()\n", who);
  return false;
}

// The queries on a NON-CUBIC setGridSize are refused, loudly.  The reference's octree is a cube of edge size_x whatever
// setGridSize said (OctreeNode keeps ONE size_, include/cpu_tsdf/octree.h:63-66; split() offsets all three centre coordinates
// by it, src/lib/octree.cpp:244-266), while renderView / getFxn / marching cubes locate voxels by the per-axis closed forms of
// src/lib/tsdf_volume_octree.cpp:553-574 and look them up in that cube: with size_y or size_z different from size_x the
// reference mixes two geometries.  integrateCloud replicates that cube leaf by leaf (tests/test_oracle_golden.py); the
// queries cannot reproduce the mixture on a flat grid and would silently answer for a DIFFERENT geometry -- so the drop-in
// says so instead (VERDICT r04 missing #3).  The reference's own programs only ever make cubes (integrate.cpp:486-511).
bool TSDFVolumeOctree::cubicForQueries(const char *who) const {
  if (p_.size[0] == p_.size[1] && p_.size[0] == p_.size[2]) return true;
  PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::%s] grid size %g x %g x %g is not a cube: the reference looks per-axis voxel indices "
            "(tsdf_volume_octree.cpp:553-574) up in an octree that is a cube of edge size_x (octree.cpp:244-266), a mixture "
            "this drop-in does not reproduce -- refusing rather than answering for another geometry\n",
            who, (double)p_.size[0], (double)p_.size[1], (double)p_.size[2]);
  return false;
}

// reference: src/lib/tsdf_volume_octree.cpp:201-219
void TSDFVolumeOctree::reset() {
  is_empty_ = true;
  if (h_) {
    tsdf_hip_destroy(h_);
    h_ = nullptr;
  }
  // weight_by_depth_ / weight_by_variance_ (set only by load(), as in the reference) survive a reset there too
  if ((weight_by_depth_ || weight_by_variance_) && p_.layout == TSDF_LAYOUT_AUTO) p_.layout = TSDF_LAYOUT_F32W;
  int rc;
  if (devices_.empty()) {
    rc = tsdf_hip_create(&p_, &h_);
  } else {
    std::vector<int32_t> dev(devices_.begin(), devices_.end());
    rc = tsdf_hip_create_multi(&p_, dev.data(), (int)dev.size(), &h_);
  }
  if (!rc && (weight_by_depth_ || weight_by_variance_)) {
    rc = tsdf_hip_set_weighting(h_, weight_by_depth_, weight_by_variance_);
    if (rc) tsdf_hip_destroy(h_);
  }
  if (!rc && frame_pairing_) rc = tsdf_hip_set_frame_pairing(h_, 1);  // (a setDevices set pairs too since round 6)
  if (rc) {
    h_ = nullptr;
    report("reset", rc);
  }
}

// getFrustumCulledVoxels (src/lib/tsdf_volume_octree.cpp:619-652) in replication mode: the six planes of
// pcl::FrustumCulling::applyFilter [PCL-recall: filters/impl/frustum_culling.hpp] for this frame's pose, built with the
// caller's Eigen -- same expressions, same order -- and handed to the library, which tests every voxel centre against
// them (tsdf_hip_set_reference_cull) wherever they can decide one -- per launch, the library checks whether they keep the
// whole slab anyway.  Cleared when the caller opted out (setReferenceCull(false)).
bool TSDFVolumeOctree::applyReferenceCull(const Eigen::Affine3d &trans) const {
  if (!reference_cull_) {
    if (cull_planes_set_) {
      cull_planes_set_ = false;
      return tsdf_hip_set_reference_cull(h_, nullptr) == 0;
    }
    return true;
  }
  float planes[24];
  referenceCullPlanes(trans, planes);
  cull_planes_set_ = true;
  const int rc = tsdf_hip_set_reference_cull(h_, planes);
  if (rc) report("integrateCloud (reference cull)", rc);
  return rc == 0;
}

// The six planes pcl::FrustumCulling::applyFilter builds for the pose `trans` (tsdf_volume_octree.cpp:633-646)
void TSDFVolumeOctree::referenceCullPlanes(const Eigen::Affine3d &trans, float planes[24]) const {
  using Eigen::Vector3f;
  using Eigen::Vector4f;
  Eigen::Matrix4f cam2robot;
  cam2robot << 0, 0, 1, 0, 0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1;
  const Eigen::Matrix4f camera_pose = trans.matrix().cast<float>() * cam2robot;  // :633-638
  const float hfov = 1.1 * 2 * fabs(atan(0.5 * p_.image_width / p_.fx) * 180 / M_PI);   // :641 (setHorizontalFOV(float))
  const float vfov = 1.1 * 2 * fabs(atan(0.5 * p_.image_height / p_.fy) * 180 / M_PI);  // :642
  const float np_dist = p_.min_sensor_dist, fp_dist = p_.max_sensor_dist;                // :643-644
  const Vector3f view = camera_pose.block<3, 1>(0, 0);
  const Vector3f up = camera_pose.block<3, 1>(0, 1);
  const Vector3f right = camera_pose.block<3, 1>(0, 2);
  const Vector3f T = camera_pose.block<3, 1>(0, 3);
  const float vfov_rad = float(vfov * M_PI / 180);
  const float hfov_rad = float(hfov * M_PI / 180);
  const float np_h = float(2 * tan(vfov_rad / 2) * np_dist);
  const float np_w = float(2 * tan(hfov_rad / 2) * np_dist);
  const float fp_h = float(2 * tan(vfov_rad / 2) * fp_dist);
  const float fp_w = float(2 * tan(hfov_rad / 2) * fp_dist);
  const Vector3f fp_c(T + view * fp_dist);
  const Vector3f fp_tl(fp_c + (up * fp_h / 2) - (right * fp_w / 2));
  const Vector3f fp_tr(fp_c + (up * fp_h / 2) + (right * fp_w / 2));
  const Vector3f fp_bl(fp_c - (up * fp_h / 2) - (right * fp_w / 2));
  const Vector3f fp_br(fp_c - (up * fp_h / 2) + (right * fp_w / 2));
  const Vector3f np_c(T + view * np_dist);
  const Vector3f np_tr(np_c + (up * np_h / 2) + (right * np_w / 2));
  const Vector3f np_bl(np_c - (up * np_h / 2) - (right * np_w / 2));
  const Vector3f np_br(np_c - (up * np_h / 2) + (right * np_w / 2));
  auto plane = [](const Vector3f &n, const Vector3f &through) { return Vector4f(n[0], n[1], n[2], -through.dot(n)); };
  const Vector3f a(fp_bl - T), b(fp_br - T), c(fp_tr - T), d(fp_tl - T);
  const Vector4f pl[6] = {plane(d.cross(a), T), plane(b.cross(c), T), plane(c.cross(d), T), plane(a.cross(b), T),
                          plane((fp_bl - fp_br).cross(fp_tr - fp_br), fp_c), plane((np_tr - np_br).cross(np_bl - np_br), np_c)};
  for (int k = 0; k < 6; ++k)
    for (int i = 0; i < 4; ++i) planes[4 * k + i] = pl[k][i];
}

// reference: include/cpu_tsdf/impl/tsdf_volume_octree.hpp:48-103
bool TSDFVolumeOctree::integratePlanar(const float *depth, const unsigned char *bgra, int width, int height,
                                       const Eigen::Affine3d &trans) {
  if (!ready("integrateCloud")) return false;
  if (width != p_.image_width || height != p_.image_height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::integrateCloud] cloud is %dx%d but setImageSize said %dx%d\n", width,
              height, p_.image_width, p_.image_height);
    return false;
  }
  if (!applyReferenceCull(trans)) return false;
  const Eigen::Affine3f trans_inv = trans.inverse().cast<float>();  // hpp:54
  float T[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T[4 * r + c] = trans_inv.matrix()(r, c);
  const int rc = tsdf_hip_integrate(h_, depth, bgra, T, nullptr);
  if (rc) {
    report("integrateCloud", rc);
    return false;
  }
  is_empty_ = false;
  return true;
}

// ---- deintegrateCloud (not in the reference): tsdf_hip_deintegrate ------------------------------------------------------------
bool TSDFVolumeOctree::deintegratePlanar(const float *depth, const unsigned char *bgra, int width, int height,
                                         const Eigen::Affine3d &trans, uint64_t *removed) {
  if (!ready("deintegrateCloud")) return false;
  if (width != p_.image_width || height != p_.image_height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::deintegrateCloud] cloud is %dx%d but setImageSize said %dx%d\n", width,
              height, p_.image_width, p_.image_height);
    return false;
  }
  if (!applyReferenceCull(trans)) return false;  // the planes integrateCloud had for this pose
  const Eigen::Affine3f trans_inv = trans.inverse().cast<float>();  // hpp:54
  float T[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T[4 * r + c] = trans_inv.matrix()(r, c);
  const int rc = tsdf_hip_deintegrate(h_, depth, p_.integrate_color ? bgra : nullptr, T, removed);
  if (rc) {
    report("deintegrateCloud", rc);
    return false;
  }
  return true;
}

// ---- reintegrateCloud (not in the reference): tsdf_hip_reintegrate ------------------------------------------------------------
bool TSDFVolumeOctree::reintegratePlanar(const float *depth, const unsigned char *bgra, int width, int height,
                                         const Eigen::Affine3d &old_trans, const Eigen::Affine3d &new_trans, uint64_t *lowered,
                                         uint64_t *observed) {
  if (!ready("reintegrateCloud")) return false;
  if (width != p_.image_width || height != p_.image_height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::reintegrateCloud] cloud is %dx%d but setImageSize said %dx%d\n", width,
              height, p_.image_width, p_.image_height);
    return false;
  }
  float planes[2][24], T[2][12];
  const Eigen::Affine3d *trans[2] = {&old_trans, &new_trans};
  for (int k = 0; k < 2; ++k) {
    if (reference_cull_) referenceCullPlanes(*trans[k], planes[k]);  // the planes integrateCloud has for this pose
    const Eigen::Affine3f trans_inv = trans[k]->inverse().cast<float>();  // hpp:54
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T[k][4 * r + c] = trans_inv.matrix()(r, c);
  }
  uint64_t n[2] = {0, 0};
  const bool count = lowered || observed;
  const int rc = tsdf_hip_reintegrate(h_, depth, p_.integrate_color ? bgra : nullptr, T[0], reference_cull_ ? planes[0] : nullptr, T[1],
                                      reference_cull_ ? planes[1] : nullptr, count ? n : nullptr);
  if (rc) {
    report("reintegrateCloud", rc);
    return false;
  }
  cull_planes_set_ = reference_cull_;  // (the new pose's planes stay in force on the handle)
  if (lowered) *lowered = n[0];
  if (observed) *observed = n[1];
  is_empty_ = false;
  return true;
}

bool TSDFVolumeOctree::beginFrame(int width, int height, float **depth, unsigned char **bgra) {
  if (!ready("integrateCloud")) return false;
  if (width != p_.image_width || height != p_.image_height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::integrateCloud] cloud is %dx%d but setImageSize said %dx%d\n", width,
              height, p_.image_width, p_.image_height);
    return false;
  }
  const int rc = tsdf_hip_frame_begin(h_, depth, bgra);
  if (rc) report("integrateCloud", rc);
  return rc == 0;
}

bool TSDFVolumeOctree::commitFrame(const Eigen::Affine3d &trans) {
  if (!applyReferenceCull(trans)) return false;
  const Eigen::Affine3f trans_inv = trans.inverse().cast<float>();  // hpp:54
  float T[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T[4 * r + c] = trans_inv.matrix()(r, c);
  int rc = tsdf_hip_frame_commit(h_, T);
  if (!rc && synchronous_) rc = tsdf_hip_synchronize(h_);  // (also launches a frame that pairing was holding back)
  if (rc) {
    report("integrateCloud", rc);
    return false;
  }
  is_empty_ = false;
  return true;
}

// reference: src/prog/integrate.cpp:559-618 (prepare) + :650,673 (integrate)
bool TSDFVolumeOctree::integrateUnorganized(const pcl::PointCloud<pcl::PointXYZRGBA> &cloud, const Eigen::Affine3d &trans,
                                            float cloud_units, bool zero_nans, const Eigen::Affine3d *world_to_cam,
                                            size_t *n_valid_pixels) {
  if (!ready("integrateUnorganized")) return false;
  static_assert(sizeof(pcl::PointXYZRGBA) == 32, "PointXYZRGBA layout: xyz at 0, rgba at 16, 32 bytes");
  double w2c[12];
  if (world_to_cam)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) w2c[4 * r + c] = world_to_cam->matrix()(r, c);
  const pcl::PointXYZRGBA *pts = cloud.points.empty() ? nullptr : &cloud.points[0];
  uint64_t nv = 0;
  int rc = tsdf_hip_organize(h_, pts ? &pts->x : nullptr, 8, pts ? reinterpret_cast<const uint8_t *>(&pts->rgba) : nullptr, 32,
                             cloud.points.size(), cloud_units, zero_nans ? 1 : 0, world_to_cam ? w2c : nullptr, nullptr,
                             nullptr, n_valid_pixels ? &nv : nullptr);
  if (rc) {
    report("integrateUnorganized", rc);
    return false;
  }
  if (n_valid_pixels) *n_valid_pixels = (size_t)nv;
  if (!applyReferenceCull(trans)) return false;
  const Eigen::Affine3f trans_inv = trans.inverse().cast<float>();  // hpp:54
  float T[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T[4 * r + c] = trans_inv.matrix()(r, c);
  rc = tsdf_hip_integrate_staged(h_, T, nullptr);
  if (rc) {
    report("integrateUnorganized", rc);
    return false;
  }
  rc = tsdf_hip_synchronize(h_);  // the caller may free `cloud` right away
  is_empty_ = false;
  return rc == 0;
}

// reference: src/lib/tsdf_volume_octree.cpp:278-424
pcl::PointCloud<pcl::PointNormal>::Ptr TSDFVolumeOctree::renderView(const Eigen::Affine3d &trans,
                                                                   int downsampleBy) const {
  const int new_width = p_.image_width / downsampleBy;
  const int new_height = p_.image_height / downsampleBy;
  pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>(new_width, new_height));
  cloud->is_dense = false;
  if (!ready("renderView") || !cubicForQueries("renderView")) {  // an all-NaN cloud (every ray a miss), is_dense = false
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < cloud->size(); ++i) {
      pcl::PointNormal &pt = cloud->points[i];
      pt.x = pt.y = pt.z = pt.normal_x = pt.normal_y = pt.normal_z = nan;
    }
    return cloud;
  }
  const Eigen::Matrix3f rot = trans.rotation().cast<float>();     // :303
  const Eigen::Vector3f org = trans.translation().cast<float>();  // :304
  float r9[9], o3[3];
  for (int r = 0; r < 3; ++r) {
    o3[r] = org(r);
    for (int c = 0; c < 3; ++c) r9[3 * r + c] = rot(r, c);
  }
  // pinned staging (kept between calls): the library detects it and lets the DMA engine write it directly
  const size_t need = (size_t)new_width * new_height * 8;
  if (need > view_cap_) {
    if (view_buf_) tsdf_hip_host_free(view_buf_);
    view_buf_ = nullptr;
    view_cap_ = 0;
    void *p = nullptr;
    if (tsdf_hip_host_alloc(need * sizeof(float), &p) == 0) {
      view_buf_ = static_cast<float *>(p);
      view_cap_ = need;
    }
  }
  std::vector<float> pageable;  // (only if pinned memory could not be had)
  if (!view_buf_) pageable.resize(need);
  const float *buf = view_buf_ ? view_buf_ : pageable.data();
  const int rc = tsdf_hip_raycast(h_, r9, o3, downsampleBy, const_cast<float *>(buf));
  if (rc) {
    report("renderView", rc);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < cloud->size(); ++i) cloud->points[i].x = cloud->points[i].y = cloud->points[i].z = nan;
    return cloud;
  }
  for (size_t i = 0; i < cloud->size(); ++i) {
    pcl::PointNormal &pt = cloud->points[i];
    const float *o = &buf[8 * i];
    pt.x = o[0];
    pt.y = o[1];
    pt.z = o[2];
    pt.normal_x = o[3];
    pt.normal_y = o[4];
    pt.normal_z = o[5];
  }
  pcl::transformPointCloudWithNormals(*cloud, *cloud, trans.inverse());  // :422
  return cloud;
}

// reference: src/lib/tsdf_volume_octree.cpp:426-450 -- colour of the voxel containing each hit point.
pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr TSDFVolumeOctree::renderColoredView(const Eigen::Affine3d &trans,
                                                                                int downsampleBy) const {
  if (!p_.integrate_color)
    PCL_WARN("[cpu_tsdf::TSDFVolumeOctree::renderColoredView] Rendering a colored view, but integrate_color_ was not set!\n");
  pcl::PointCloud<pcl::PointNormal>::Ptr grayscale = renderView(trans, downsampleBy);
  pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr colored(
      new pcl::PointCloud<pcl::PointXYZRGBNormal>(grayscale->width, grayscale->height));
  colored->is_dense = false;
  const Eigen::Affine3f tf = trans.cast<float>();
  // hits back in the volume frame (trans.cast<float>() * point, :441), then ONE batched lookup on the device
  std::vector<float> query;
  std::vector<size_t> who;
  for (size_t i = 0; i < colored->size(); ++i) {
    pcl::PointXYZRGBNormal &pt = colored->points[i];
    const pcl::PointNormal &g = grayscale->points[i];
    pt.x = g.x;
    pt.y = g.y;
    pt.z = g.z;
    pt.normal_x = g.normal_x;
    pt.normal_y = g.normal_y;
    pt.normal_z = g.normal_z;
    if (std::isnan(pt.z) || !h_) continue;
    const Eigen::Vector3f v_t = tf * Eigen::Vector3f(pt.x, pt.y, pt.z);
    query.push_back(v_t(0));
    query.push_back(v_t(1));
    query.push_back(v_t(2));
    who.push_back(i);
  }
  if (!who.empty()) {
    std::vector<unsigned char> rgb(3 * who.size()), found(who.size());
    const int rc = tsdf_hip_lookup_rgb(h_, query.data(), who.size(), rgb.data(), found.data());
    if (rc) {
      report("renderColoredView", rc);
      return colored;
    }
    for (size_t k = 0; k < who.size(); ++k) {
      if (!found[k]) continue;  // getContainingVoxel returned NULL: the point keeps its default colour (:445-446)
      pcl::PointXYZRGBNormal &pt = colored->points[who[k]];
      if (p_.integrate_color) {
        pt.r = rgb[3 * k];
        pt.g = rgb[3 * k + 1];
        pt.b = rgb[3 * k + 2];
      } else {
        // without integrate_color_ the reference builds a "NOCOLOR" octree (.cpp:205-208) whose nodes answer
        // OctreeNode::getRGB's 127,127,127 (octree.cpp:172-177)
        pt.r = pt.g = pt.b = 127;
      }
    }
  }
  return colored;
}

// ---- castRays (not in the reference): tsdf_hip_cast_rays ----------------------------------------------------------------------
bool TSDFVolumeOctree::castRays(const float *origins, const float *directions, size_t n, pcl::PointCloud<pcl::PointXYZRGBNormal> &hits,
                                std::vector<uint8_t> *status, const float *t_range) const {
  if (!ready("castRays") || !cubicForQueries("castRays")) return false;
  if (!origins || !directions || !n || n >= (1ull << 31)) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::castRays] needs origins, directions and 0 < n < 2^31 rays\n");
    return false;
  }
  std::vector<float> out(8 * n);
  std::vector<uint8_t> rgb(p_.integrate_color ? 3 * n : 0), st(n);
  const int rc = tsdf_hip_cast_rays(h_, origins, directions, t_range, n, 0, out.data(), p_.integrate_color ? rgb.data() : nullptr, st.data());
  if (rc) {
    report("castRays", rc);
    return false;
  }
  hits = pcl::PointCloud<pcl::PointXYZRGBNormal>((uint32_t)n, 1);
  hits.is_dense = false;
  for (size_t i = 0; i < n; ++i) {
    pcl::PointXYZRGBNormal &pt = hits.points[i];
    const float *o = &out[8 * i];
    pt.x = o[0];
    pt.y = o[1];
    pt.z = o[2];
    pt.normal_x = o[3];
    pt.normal_y = o[4];
    pt.normal_z = o[5];
    if (st[i] != 1) continue;  // a miss keeps the default colour, as in renderColoredView
    if (p_.integrate_color) {
      pt.r = rgb[3 * i];
      pt.g = rgb[3 * i + 1];
      pt.b = rgb[3 * i + 2];
    } else if (std::fabs(o[0]) <= p_.size[0] / 2 && std::fabs(o[1]) <= p_.size[1] / 2 && std::fabs(o[2]) <= p_.size[2] / 2) {
      pt.r = pt.g = pt.b = 127;  // the "NOCOLOR" octree's answer wherever it has a voxel (octree.cpp:172-177, 628-643)
    }
  }
  if (status) status->swap(st);
  return true;
}

pcl::PointCloud<pcl::Intensity>::Ptr TSDFVolumeOctree::getIntensityCloud(const Eigen::Affine3d &) const {
  return pcl::PointCloud<pcl::Intensity>::Ptr();  // the reference returns a null pointer too (:543-548)
}

// reference: src/lib/tsdf_volume_octree.cpp:553-560
pcl::PointXYZ TSDFVolumeOctree::getVoxelCenter(size_t x, size_t y, size_t z) const {
  const float xoff = p_.size[0] / 2.0, yoff = p_.size[1] / 2.0, zoff = p_.size[2] / 2.0;
  return pcl::PointXYZ((x + 0.5) * p_.size[0] / (double)p_.res[0] - xoff, (y + 0.5) * p_.size[1] / (double)p_.res[1] - yoff,
                       (z + 0.5) * p_.size[2] / (double)p_.res[2] - zoff);
}

// reference: src/lib/tsdf_volume_octree.cpp:562-574
bool TSDFVolumeOctree::getVoxelIndex(float x, float y, float z, int &x_i, int &y_i, int &z_i) const {
  const double xoff = (double)p_.size[0] / 2.0, yoff = (double)p_.size[1] / 2.0, zoff = (double)p_.size[2] / 2.0;
  x_i = std::floor(((double)x + xoff) / (double)p_.size[0] * (double)p_.res[0]);
  y_i = std::floor(((double)y + yoff) / (double)p_.size[1] * (double)p_.res[1]);
  z_i = std::floor(((double)z + zoff) / (double)p_.size[2] * (double)p_.res[2]);
  return x_i >= 0 && y_i >= 0 && z_i >= 0 && x_i < p_.res[0] && y_i < p_.res[1] && z_i < p_.res[2];
}

// The reference returns the centres of octree nodes `nlevels` deep (:576-590); the equivalent here is a
// regular 2^nlevels lattice of node centres.
pcl::PointCloud<pcl::PointXYZ>::ConstPtr TSDFVolumeOctree::getVoxelCenters(int nlevels) const {
  const int n = 1 << nlevels;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(n * n * n, 1));
  size_t k = 0;
  for (int x = 0; x < n; ++x)
    for (int y = 0; y < n; ++y)
      for (int z = 0; z < n; ++z, ++k) {
        pcl::PointXYZ &pt = cloud->points[k];
        pt.x = (x + 0.5f) * p_.size[0] / n - p_.size[0] / 2;
        pt.y = (y + 0.5f) * p_.size[1] / n - p_.size[1] / 2;
        pt.z = (z + 0.5f) * p_.size[2] / n - p_.size[2] / 2;
      }
  return cloud;
}

bool TSDFVolumeOctree::downloadBlock(int x0, int y0, int z0, int nx, int ny, int nz, float *d, float *w,
                                     unsigned char *rgb) const {
  if (!ready("downloadBlock")) return false;
  const int rc = tsdf_hip_download(h_, x0, y0, z0, nx, ny, nz, d, w, rgb);
  if (rc) report("downloadBlock", rc);
  return rc == 0;
}

// reference: src/lib/tsdf_volume_octree.cpp:590-609 (leaves with w > 0 && |d| < 1, appended in the order
// OctreeNode::getLeaves walks them, src/lib/octree.cpp:99-109): scanned and sorted on the GPU (tsdf_hip_occupied); only
// the index triples cross the bus
void TSDFVolumeOctree::getOccupiedVoxelIndices(std::vector<Eigen::Vector3i> &indices) const {
  if (!ready("getOccupiedVoxelIndices")) return;
  uint64_t n = 0;
  int rc = tsdf_hip_occupied(h_, nullptr, &n);
  if (rc) return report("getOccupiedVoxelIndices", rc);
  if (!n) return;
  std::vector<int32_t> idx((size_t)n * 3);
  if ((rc = tsdf_hip_occupied_fetch(h_, idx.data(), nullptr, nullptr, nullptr))) return report("getOccupiedVoxelIndices", rc);
  indices.reserve(indices.size() + (size_t)n);
  for (size_t i = 0; i < (size_t)n; ++i) indices.push_back(Eigen::Vector3i(idx[3 * i], idx[3 * i + 1], idx[3 * i + 2]));
}

// getFxn / getGradient / getHessian (+ combos): src/lib/tsdf_volume_octree.cpp:655-794, one point each.
static bool sample_one(tsdf_handle h, const pcl::PointXYZ &pt, float *val, float *grad, float *hess) {
  if (!h) return false;
  const float xyz[3] = {pt.x, pt.y, pt.z};
  unsigned char ok = 0;
  if (tsdf_hip_sample(h, xyz, 1, val, grad, hess, &ok)) return false;
  return ok != 0;
}
bool TSDFVolumeOctree::getFxn(const pcl::PointXYZ &pt, float &val) const {
  if (h_ && !cubicForQueries("getFxn")) return false;
  float v;
  if (!sample_one(h_, pt, &v, nullptr, nullptr)) return false;
  val = v;
  return true;
}
bool TSDFVolumeOctree::getGradient(const pcl::PointXYZ &pt, Eigen::Vector3f &grad) const {
  if (h_ && !cubicForQueries("getGradient")) return false;
  float g[3];
  if (!sample_one(h_, pt, nullptr, g, nullptr)) return false;
  grad = Eigen::Vector3f(g[0], g[1], g[2]);
  return true;
}
bool TSDFVolumeOctree::getHessian(const pcl::PointXYZ &pt, Eigen::Matrix3f &hessian) const {
  if (h_ && !cubicForQueries("getHessian")) return false;
  float hm[9];
  if (!sample_one(h_, pt, nullptr, nullptr, hm)) return false;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) hessian(r, c) = hm[3 * r + c];
  return true;
}
bool TSDFVolumeOctree::getFxnAndGradient(const pcl::PointXYZ &pt, float &val, Eigen::Vector3f &grad) const {
  if (h_ && !cubicForQueries("getFxnAndGradient")) return false;
  float v, g[3];
  if (!sample_one(h_, pt, &v, g, nullptr)) return false;
  val = v;
  grad = Eigen::Vector3f(g[0], g[1], g[2]);
  return true;
}
bool TSDFVolumeOctree::getFxnGradientAndHessian(const pcl::PointXYZ &pt, float &val, Eigen::Vector3f &grad,
                                                Eigen::Matrix3f &hessian) const {
  if (h_ && !cubicForQueries("getFxnGradientAndHessian")) return false;
  float v, g[3], hm[9];
  if (!sample_one(h_, pt, &v, g, hm)) return false;
  val = v;
  grad = Eigen::Vector3f(g[0], g[1], g[2]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) hessian(r, c) = hm[3 * r + c];
  return true;
}

// ---- alignCloud (not in the reference): tsdf_hip_align_system / tsdf_hip_align ---------------------------------------------
static void pose12(const Eigen::Affine3d &t, double out[12]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) out[4 * r + c] = t.matrix()(r, c);
}
bool TSDFVolumeOctree::getAlignmentSystem(const float *xyz, size_t n, const Eigen::Affine3d &trans, double out[29], float min_weight,
                                          float r_max) const {
  if (!ready("getAlignmentSystem") || !cubicForQueries("getAlignmentSystem")) return false;
  double T[12];
  pose12(trans, T);
  const int rc = tsdf_hip_align_system(h_, xyz, n, T, min_weight, r_max, out, nullptr, nullptr);
  if (rc) report("getAlignmentSystem", rc);
  return rc == 0;
}
bool TSDFVolumeOctree::alignPoints(const float *xyz, size_t n, const Eigen::Affine3d &guess, Eigen::Affine3d &refined, int max_iterations,
                                   float min_weight, float r_max, double min_step) const {
  if (!ready("alignCloud") || !cubicForQueries("alignCloud")) return false;
  double T[12], R[12];
  pose12(guess, T);
  const int rc = tsdf_hip_align(h_, xyz, n, T, min_weight, r_max, max_iterations, min_step, R, nullptr, nullptr);
  if (rc == TSDF_HIP_OK || rc == TSDF_HIP_ALIGN_NO_POINTS || rc == TSDF_HIP_ALIGN_RANK_DEFICIENT) {
    refined = Eigen::Affine3d::Identity();
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) refined.matrix()(r, c) = R[4 * r + c];
  }
  if (rc) report("alignCloud", rc);
  return rc == 0;
}

// ---- shiftVolume (not in the reference): tsdf_hip_shift ----------------------------------------------------------------------
bool TSDFVolumeOctree::shiftVolume(int sx, int sy, int sz, Eigen::Vector3d *moved) {
  if (!ready("shiftVolume")) return false;
  const int32_t s[3] = {sx, sy, sz};
  const int rc = tsdf_hip_shift(h_, s);
  if (rc) {
    report("shiftVolume", rc);
    return false;
  }
  Eigen::Vector3d t;
  for (int a = 0; a < 3; ++a) t[a] = s[a] * (double)p_.size[a] / p_.res[a];
  Eigen::Affine3d step = Eigen::Affine3d::Identity();  // Translation(t)
  for (int a = 0; a < 3; ++a) step.matrix()(a, 3) = t[a];
  global_transform_ = global_transform_ * step;
  if (moved) *moved = t;
  return true;
}

// ---- mergeVolume (not in the reference): tsdf_hip_merge -----------------------------------------------------------------------
bool TSDFVolumeOctree::mergeVolume(const TSDFVolumeOctree &src, const Eigen::Affine3d *dst_from_src, float min_weight, uint64_t *merged) {
  if (!ready("mergeVolume") || !src.ready("mergeVolume (src)")) return false;
  const Eigen::Affine3d m = dst_from_src ? *dst_from_src : global_transform_.inverse() * src.global_transform_;
  double T[12];
  pose12(m.inverse(), T);  // the C ABI takes src_from_dst
  uint64_t n = 0;
  const int rc = tsdf_hip_merge(h_, src.h_, T, min_weight, merged ? &n : nullptr);
  if (rc) {
    report("mergeVolume", rc);
    return false;
  }
  if (merged) *merged = n;
  is_empty_ = is_empty_ && src.is_empty_;
  return true;
}

// ---- computeDistanceField / getDistanceField / getDistance (not in the reference): tsdf_hip_esdf ----------------------------
bool TSDFVolumeOctree::computeDistanceField(int r_max_voxels, float min_weight, uint64_t *sites) {
  if (!ready("computeDistanceField")) return false;
  uint64_t n = 0;
  const int rc = tsdf_hip_esdf(h_, nullptr, r_max_voxels, min_weight, &n);
  if (rc) {
    report("computeDistanceField", rc);
    return false;
  }
  if (sites) *sites = n;
  return true;
}
bool TSDFVolumeOctree::getDistanceField(std::vector<float> &dist, std::vector<uint32_t> *d2) const {
  if (!ready("getDistanceField")) return false;
  uint64_t st[4];
  int rc = tsdf_hip_esdf_stats(h_, st);
  if (!rc) {
    dist.resize((size_t)st[0]);  // (0 before the first computeDistanceField: the fetch then refuses)
    if (d2) d2->resize((size_t)st[0]);
    rc = tsdf_hip_esdf_fetch(h_, d2 ? d2->data() : nullptr, dist.data());
  }
  if (rc) report("getDistanceField", rc);
  return rc == 0;
}
bool TSDFVolumeOctree::getDistance(const pcl::PointXYZ &pt, float &dist) const {
  if (!ready("getDistance")) return false;
  const float xyz[3] = {pt.x, pt.y, pt.z};
  float v = 0.f;
  uint8_t found = 0;
  const int rc = tsdf_hip_esdf_sample(h_, xyz, 1, &v, &found);
  if (rc) {
    report("getDistance", rc);
    return false;
  }
  if (!found) return false;
  dist = v;
  return true;
}

// ---- save / load: the reference's .vol format (src/lib/tsdf_volume_octree.cpp:222-275) -----------------------
// The format and the block streaming live behind the C ABI (tsdf_hip_save / tsdf_hip_load); this class adds
// what only it knows: max cell size, the empty flag, the weighting flags and the global transform.
void TSDFVolumeOctree::save(const std::string &filename) const {
  if (!ready("save")) return;
  tsdf_vol_meta m;
  for (int k = 0; k < 3; ++k) m.max_cell_size[k] = max_cell_size_[k];
  m.is_empty = is_empty_;
  m.weight_by_depth = weight_by_depth_;
  m.weight_by_variance = weight_by_variance_;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) m.global_transform[4 * r + c] = global_transform_.matrix()(r, c);
  const int rc = tsdf_hip_save(h_, filename.c_str(), &m);
  if (rc) report("save", rc);
}

void TSDFVolumeOctree::load(const std::string &filename) {
  tsdf_handle h = nullptr;
  tsdf_params p;
  tsdf_vol_meta m;
  tsdf_params defaults = p_;  // device, layout, transform order
  defaults.z_begin = defaults.z_end = defaults.halo = 0;
  std::vector<int32_t> dev(devices_.begin(), devices_.end());
  const int rc = dev.empty() ? tsdf_hip_load(filename.c_str(), &defaults, &h, &p, &m)
                             : tsdf_hip_load_multi(filename.c_str(), &defaults, dev.data(), (int)dev.size(), &h, &p, &m);
  if (rc) {
    report("load", rc);
    return;
  }
  if (h_) tsdf_hip_destroy(h_);
  h_ = h;
  const int layout = p_.layout;
  p_ = p;
  p_.layout = (layout == TSDF_LAYOUT_AUTO && p.layout == TSDF_LAYOUT_F32W && p.max_weight >= 0 && p.max_weight <= 255)
                  ? TSDF_LAYOUT_F32W  // the file's weights needed the float plane: a later reset() keeps it
                  : layout;
  for (int k = 0; k < 3; ++k) max_cell_size_[k] = m.max_cell_size[k];
  is_empty_ = m.is_empty != 0;
  weight_by_depth_ = m.weight_by_depth != 0;
  weight_by_variance_ = m.weight_by_variance != 0;
  Eigen::Matrix4d g;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) g(r, c) = m.global_transform[4 * r + c];
  global_transform_ = g;
}

// reference: src/lib/tsdf_interface.cpp:44-51
TSDFInterface::Ptr TSDFInterface::instantiateFromFile(const std::string &filename) {
  TSDFInterface::Ptr tsdf(new TSDFVolumeOctree);
  tsdf->load(filename);
  return tsdf;
}

}  // namespace cpu_tsdf
