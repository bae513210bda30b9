// integrateCloud template of the MI355X drop-in: strips the organised PCL cloud down to the two planar images the
// kernel reads (pt.z, and b,g,r,a when colour is on) -- straight into the volume's pinned staging slot
// (tsdf_hip_frame_begin) -- and queues upload + integrate
// (tsdf_hip_frame_commit).  The call returns once the frame is staged: the upload overlaps the previous frame's kernel
// and every later call on the volume is ordered after it, so a stream of clouds runs at the kernel's rate.
// The reference reads exactly these fields (include/cpu_tsdf/impl/tsdf_volume_octree.hpp:150-159,206); like there,
// PointT needs r,g,b members.
#pragma once

#include <cmath>
#include <vector>

namespace cpu_tsdf {

template <typename PointT, typename NormalT>
bool TSDFVolumeOctree::integrateCloud(const pcl::PointCloud<PointT> &cloud, const pcl::PointCloud<NormalT> &,
                                      const Eigen::Affine3d &trans) {
  float *depth = nullptr;
  unsigned char *bgra = nullptr;
  // the staging slot holds image_width x image_height pixels: a cloud whose point count disagrees with its own
  // width x height would overrun it (more points) or leave pixels of an older frame in it (fewer)
  if (cloud.points.size() != (size_t)cloud.width * (size_t)cloud.height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::integrateCloud] cloud has %zu points but says %u x %u\n", cloud.points.size(),
              (unsigned)cloud.width, (unsigned)cloud.height);
    return false;
  }
  if (!beginFrame((int)cloud.width, (int)cloud.height, &depth, &bgra)) return false;
  const long n = (long)cloud.points.size();
  const PointT *pts = n ? &cloud.points[0] : nullptr;
  // ONE thread, on purpose.  The strip reads 32-byte points and writes 8 bytes per pixel: memory-bound, 0.5-0.6 ms for a
  // 640x480 cloud on one core -- a twentieth of the kernel it runs ahead of (the call returns once the frame is staged).  Until
  // round 6 this loop was an `omp parallel for` over the caller's default team: on a host whose container grants fewer CPUs
  // than it shows (a 256-thread team under a CPU quota) the team's barrier waited for the scheduler, 104 ms per call --
  // the drop-in ran at 8 frames/s where the kernel does 78 (profiles/r06_cpp_path_timing_before.json).
  uint32_t *bgra32 = reinterpret_cast<uint32_t *>(bgra);  // the slot is 16-byte aligned
  if (bgra32) {
    for (long i = 0; i < n; ++i) {
      depth[i] = pts[i].z;
      bgra32[i] = (uint32_t)pts[i].b | ((uint32_t)pts[i].g << 8) | ((uint32_t)pts[i].r << 16) | 0xff000000u;  // PCL order b, g, r, a
    }
  } else {
    for (long i = 0; i < n; ++i) depth[i] = pts[i].z;
  }
  return commitFrame(trans);
}

// deintegrateCloud: the same strip of the organised cloud as integrateCloud's, into host buffers, then the out-of-line
// forwarder to tsdf_hip_deintegrate (which takes them through the volume's pinned staging and waits for the kernel).
template <typename PointT, typename NormalT>
bool TSDFVolumeOctree::deintegrateCloud(const pcl::PointCloud<PointT> &cloud, const pcl::PointCloud<NormalT> &,
                                        const Eigen::Affine3d &trans, uint64_t *removed) {
  if (cloud.points.size() != (size_t)cloud.width * (size_t)cloud.height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::deintegrateCloud] cloud has %zu points but says %u x %u\n", cloud.points.size(),
              (unsigned)cloud.width, (unsigned)cloud.height);
    return false;
  }
  const size_t n = cloud.points.size();
  std::vector<float> depth(n);
  std::vector<uint32_t> bgra(n);
  for (size_t i = 0; i < n; ++i) {
    const PointT &pt = cloud.points[i];
    depth[i] = pt.z;
    bgra[i] = (uint32_t)pt.b | ((uint32_t)pt.g << 8) | ((uint32_t)pt.r << 16) | 0xff000000u;  // PCL order b, g, r, a
  }
  return deintegratePlanar(n ? &depth[0] : nullptr, n ? reinterpret_cast<const unsigned char *>(&bgra[0]) : nullptr, (int)cloud.width,
                           (int)cloud.height, trans, removed);
}

// reintegrateCloud: deintegrateCloud's strip, then the out-of-line forwarder to tsdf_hip_reintegrate.
template <typename PointT, typename NormalT>
bool TSDFVolumeOctree::reintegrateCloud(const pcl::PointCloud<PointT> &cloud, const pcl::PointCloud<NormalT> &,
                                        const Eigen::Affine3d &old_trans, const Eigen::Affine3d &new_trans, uint64_t *lowered,
                                        uint64_t *observed) {
  if (cloud.points.size() != (size_t)cloud.width * (size_t)cloud.height) {
    PCL_ERROR("[cpu_tsdf::TSDFVolumeOctree::reintegrateCloud] cloud has %zu points but says %u x %u\n", cloud.points.size(),
              (unsigned)cloud.width, (unsigned)cloud.height);
    return false;
  }
  const size_t n = cloud.points.size();
  std::vector<float> depth(n);
  std::vector<uint32_t> bgra(n);
  for (size_t i = 0; i < n; ++i) {
    const PointT &pt = cloud.points[i];
    depth[i] = pt.z;
    bgra[i] = (uint32_t)pt.b | ((uint32_t)pt.g << 8) | ((uint32_t)pt.r << 16) | 0xff000000u;  // PCL order b, g, r, a
  }
  return reintegratePlanar(n ? &depth[0] : nullptr, n ? reinterpret_cast<const unsigned char *>(&bgra[0]) : nullptr, (int)cloud.width,
                           (int)cloud.height, old_trans, new_trans, lowered, observed);
}

// alignCloud: x, y, z of the points with a finite z into one contiguous buffer (as integrateCloud strips its cloud), then
// the out-of-line forwarder to tsdf_hip_align.
template <typename PointT>
bool TSDFVolumeOctree::alignCloud(const pcl::PointCloud<PointT> &cloud, const Eigen::Affine3d &guess, Eigen::Affine3d &refined,
                                  int max_iterations, float min_weight, float r_max, double min_step) const {
  std::vector<float> xyz;
  xyz.reserve(3 * cloud.points.size());
  for (size_t i = 0; i < cloud.points.size(); ++i) {
    const PointT &pt = cloud.points[i];
    if (!std::isfinite(pt.z)) continue;
    xyz.push_back(pt.x);
    xyz.push_back(pt.y);
    xyz.push_back(pt.z);
  }
  return alignPoints(xyz.empty() ? nullptr : &xyz[0], xyz.size() / 3, guess, refined, max_iterations, min_weight, r_max, min_step);
}

}  // namespace cpu_tsdf
