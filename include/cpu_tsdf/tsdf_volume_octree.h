// cpu_tsdf::TSDFVolumeOctree -- MI355X drop-in for the reference class of the same name
// (include/cpu_tsdf/tsdf_volume_octree.h:49-377).  Public signatures are kept; the octree of
// shared_ptr voxels is gone: voxels live in a flat SoA grid in HBM behind the C ABI of tsdf_hip.h, and
// every heavy method forwards to a HIP kernel.  What is intentionally absent: the public `octree_`
// member and getFrustumCulledVoxels (they expose OctreeNode pointers).  setColorMode takes "RGB", "RGBNormalized"
// and "LAB" like the reference (LAB: L, A, B state bit-identical, displayed bytes within 1 -- see tsdf_hip.h).
//
// Host-side arithmetic that decides results is done here with the caller's own Eigen/PCL, exactly where
// the reference does it: trans.inverse().cast<float>() (hpp:54), trans.rotation().cast<float>() /
// translation (:303-304), transformPointCloudWithNormals (:422), transformPointCloud in the mesher.
#pragma once

#include <cpu_tsdf/tsdf_interface.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <Eigen/Geometry>
#include <tsdf_hip.h>

#include <string>
#include <vector>

namespace cpu_tsdf {

class TSDFVolumeOctree : public TSDFInterface {
 public:
  typedef boost::shared_ptr<TSDFVolumeOctree> Ptr;
  typedef boost::shared_ptr<const TSDFVolumeOctree> ConstPtr;

  TSDFVolumeOctree();
  ~TSDFVolumeOctree();
  TSDFVolumeOctree(const TSDFVolumeOctree &) = delete;
  TSDFVolumeOctree &operator=(const TSDFVolumeOctree &) = delete;

  void setResolution(int xres, int yres, int zres);
  void getResolution(int &xres, int &yres, int &zres) const;
  void setGridSize(float xsize, float ysize, float zsize);
  void getGridSize(float &xsize, float &ysize, float &zsize) const;
  void setImageSize(int width, int height);
  void getImageSize(int &width, int &height) const;
  void setDepthTruncationLimits(float max_dist_pos, float max_dist_neg);
  void getDepthTruncationLimits(float &max_dist_pos, float &max_dist_neg) const;
  void setWeightTruncationLimit(float max_weight);
  float getWeightTruncationLimit() const;
  void setGlobalTransform(const Eigen::Affine3d &trans) { global_transform_ = trans; }
  Eigen::Affine3d getGlobalTransform() const { return global_transform_; }
  void setCameraIntrinsics(const double focal_length_x, const double focal_length_y,
                           const double principal_point_x, const double principal_point_y);
  void getCameraIntrinsics(double &focal_length_x, double &focal_length_y, double &principal_point_x,
                           double &principal_point_y) const;
  // Accepted and remembered (save() writes them), but a dense grid has no coarse cells / pre-split pass.
  void setMaxVoxelSize(float x, float y, float z);
  void setNumRandomSplts(int n) { num_random_splits_ = n; }
  int getNumRandomSplits() { return num_random_splits_; }
  void setIntegrateColor(bool integrate_color);
  void setColorMode(const std::string &color_mode);
  void setSensorDistanceBounds(float min_sensor_dist, float max_sensor_dist);
  void getSensorDistanceBounds(float &min_sensor_dist, float &max_sensor_dist) const;

  // (Re)allocates the grid on the GPU; every voxel (d = -1, w = 0).
  void reset();
  void save(const std::string &filename) const;
  void load(const std::string &filename);

  bool getFxn(const pcl::PointXYZ &pt, float &val) const;
  bool getGradient(const pcl::PointXYZ &pt, Eigen::Vector3f &grad) const;
  bool getHessian(const pcl::PointXYZ &pt, Eigen::Matrix3f &hessian) const;
  bool getFxnAndGradient(const pcl::PointXYZ &pt, float &val, Eigen::Vector3f &grad) const;
  bool getFxnGradientAndHessian(const pcl::PointXYZ &pt, float &val, Eigen::Vector3f &grad,
                                Eigen::Matrix3f &hessian) const;

  // `cloud` must be organised with the configured image size; only pt.z (and r,g,b when colour is on) is
  // read, `normals` is unused (as in the reference's default settings).  trans: camera -> volume.
  template <typename PointT, typename NormalT>
  bool integrateCloud(const pcl::PointCloud<PointT> &cloud, const pcl::PointCloud<NormalT> &normals,
                      const Eigen::Affine3d &trans = Eigen::Affine3d::Identity());

  pcl::PointCloud<pcl::PointNormal>::Ptr renderView(const Eigen::Affine3d &trans = Eigen::Affine3d::Identity(),
                                                    int downsampleBy = 1) const;
  pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr renderColoredView(
      const Eigen::Affine3d &trans = Eigen::Affine3d::Identity(), int downsampleBy = 1) const;
  pcl::PointCloud<pcl::Intensity>::Ptr getIntensityCloud(const Eigen::Affine3d &trans = Eigen::Affine3d::Identity()) const;

  pcl::PointXYZ getVoxelCenter(size_t x, size_t y, size_t z) const;
  bool getVoxelIndex(float x, float y, float z, int &x_i, int &y_i, int &z_i) const;
  pcl::PointCloud<pcl::PointXYZ>::ConstPtr getVoxelCenters(int nlevels = 4) const;
  void getOccupiedVoxelIndices(std::vector<Eigen::Vector3i> &indices) const;
  bool isEmpty() const { return is_empty_; }

  // ---- extensions (not in the reference) -----------------------------------------------------------------
  // Planar entry point used by the integrateCloud template: depth H x W floats (NaN = no return), bgra
  // 4 bytes per pixel in PointXYZRGBA byte order or NULL.
  bool integratePlanar(const float *depth, const unsigned char *bgra, int width, int height,
                       const Eigen::Affine3d &trans);
  // The two halves the integrateCloud template is made of: beginFrame hands out the pinned staging slot of the next
  // frame (*depth: height x width floats; *bgra: 4 bytes per pixel, or NULL when colour is off), commitFrame queues its
  // upload and the integrate launch and returns (pipelined: see impl/tsdf_volume_octree.hpp).
  bool beginFrame(int width, int height, float **depth, unsigned char **bgra);
  bool commitFrame(const Eigen::Affine3d &trans);
  // The `integrate` program's per-cloud preparation + integrateCloud in one call (src/prog/integrate.cpp:
  // 559-618, 650, 673): an UNORGANISED cloud in sensor units is scaled by cloud_units, (0,0,0) becomes NaN if
  // zero_nans, it is moved by *world_to_cam (= poses[i].inverse()) when given, z-buffered into the configured
  // image on the GPU (tsdf_hip_organize) and integrated with pose `trans`.
  bool integrateUnorganized(const pcl::PointCloud<pcl::PointXYZRGBA> &cloud, const Eigen::Affine3d &trans,
                            float cloud_units = 1.f, bool zero_nans = false,
                            const Eigen::Affine3d *world_to_cam = nullptr, size_t *n_valid_pixels = nullptr);
  // Raw voxel block readback ([z][y][x]); any pointer may be NULL; rgb is 3 bytes per voxel.
  bool downloadBlock(int x0, int y0, int z0, int nx, int ny, int nz, float *d, float *w, unsigned char *rgb) const;
  // The C-ABI handle (NULL before reset()); used by MarchingCubesTSDFOctree.
  tsdf_handle handle() const { return h_; }
  void setTransformOrder(int order) { p_.xform_order = order; }
  void setDevice(int device) { p_.device = device; }
  // Spread the volume over several GPUs of this node: contiguous Z-slabs, one per entry (tsdf_hip_create_multi);
  // takes effect at the next reset() / load().  Every method of this class and MarchingCubesTSDFOctree then drives
  // all of them from this one process: the frame of integrateCloud fans out to every GPU, each integrates its own
  // planes, reconstruct / renderView / getFxn exchange halo planes and ray records between them.  Results do not
  // depend on the partition.  An empty list = one GPU (setDevice).
  void setDevices(const std::vector<int> &devices) { devices_ = devices; }
  const std::vector<int> &getDevices() const { return devices_; }
  // The reference's integrateCloud only visits the voxels pcl::FrustumCulling keeps (getFrustumCulledVoxels,
  // src/lib/tsdf_volume_octree.cpp:619-652): 1.1 x the field of view around the optical AXIS between the sensor-range
  // planes.  integrateCloud here does the same: the six planes are built with the caller's Eigen, operation by operation as
  // pcl::FrustumCulling::applyFilter builds them, and handed to the library per frame (tsdf_hip_set_reference_cull), which
  // applies them wherever they can decide a voxel (for an ordinary camera looking at a volume inside its sensor range:
  // nowhere, at no cost).  setReferenceCull(false) opts out: every voxel updateVoxel itself accepts is integrated.
  void setReferenceCull(bool flag) { reference_cull_ = flag; }
  // Not in the reference: integrateCloud calls are integrated two per sweep of the volume where both camera poses see
  // the whole grid (tsdf_hip_set_frame_pairing: a cloud's kernel waits for the next integrateCloud -- or for any other
  // method of this class, which launches it on its own first).  The same voxels, bit for bit; ~1.15x the frames per
  // second on a stream of clouds.  Takes effect at once and survives reset(); on a setDevices set every slab pairs by itself.
  void setFramePairing(bool flag) {
    frame_pairing_ = flag;
    if (h_) (void)tsdf_hip_set_frame_pairing(h_, flag ? 1 : 0);
  }
  bool getFramePairing() const { return frame_pairing_; }
  // integrateCloud returns as soon as the cloud is staged and its upload + kernel are queued (the reference returns after
  // the work, always `true`; here `false` means the call could not be queued).  A device error of the queued work surfaces
  // at the next call that waits for the device (renderView, getFxn, save, reconstruct, ...).  setSynchronous(true) makes
  // every integrateCloud wait for its own kernel and report its status itself -- the reference's timing, at the price of
  // the overlap (measured: 59.8 against 60.5 frames/s at 2048^3, where the kernel dwarfs the upload; 2x at 512^3).
  void setSynchronous(bool flag) { synchronous_ = flag; }
  bool getSynchronous() const { return synchronous_; }
  bool getReferenceCull() const { return reference_cull_; }
  // TSDF_LAYOUT_* (include/tsdf_hip.h): how the weight is stored in HBM; default AUTO
  void setLayout(int layout) { p_.layout = layout; }
  // Register a cloud to the fused surface (tsdf_hip_align): Gauss-Newton on getFxn over the whole cloud, on the GPU --
  // what getFxn / getGradient exist for in the reference, which leaves the loop to the caller, one point per call.
  // guess / refined: cloud -> volume.  Points with a non-finite z are skipped.  A point counts iff getFxn succeeds, its
  // eight neighbour voxels have weight > min_weight and |getFxn| < r_max (d units).  Stops after max_iterations steps or
  // when the step's norm falls below min_step.  false (and a PCL_ERROR) where no point counts or the cloud leaves a
  // freedom unconstrained; refined then holds the last good step.  Refuses on a non-cubic grid like getFxn.
  template <typename PointT>
  bool alignCloud(const pcl::PointCloud<PointT> &cloud, const Eigen::Affine3d &guess, Eigen::Affine3d &refined,
                  int max_iterations = 10, float min_weight = 0.f, float r_max = 0.9f, double min_step = 1e-7) const;
  // The normal equations of one such step at `trans` (tsdf_hip_align_system): out = 21 upper-triangle entries of
  // sum J J^T, 6 of sum J r, sum r^2, the number of points that count; xyz = n x 3 floats.
  bool getAlignmentSystem(const float *xyz, size_t n, const Eigen::Affine3d &trans, double out[29], float min_weight = 0.f,
                          float r_max = 0.9f) const;
  // out-of-line half of the alignCloud template: xyz = n x 3 floats
  bool alignPoints(const float *xyz, size_t n, const Eigen::Affine3d &guess, Eigen::Affine3d &refined, int max_iterations,
                   float min_weight, float r_max, double min_step) const;
  // Not in the reference: move the volume's window by whole voxels along +x, +y, +z of the volume frame, in place on the
  // GPU (tsdf_hip_shift), so that the dense grid can follow the camera.  Afterwards voxel (x, y, z) holds what voxel
  // (x + sx, y + sy, z + sz) held, or the reset state where that lies outside the grid.  *moved (optional) receives the
  // translation of the volume frame in its own coordinates, s * size / res per axis.  The world stays where it is:
  // global_transform_ becomes global_transform_ * Translation(moved), so MarchingCubesTSDFOctree::reconstruct returns the
  // surviving surface where it was (up to float rounding of the voxel-centre tables).  What the caller owes in return: a
  // pose handed to integrateCloud / renderView / alignCloud afterwards is Translation(-moved) * trans_old.
  // false (and a PCL_ERROR) before reset(), or when the call fails (a setZSlab volume with sz != 0).
  bool shiftVolume(int sx, int sy, int sz, Eigen::Vector3d *moved = nullptr);
  // Not in the reference: resample `src` at this volume's voxel centres under a rigid transform and add the samples as
  // weighted observations, on the GPU (tsdf_hip_merge: the rule and every refusal are in include/tsdf_hip.h) -- joining
  // submaps, changing the resolution, re-centring by a fraction of a voxel or a rotation.  dst_from_src takes src volume
  // coordinates to this volume's; nullptr = getGlobalTransform().inverse() * src.getGlobalTransform().  A voxel is merged
  // iff getFxn(src, q) succeeds at its centre q, the eight neighbour voxels there all have weight > min_weight, and src has
  // a voxel containing q, whose weight and colour the observation carries (RGBNode::addObservation).  *merged (optional)
  // receives the number of merged voxels; the call then waits for the kernel.  src is unchanged.  One device, whole-grid
  // volumes, "RGB" colour, no depth / variance weighting, src cubic; a PACKED volume takes a PACKED src with the same
  // weight limit.  false (and a PCL_ERROR) before reset() of either volume and on any refusal, which changes nothing.
  bool mergeVolume(const TSDFVolumeOctree &src, const Eigen::Affine3d *dst_from_src = nullptr, float min_weight = 0.f,
                   uint64_t *merged = nullptr);
  // Not in the reference: take a cloud back out of the volume on the GPU (tsdf_hip_deintegrate: the rule and every refusal
  // are in include/tsdf_hip.h) -- integrateCloud's signature, with the pose the cloud was integrated under; followed by
  // integrateCloud under a corrected pose this is what a loop closure asks of the map.  The cloud, the pose and the
  // reference cull select exactly the voxels integrateCloud observed, with the same distance and colour; each loses one
  // count and that observation from its running means, and a voxel whose weight reaches 0 returns to the reset state.  A
  // voxel at the weight limit has forgotten how many clouds it saw and loses one count like any other.  *removed
  // (optional) receives the number of voxels whose weight went down.  The call waits for the kernel.  "RGB" colour, no
  // depth / variance weighting, not on a setDevices set.  false (and a PCL_ERROR) before reset() and on any refusal, which
  // changes nothing.  deintegratePlanar: the same on planar images, as integratePlanar.
  template <typename PointT, typename NormalT>
  bool deintegrateCloud(const pcl::PointCloud<PointT> &cloud, const pcl::PointCloud<NormalT> &normals,
                        const Eigen::Affine3d &trans = Eigen::Affine3d::Identity(), uint64_t *removed = nullptr);
  bool deintegratePlanar(const float *depth, const unsigned char *bgra, int width, int height, const Eigen::Affine3d &trans,
                         uint64_t *removed = nullptr);
  // Not in the reference: re-pose a fused cloud in ONE sweep of the volume on the GPU (tsdf_hip_reintegrate: the definition
  // and every refusal are in include/tsdf_hip.h) -- what a corrected pose from a pose graph asks of the map.  The voxels
  // come out, bit for bit, as deintegrateCloud(cloud, normals, old_trans) followed by integrateCloud(cloud, normals,
  // new_trans) leaves them, each half with the default reference-cull planes of its own pose, but every word is read and
  // written once and the band flags survive where the two calls lose them.  The saturation caveat of deintegrateCloud is
  // inherited.  *lowered / *observed (optional) receive the voxels whose weight the removal lowered and the voxels the
  // new pose observed.  The call waits for the kernel.  "RGB" colour, no depth / variance weighting, not on a setDevices
  // set.  false (and a PCL_ERROR) before reset() and on any refusal, which changes nothing.  reintegratePlanar: the same
  // on planar images.
  template <typename PointT, typename NormalT>
  bool reintegrateCloud(const pcl::PointCloud<PointT> &cloud, const pcl::PointCloud<NormalT> &normals, const Eigen::Affine3d &old_trans,
                        const Eigen::Affine3d &new_trans, uint64_t *lowered = nullptr, uint64_t *observed = nullptr);
  bool reintegratePlanar(const float *depth, const unsigned char *bgra, int width, int height, const Eigen::Affine3d &old_trans,
                         const Eigen::Affine3d &new_trans, uint64_t *lowered = nullptr, uint64_t *observed = nullptr);
  // Not in the reference: cast n arbitrary rays into the fused volume on the GPU (tsdf_hip_cast_rays: the definition, the
  // admission rule and every refusal are in include/tsdf_hip.h) -- line of sight, a simulated lidar, picking, view scoring.
  // origins / directions: n x 3 floats, volume frame; a direction is used as given (the step rule is the reference's only for
  // unit directions); t_range: n x 2 floats tmin, tmax per ray, nullptr = the sensor distance bounds.  Ray i gives point i
  // of `hits` (n x 1, is_dense = false): exactly what renderView's loop (tsdf_volume_octree.cpp:290-421) computes for a
  // pixel with that direction, origin and range, in the volume frame -- NaN x, y, z for a miss -- coloured as
  // renderColoredView colours a hit (the voxel that contains it; 127,127,127 without setIntegrateColor).  *status
  // (optional): per ray 0 miss, 1 hit, 2 not admitted (an input that is not finite, or a range of more than 2^24 trips),
  // 3 stopped by the trip cap; no ray can hang the device.  One device, a whole-grid volume, not "LAB" with
  // setIntegrateColor.  false (and a PCL_ERROR) before reset(), on a non-cubic grid and on any refusal, which changes nothing.
  bool castRays(const float *origins, const float *directions, size_t n, pcl::PointCloud<pcl::PointXYZRGBNormal> &hits,
                std::vector<uint8_t> *status = nullptr, const float *t_range = nullptr) const;
  // Not in the reference: the exact Euclidean distance transform of the volume's zero crossing, on the GPU (tsdf_hip_esdf:
  // the rule and every refusal are in include/tsdf_hip.h) -- what a planner or a collision checker asks of the map.  A voxel
  // is a site iff it is observed (weight > min_weight, d not NaN) and a 6-neighbour is observed with the other sign of d;
  // every voxel gets the squared distance in voxels to the nearest site, exactly, or FAR above r_max_voxels^2 when
  // r_max_voxels > 0.  *sites (optional) receives the number of sites.  The field stays on the volume, describing it as it
  // was at this call, until reset(), the destructor or the next computeDistanceField; after shiftVolume it has to be
  // computed again.  getDistanceField returns it for the whole grid, [z][y][x]: dist in metres (sgn * voxel * sqrt(d2),
  // negative where the voxel was observed with d < 0, +-inf where FAR) and, optionally, d2 itself.  getDistance returns the
  // value of the voxel that CONTAINS pt (Octree::getContainingVoxel, no interpolation); false where there is none.
  // One device, a whole-grid volume with cubic voxels on a cubic grid.  All three return false (with a PCL_ERROR) before
  // reset() and on any refusal; the getters also before the first computeDistanceField.
  bool computeDistanceField(int r_max_voxels = 0, float min_weight = 0.f, uint64_t *sites = nullptr);
  bool getDistanceField(std::vector<float> &dist, std::vector<uint32_t> *d2 = nullptr) const;
  bool getDistance(const pcl::PointXYZ &pt, float &dist) const;

  const float UNOBSERVED_VOXEL;

 private:
  bool ready(const char *who) const;
 public:
  // false (and a PCL_ERROR) if setGridSize was not a cube: renderView / getFxn... / MarchingCubesTSDFOctree refuse then
  // (the reference mixes two geometries there; see the definition)
  bool cubicForQueries(const char *who) const;
 private:
  tsdf_params p_;
  tsdf_handle h_;
  float max_cell_size_[3];
  int num_random_splits_;
  bool is_empty_, weight_by_depth_, weight_by_variance_;
  std::string color_mode_;
  std::vector<int> devices_;
  bool reference_cull_ = true;
  bool frame_pairing_ = false;
  bool synchronous_ = false;
  mutable bool cull_planes_set_ = false;
  bool applyReferenceCull(const Eigen::Affine3d &trans) const;
  void referenceCullPlanes(const Eigen::Affine3d &trans, float planes[24]) const;
  // pinned staging for renderView's readback (tsdf_hip_host_alloc): the GPU writes it by DMA, the conversion into the
  // returned PointCloud reads it -- no intermediate copy
  mutable float *view_buf_;
  mutable size_t view_cap_;
  Eigen::Affine3d global_transform_;

 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
};

}  // namespace cpu_tsdf

#include <cpu_tsdf/impl/tsdf_volume_octree.hpp>
