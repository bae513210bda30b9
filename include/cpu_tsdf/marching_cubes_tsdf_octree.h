// cpu_tsdf::MarchingCubesTSDFOctree -- MI355X drop-in for the reference mesher
// (include/cpu_tsdf/marching_cubes_tsdf_octree.h:50-100).  As there, it IS a pcl::MarchingCubes<pcl::PointXYZ>: code
// that holds it as a pcl::SurfaceReconstruction / pcl::MarchingCubes reference, or calls the inherited setters
// (setIsoLevel, setGridResolution, setPercentageExtendGrid, setInputCloud -- used by the reference's own setInputTSDF,
// src/lib/marching_cubes_tsdf_octree.cpp:71-78), keeps compiling; reconstruct(pcl::PolygonMesh&) is the inherited
// entry point and lands in performReconstruction below, which runs the HIP marching-cubes kernels instead of walking
// octree leaves.  Triangle order, vertex values and colours equal the reference's.
#pragma once

#include <cpu_tsdf/tsdf_volume_octree.h>
#include <pcl/PolygonMesh.h>
#include <pcl/surface/marching_cubes.h>

#include <vector>

namespace cpu_tsdf {

class MarchingCubesTSDFOctree : public pcl::MarchingCubes<pcl::PointXYZ> {
 public:
  MarchingCubesTSDFOctree()
      : pcl::MarchingCubes<pcl::PointXYZ>(), color_by_confidence_(false), color_by_rgb_(false), w_min_(2.5f) {}
  ~MarchingCubesTSDFOctree() override;  // forgets the object's setCleanup / setFlatten / setDecimate / setSmooth / setNormals (see there)

  // Mirrors the reference (:44-83): remembers the volume and dresses the base class the same way -- grid resolution,
  // the 8-corner "input cloud", no grid extension, iso level 0, bounding box and size_voxel_.
  void setInputTSDF(TSDFVolumeOctree::ConstPtr tsdf_volume);
  void setColorByConfidence(bool color_by_confidence) { color_by_confidence_ = color_by_confidence; }
  void setColorByRGB(bool color_by_rgb) { color_by_rgb_ = color_by_rgb; }
  void setMinWeight(float w_min) { w_min_ = w_min; }
  // Extension (the reference class has no such member): reconstruct drops the faces in connected groups of at most
  // min_neighbors faces -- cleanupMesh of the `integrate` program (src/prog/integrate.cpp:152-214) -- on the GPU, between
  // the march and the fetch (tsdf_hip_march_cleanup).  It acts in the VOLUME frame, before the global transform, and,
  // unlike the program's pass, keeps the colours.
  // The setting lives in the shell library, keyed by the object, NOT in a data member: the class keeps the size and layout
  // it had, so a binary compiled against the earlier header and only re-linked keeps working (its objects end where they
  // used to; a member read behind them would be whatever the stack held).  A copy of the object does not carry it.
  void setCleanup(float face_dist = 0.02f, int min_neighbors = 5);
  void clearCleanup();
  // Extension likewise: reconstruct merges the vertices closer than min_dist -- flattenVertices of the `integrate` program
  // (src/prog/integrate.cpp:103-150) -- on the GPU, after the march (and after setCleanup's pass, which runs FIRST, on the
  // soup), and fills the PolygonMesh with the INDEXED mesh: the merged vertices, each with the colour of the vertex that
  // opened it, and polygons that name them; a face with two equal corners is dropped.  The `integrate` program uses the
  // other order (flatten, then cleanup), as the reference does, and therefore goes through the host-array entry points.
  // The argument lives in the shell library next to setCleanup's: the class keeps its size.
  void setFlatten(float min_dist = 0.0001f);
  void clearFlatten();
  // Extension likewise: reconstruct decimates the mesh by vertex clustering on a grid of edge cell_size (metres, VOLUME
  // frame) -- on the GPU, after the march and after setCleanup's pass, which runs FIRST, on the soup
  // (tsdf_hip_march_decimate; include/tsdf_hip.h states the rules) -- and fills the PolygonMesh with the INDEXED mesh: one
  // vertex per occupied cell, the mean of the cell's vertices and colours; degenerate and duplicate faces are dropped.
  // With BOTH setFlatten and setDecimate, decimate runs and flatten is SKIPPED: clustering already merges what flatten
  // would.  The argument lives in the shell library next to setFlatten's: the class keeps its size.
  void setDecimate(float cell_size);
  void clearDecimate();
  // Extension likewise: reconstruct smooths the INDEXED mesh LAST -- Taubin's lambda | mu, `iterations` times a step with
  // lambda and, iff mu != 0, a step with mu; keep_boundary fixes the endpoints of boundary edges (tsdf_hip_march_smooth;
  // include/tsdf_hip.h states the rules) -- in the VOLUME frame, before the global transform.  Only the vertices move.  With
  // neither setFlatten nor setDecimate, flatten runs first at its default min_dist: a soup has no shared vertices to smooth
  // over.  The arguments live in the shell library next to setDecimate's: the class keeps its size.
  void setSmooth(int iterations, float lambda = 0.5f, float mu = -0.53f, bool keep_boundary = true);
  void clearSmooth();
  // Extension likewise: reconstruct(PolygonMesh&) computes area-weighted vertex normals LAST of all -- after cleanup,
  // flatten / decimate and smooth -- from the mesh it returns (tsdf_hip_march_normals; include/tsdf_hip.h states the rule and
  // the orientation: out of the surface, into observed free space), and appends three FLOAT32 fields normal_x, normal_y,
  // normal_z to the cloud blob.  It works on the soup as well (flat normals).  The normals are computed in the VOLUME frame
  // and turned by the global transform's rotation.  reconstruct(points, polygons) has no place for them.  The argument lives
  // in the shell library next to setSmooth's: the class keeps its size.
  void setNormals(bool on = true);

  using pcl::MarchingCubes<pcl::PointXYZ>::reconstruct;  // reconstruct(PolygonMesh&), reconstruct(points, polygons)

 protected:
  void voxelizeData() override {}  // as in the reference (:86-90): nothing to voxelize, the TSDF is the grid
  // fills output.cloud (PointXYZ, or PointXYZRGB when a colour mode is on) and output.polygons ({3i, 3i+1, 3i+2}, or the
  // indexed mesh's with setFlatten / setDecimate); vertices are moved by the volume's global transform (:108-143)
  void performReconstruction(pcl::PolygonMesh &output) override;
  void performReconstruction(pcl::PointCloud<pcl::PointXYZ> &points, std::vector<pcl::Vertices> &polygons) override;

  TSDFVolumeOctree::ConstPtr tsdf_volume_;
  bool color_by_confidence_, color_by_rgb_;
  float w_min_;
};

}  // namespace cpu_tsdf
