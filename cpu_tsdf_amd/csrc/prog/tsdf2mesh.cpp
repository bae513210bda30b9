// `tsdf2mesh` -- the reference's volume-to-mesh program (src/prog/tsdf2mesh.cpp:50-74) on the MI355X path:
// `tsdf2mesh foo.vol foo.ply` loads a volume written by TSDFVolumeOctree::save (either implementation's),
// runs marching cubes on the GPU with the class defaults (min weight 2.5, no colour) and writes a binary PLY.
// An extension: `tsdf2mesh foo.vol foo.ply --decimate <cell size in metres>` decimates the mesh by vertex clustering before
// it is written (cpu_tsdf::mesh_post::decimateMeshAuto); without the option the output is what it was.
// Likewise `--smooth <iterations> [--smooth-lambda L] [--smooth-mu M]`: Taubin's lambda | mu smoothing (defaults 0.5 and -0.53),
// applied last; a mesh that no --decimate has indexed is flattened first (cpu_tsdf::mesh_post::smoothProgramMesh).
// And `--normals`: area-weighted vertex normals of the mesh that is written, computed from it last of all -- on the soup as well
// (flat normals need no flatten) -- and written as the PLY properties nx, ny, nz (cpu_tsdf::mesh_post::meshNormalsAuto).
// Another: `tsdf2mesh foo.vol foo.ply --merge bar.vol [--merge baz.vol ...]` loads every further volume and merges it into the
// first by the global transforms the files carry (TSDFVolumeOctree::mergeVolume), in the order given, before meshing.
// And: `tsdf2mesh foo.vol foo.ply --esdf foo.npy [--esdf-radius N]` also writes the Euclidean distance field of the whole grid
// (TSDFVolumeOctree::computeDistanceField, after any --merge; truncated at N voxels if given) as a NumPy .npy file: float32
// metres, shape (nz, ny, nx).
#include <cpu_tsdf/marching_cubes_tsdf_octree.h>
#include <cpu_tsdf/tsdf_interface.h>
#include <cpu_tsdf/tsdf_volume_octree.h>

#include <pcl/console/print.h>
#include <pcl/io/ply_io.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mesh_post.h"
#include "npy_write.h"

int main(int argc, char **argv) {
  if (argc < 3) {
    PCL_INFO("Renders a mesh from a TSDF volume saved with TSDFVolumeOctree::save.\nUsage: %s foo.vol foo.ply [--merge other.vol]... [--decimate <cell size in metres>] [--smooth <iterations> [--smooth-lambda L] [--smooth-mu M]] [--normals] [--esdf field.npy [--esdf-radius <voxels>]]\n",
             argv[0]);
    return 1;
  }
  bool decimate_on = false;
  float decimate = 0.f;
  bool smooth_on = false;
  int smooth = 0;
  float smooth_lambda = 0.5f, smooth_mu = -0.53f;
  bool normals_on = false;
  std::vector<std::string> merge;
  std::string esdf;
  int esdf_radius = 0;
  for (int i = 3; i < argc; ++i) {
    if (!strcmp(argv[i], "--merge") && i + 1 < argc) {
      merge.push_back(argv[++i]);
    } else if (!strcmp(argv[i], "--esdf") && i + 1 < argc) {
      esdf = argv[++i];
    } else if (!strcmp(argv[i], "--esdf-radius") && i + 1 < argc) {
      esdf_radius = atoi(argv[++i]);
    } else if (!strcmp(argv[i], "--decimate") && i + 1 < argc) {
      decimate_on = true;
      decimate = (float)atof(argv[++i]);
    } else if (!strcmp(argv[i], "--smooth") && i + 1 < argc) {
      smooth_on = true;
      smooth = atoi(argv[++i]);
    } else if (!strcmp(argv[i], "--smooth-lambda") && i + 1 < argc) {
      smooth_lambda = (float)atof(argv[++i]);
    } else if (!strcmp(argv[i], "--smooth-mu") && i + 1 < argc) {
      smooth_mu = (float)atof(argv[++i]);
    } else if (!strcmp(argv[i], "--normals")) {
      normals_on = true;
    } else {
      PCL_ERROR("unknown option %s\n", argv[i]);
      return 1;
    }
  }
  cpu_tsdf::TSDFVolumeOctree::Ptr tsdf(new cpu_tsdf::TSDFVolumeOctree);
  tsdf->load(argv[1]);
  if (!tsdf->handle()) return 1;
  for (const std::string &name : merge) {
    cpu_tsdf::TSDFVolumeOctree other;
    other.load(name);
    uint64_t merged = 0;  // (asking for the count makes the call wait: `other` is freed at the end of this block)
    if (!other.handle() || !tsdf->mergeVolume(other, nullptr, 0.f, &merged)) {
      PCL_ERROR("--merge %s failed\n", name.c_str());
      return 1;
    }
    PCL_INFO("merged %llu voxels of %s\n", (unsigned long long)merged, name.c_str());
  }
  if (!esdf.empty()) {
    std::vector<float> dist;
    uint64_t sites = 0;
    int rx, ry, rz;
    tsdf->getResolution(rx, ry, rz);
    if (!tsdf->computeDistanceField(esdf_radius, 0.f, &sites) || !tsdf->getDistanceField(dist) ||
        !npy_write_f32(esdf.c_str(), dist.data(), (size_t)rz, (size_t)ry, (size_t)rx)) {
      PCL_ERROR("--esdf %s failed\n", esdf.c_str());
      return 1;
    }
    PCL_INFO("distance field: %llu sites, written to %s\n", (unsigned long long)sites, esdf.c_str());
  }
  cpu_tsdf::MarchingCubesTSDFOctree mc;
  mc.setInputTSDF(tsdf);
  mc.setColorByConfidence(false);
  mc.setColorByRGB(false);
  pcl::PolygonMesh mesh;
  mc.reconstruct(mesh);
  if (decimate_on) {
    std::string why;
    if (const int rc = cpu_tsdf::mesh_post::decimateMeshAuto(mesh, decimate, &why)) {
      PCL_ERROR("--decimate: %s: %s\n", tsdf_hip_error_string(rc), why.c_str());
      return 1;
    }
  }
  if (smooth_on) {
    std::string why;
    if (const int rc = cpu_tsdf::mesh_post::smoothProgramMesh(mesh, !decimate_on, smooth, smooth_lambda, smooth_mu, &why)) {
      PCL_ERROR("--smooth: %s: %s\n", tsdf_hip_error_string(rc), why.c_str());
      return 1;
    }
  }
  if (normals_on) {
    std::string why;
    if (const int rc = cpu_tsdf::mesh_post::meshNormalsAuto(mesh, &why)) {
      PCL_ERROR("--normals: %s: %s\n", tsdf_hip_error_string(rc), why.c_str());
      return 1;
    }
  }
  return pcl::io::savePLYFileBinary(argv[2], mesh);
}
