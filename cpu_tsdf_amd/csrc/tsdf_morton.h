// Internal: the Morton key of a voxel or cell, x the high bit of every triple -- the order OctreeNode::getLeaves walks the
// leaves in (octree.cpp:119,257-264), which marching cubes and the occupied-voxel list emit in.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

static inline __host__ __device__ uint64_t tsdf_spread3(uint64_t v) {  // 21 bits -> every third bit
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

static inline __host__ __device__ uint32_t tsdf_compact3(uint64_t v) {  // every third bit -> 21 bits (tsdf_spread3's inverse)
  v &= 0x1249249249249249ull;
  v = (v | v >> 2) & 0x10c30c30c30c30c3ull;
  v = (v | v >> 4) & 0x100f00f00f00f00full;
  v = (v | v >> 8) & 0x1f0000ff0000ffull;
  v = (v | v >> 16) & 0x1f00000000ffffull;
  v = (v | v >> 32) & 0x1fffffull;
  return (uint32_t)v;
}

static inline __host__ __device__ uint64_t tsdf_morton_key(uint64_t x, uint64_t y, uint64_t z) {
  return (tsdf_spread3(x) << 2) | (tsdf_spread3(y) << 1) | tsdf_spread3(z);
}
