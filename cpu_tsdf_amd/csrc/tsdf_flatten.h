// Internal: what tsdf_flatten.hip (flattenVertices on the GPU) shares with the other translation units.  Kept out of
// tsdf_common.h for the reason tsdf_occupied.h gives.
#pragma once

#include "tsdf_common.h"

// The indexed mesh tsdf_hip_march_flatten left on a handle describes the soup it was made from: a later tsdf_hip_march or
// tsdf_hip_march_cleanup (tsdf_meshpost.hip calls this from both) makes tsdf_hip_march_fetch_indexed refuse until
// flatten has run again.
void tsdf_flatten_invalidate(tsdf_hip_volume *v);
// Frees the per-handle state tsdf_flatten.hip keeps in its own registry (tsdf_meshpost_release calls it).
void tsdf_flatten_release(tsdf_hip_volume *v);

// tsdf_multi.hip: the merged soup of a multi-GPU set (host memory, h->mc_ntri triangles; rgb NULL without a colour mode).
// It goes through tsdf_hip_mesh_flatten on the first slab's device.
void tsdf_multi_mesh(tsdf_handle h, const float **verts, const uint8_t **rgb, const uint64_t **cell);
