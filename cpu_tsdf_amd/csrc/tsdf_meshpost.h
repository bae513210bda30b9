// Internal: what tsdf_meshpost.hip (cleanupMesh on the GPU) shares with the other translation units.  Kept out of
// tsdf_common.h for the reason tsdf_occupied.h gives: that header's hash stamps the committed k_integrate profiles.
#pragma once

#include "tsdf_common.h"

// Frees the per-handle state tsdf_meshpost.hip keeps in its own registry (workspace, events).  tsdf_hip_destroy calls it
// for every handle; a handle that only marched has just the note below.
void tsdf_meshpost_release(tsdf_hip_volume *v);
// tsdf_hip_march notes the outcome of every call here: tsdf_hip_march_cleanup refuses a handle that never marched, or whose
// last march failed (its buffers then hold nothing that call vouches for).
void tsdf_meshpost_note_march(tsdf_hip_volume *v, bool succeeded);
// Did the last tsdf_hip_march on this handle succeed?  (tsdf_hip_march_flatten asks: it works on that result too.)
bool tsdf_meshpost_marched(tsdf_hip_volume *v);

// tsdf_multi.hip: the merged mesh of a multi-GPU set lives on the host; it goes through tsdf_hip_mesh_cleanup on the first
// slab's device and the host copy is compacted.
int tsdf_multi_march_cleanup(tsdf_handle h, float face_dist, int min_neighbors, uint64_t *n_tri);
