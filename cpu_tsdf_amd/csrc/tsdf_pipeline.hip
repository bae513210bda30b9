// libtsdf_hip.so -- the pinned staging ring of tsdf_hip_integrate_async / tsdf_hip_frame_begin / tsdf_hip_frame_commit, and frame
// pairing on it.  Host code only: the launches themselves are tsdf_integrate.hip's (tsdf_integrate_frame, tsdf_integrate_launch2).
#include <string.h>

#include <string>

#include "tsdf_common.h"

// Pipelined host entry point: the caller's frame is copied into one of two pinned staging slots and the call
// returns; the host-to-device copy runs on a private copy stream while the previous frame's kernel is still
// busy, and the kernel of this frame waits for the copy through an event.  A stream of host frames then runs
// at the kernel's rate instead of kernel + upload + synchronise.  Results are identical to tsdf_hip_integrate;
// every other entry point is ordered after it on the handle's stream; errors of the asynchronous part surface
// at the next synchronising call (tsdf_hip_synchronize, download, march, ...).
struct tsdf_hip_pipeline {
  static const int SLOTS = 4;  // two frames may wait for their shared sweep while the next two are being staged
  hipStream_t copy_stream = nullptr;
  float *pinned[SLOTS] = {nullptr, nullptr, nullptr, nullptr};   // host, [depth | bgra]
  float *device[SLOTS] = {nullptr, nullptr, nullptr, nullptr};   // device, [depth | bgra]
  hipEvent_t copied[SLOTS] = {nullptr, nullptr, nullptr, nullptr}, consumed[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  unsigned long long frames = 0;
  // frame pairing (tsdf_hip_set_frame_pairing): a committed frame whose kernel launch waits for a partner
  bool pairing = false;
  int pend_slot = 0;
  float pend_T[12];
  bool pend_has_planes = false;
  float pend_planes[24];
};

void tsdf_pipeline_destroy(tsdf_hip_volume *v) {
  tsdf_hip_pipeline *p = v->pipe;
  if (!p) return;
  for (int i = 0; i < tsdf_hip_pipeline::SLOTS; ++i) {
    if (p->consumed[i]) (void)hipEventSynchronize(p->consumed[i]);
    if (p->pinned[i]) (void)hipHostFree(p->pinned[i]);
    if (p->device[i]) (void)hipFree(p->device[i]);
    if (p->copied[i]) (void)hipEventDestroy(p->copied[i]);
    if (p->consumed[i]) (void)hipEventDestroy(p->consumed[i]);
  }
  if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
  delete p;
  v->pipe = nullptr;
  v->pair_pending = false;
}

// The ring itself: tsdf_hip_frame_begin hands out the next pinned slot (waiting until the kernel that last read it
// has finished), tsdf_hip_frame_commit uploads it on the private copy stream and queues the integrate launch behind
// the upload.  A caller that can write its frame straight into the slot (the C++ integrateCloud template stripping a
// PCL cloud) saves the intermediate copy; tsdf_hip_integrate_async is begin + memcpy + commit.
static int pipeline_ready(tsdf_handle h) {
  if (h->pipe) return TSDF_HIP_OK;
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  tsdf_hip_pipeline *p = new tsdf_hip_pipeline;
  // the ring is attached to the handle only once every allocation has succeeded: a half-built one would hand NULL
  // slot pointers to the next tsdf_hip_frame_begin
  auto build = [&]() -> int {
    TSDF_HIP_TRY(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < tsdf_hip_pipeline::SLOTS; ++i) {
      TSDF_HIP_TRY(hipHostMalloc((void **)&p->pinned[i], npx * 8, hipHostMallocPortable));
      TSDF_HIP_TRY(hipMalloc((void **)&p->device[i], npx * 8));
      TSDF_HIP_TRY(hipEventCreateWithFlags(&p->copied[i], hipEventDisableTiming));
      TSDF_HIP_TRY(hipEventCreateWithFlags(&p->consumed[i], hipEventDisableTiming));
    }
    return TSDF_HIP_OK;
  };
  const int rc = build();
  h->pipe = p;
  if (rc) tsdf_pipeline_destroy(h);  // frees what was built and detaches it
  return rc;
}

// Frame pairing launches the frame it has been holding back on its own: with that frame's pose and cull planes, the
// handle's current planes put back afterwards.  Called by every entry point that reads or writes the volume (TSDF_ENTER).
int tsdf_pipeline_flush(tsdf_hip_volume *h) {
  tsdf_hip_pipeline *p = h->pipe;
  if (!h->pair_pending || !p) {
    h->pair_pending = false;
    return TSDF_HIP_OK;
  }
  h->pair_pending = false;
  const bool color = h->p.integrate_color != 0;
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  const bool cur_has = h->ref_cull;
  float cur[24];
  for (int i = 0; i < 24; ++i) cur[i] = h->cull_planes[i];
  h->ref_cull = p->pend_has_planes;
  for (int i = 0; i < 24; ++i) h->cull_planes[i] = p->pend_has_planes ? p->pend_planes[i] : 0.f;
  const int s = p->pend_slot;
  const int rc = tsdf_integrate_launch(h, p->device[s], color ? reinterpret_cast<const uint32_t *>(p->device[s] + npx) : nullptr, p->pend_T, false);
  h->ref_cull = cur_has;
  for (int i = 0; i < 24; ++i) h->cull_planes[i] = cur[i];
  if (rc) return rc;
  TSDF_HIP_TRY(hipEventRecord(p->consumed[s], h->stream));
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_set_frame_pairing(tsdf_handle h, int on) {
  if (!h) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_set_frame_pairing(h, on);
  TSDF_ENTER(h);  // (switching it off launches what was waiting)
  const int rc = pipeline_ready(h);
  if (rc) return rc;
  h->pipe->pairing = on != 0;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_frame_begin(tsdf_handle h, float **depth, uint8_t **bgra) {
  if (!h || !depth) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_frame_begin(h, depth, bgra);
  TSDF_ON_DEVICE(h->device);
  const int rc = pipeline_ready(h);
  if (rc) return rc;
  tsdf_hip_pipeline *p = h->pipe;
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  const int slot = (int)(p->frames % tsdf_hip_pipeline::SLOTS);
  // the slot was last used SLOTS frames ago: its kernel must be done before the staging buffers are reused
  if (p->frames >= (unsigned)tsdf_hip_pipeline::SLOTS) TSDF_HIP_TRY(hipEventSynchronize(p->consumed[slot]));
  *depth = p->pinned[slot];
  if (bgra) *bgra = h->p.integrate_color ? reinterpret_cast<uint8_t *>(p->pinned[slot] + npx) : nullptr;
  return TSDF_HIP_OK;
}

// The ring's second half, once frame `slot` is on its way into p->device[slot] and the handle's stream waits for it: launch
// it, or -- frame pairing -- hold it back for a partner / launch it together with the frame that was waiting.
static int pipeline_commit_uploaded(tsdf_handle h, int slot, const float cam_from_vol[12]) {
  tsdf_hip_pipeline *p = h->pipe;
  const bool color = h->p.integrate_color != 0;
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  auto bgra_of = [&](int s) { return color ? reinterpret_cast<const uint32_t *>(p->device[s] + npx) : nullptr; };
  if (h->pair_pending) {  // the partner has arrived: one sweep for both where the poses allow it, two launches otherwise
    h->pair_pending = false;
    const int sa = p->pend_slot;
    const int rc = tsdf_integrate_launch2(h, p->device[sa], bgra_of(sa), p->pend_T, p->pend_has_planes ? p->pend_planes : nullptr,
                                          p->device[slot], bgra_of(slot), cam_from_vol, h->ref_cull ? h->cull_planes : nullptr, false, nullptr);
    // Whatever the launch did, both ring slots are handed back in order (their `consumed` events recorded, the frame
    // counter advanced): a failure must not leave a slot whose upload or launch state the next frame_begin cannot know
    // (ADVICE r04).  A failed launch integrated NEITHER frame or only the first: the error text says a frame was lost.
    (void)hipEventRecord(p->consumed[sa], h->stream);
    (void)hipEventRecord(p->consumed[slot], h->stream);
    if (rc) {
      p->frames++;
      const std::string why = tsdf_hip_last_error();
      tsdf_set_error("paired commit failed -- the frame held back for pairing and this one are LOST (not integrated): " + why);
      return rc;
    }
  } else if (p->pairing) {  // uploaded, but its kernel waits for the next frame (or for any other call on the volume)
    p->pend_slot = slot;
    for (int i = 0; i < 12; ++i) p->pend_T[i] = cam_from_vol[i];
    p->pend_has_planes = h->ref_cull;
    for (int i = 0; i < 24; ++i) p->pend_planes[i] = h->cull_planes[i];
    h->pair_pending = true;
  } else {
    const int rc = tsdf_integrate_frame(h, p->device[slot], bgra_of(slot), cam_from_vol, nullptr);
    if (rc) return rc;
    TSDF_HIP_TRY(hipEventRecord(p->consumed[slot], h->stream));
  }
  p->frames++;
  return TSDF_HIP_OK;
}

extern "C" int tsdf_hip_frame_commit(tsdf_handle h, const float cam_from_vol[12]) {
  if (!h || !cam_from_vol) return TSDF_HIP_E_INVALID;
  if (h->multi) return tsdf_multi_frame_commit(h, cam_from_vol);
  if (!h->pipe) {
    tsdf_set_error("tsdf_hip_frame_commit without tsdf_hip_frame_begin");
    return TSDF_HIP_E_INVALID;
  }
  TSDF_ON_DEVICE(h->device);
  tsdf_hip_pipeline *p = h->pipe;
  const bool color = h->p.integrate_color != 0;
  const size_t npx = (size_t)h->p.image_width * h->p.image_height, bytes = npx * 4 * (color ? 2 : 1);
  const int slot = (int)(p->frames % tsdf_hip_pipeline::SLOTS);
  TSDF_HIP_TRY(hipMemcpyAsync(p->device[slot], p->pinned[slot], bytes, hipMemcpyHostToDevice, p->copy_stream));
  TSDF_HIP_TRY(hipEventRecord(p->copied[slot], p->copy_stream));
  TSDF_HIP_TRY(hipStreamWaitEvent(h->stream, p->copied[slot], 0));
  return pipeline_commit_uploaded(h, slot, cam_from_vol);
}

// A SLAB of a multi-GPU set takes a frame through its own ring (tsdf_multi.hip, frame pairing on a set): the frame already
// sits in `src` -- the set's pinned host slot (src_dev < 0: one upload over this GPU's own PCIe link) or a device buffer on
// GPU src_dev (a peer copy, or the pinned relay where the driver refuses peer access: `copy`) -- and goes into the slab's next
// ring slot on the slab's copy stream; then exactly what tsdf_hip_frame_commit does.  *uploaded, when given, is recorded on
// the copy stream behind the copy (the set waits for it before it reuses its pinned slot).
int tsdf_pipeline_commit_from(tsdf_handle s, const void *src, int src_dev, const float T[12], bool pairing, hipEvent_t uploaded,
                              int (*copy)(void *ctx, void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipStream_t st), void *ctx) {
  TSDF_ON_DEVICE(s->device);
  int rc = pipeline_ready(s);
  if (rc) return rc;
  tsdf_hip_pipeline *p = s->pipe;
  if (p->pairing != pairing) {
    if (s->pair_pending && (rc = tsdf_pipeline_flush(s))) return rc;
    p->pairing = pairing;
  }
  const bool color = s->p.integrate_color != 0;
  const size_t npx = (size_t)s->p.image_width * s->p.image_height, bytes = npx * 4 * (color ? 2 : 1);
  const int slot = (int)(p->frames % tsdf_hip_pipeline::SLOTS);
  if (p->frames >= (unsigned)tsdf_hip_pipeline::SLOTS) TSDF_HIP_TRY(hipEventSynchronize(p->consumed[slot]));
  if (src_dev < 0) {
    TSDF_HIP_TRY(hipMemcpyAsync(p->device[slot], src, bytes, hipMemcpyHostToDevice, p->copy_stream));
  } else if ((rc = copy(ctx, p->device[slot], s->device, src, src_dev, bytes, p->copy_stream))) {
    return rc;
  }
  TSDF_HIP_TRY(hipEventRecord(p->copied[slot], p->copy_stream));
  if (uploaded) TSDF_HIP_TRY(hipEventRecord(uploaded, p->copy_stream));
  TSDF_HIP_TRY(hipStreamWaitEvent(s->stream, p->copied[slot], 0));
  return pipeline_commit_uploaded(s, slot, T);
}

// ... and two device frames at once (tsdf_hip_integrate_device2 on a set): both into ring slots, one tsdf_integrate_launch2.
int tsdf_pipeline_pair_from(tsdf_handle s, const void *src_a, const void *src_b, int src_dev, const float TA[12], const float *planes_a,
                            const float TB[12], const float *planes_b, bool count, bool *fused,
                            int (*copy)(void *ctx, void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipStream_t st), void *ctx) {
  TSDF_ENTER(s);  // (a frame this slab was holding back goes first)
  int rc = pipeline_ready(s);
  if (rc) return rc;
  tsdf_hip_pipeline *p = s->pipe;
  const bool color = s->p.integrate_color != 0;
  const size_t npx = (size_t)s->p.image_width * s->p.image_height, bytes = npx * 4 * (color ? 2 : 1);
  int slot[2];
  const void *src[2] = {src_a, src_b};
  for (int k = 0; k < 2; ++k) {
    slot[k] = (int)((p->frames + k) % tsdf_hip_pipeline::SLOTS);
    if (p->frames + k >= (unsigned)tsdf_hip_pipeline::SLOTS) TSDF_HIP_TRY(hipEventSynchronize(p->consumed[slot[k]]));
    if ((rc = copy(ctx, p->device[slot[k]], s->device, src[k], src_dev, bytes, p->copy_stream))) return rc;
    TSDF_HIP_TRY(hipEventRecord(p->copied[slot[k]], p->copy_stream));
    TSDF_HIP_TRY(hipStreamWaitEvent(s->stream, p->copied[slot[k]], 0));
  }
  auto bgra_of = [&](int q) { return color ? reinterpret_cast<const uint32_t *>(p->device[q] + npx) : nullptr; };
  rc = tsdf_integrate_launch2(s, p->device[slot[0]], bgra_of(slot[0]), TA, planes_a, p->device[slot[1]], bgra_of(slot[1]), TB, planes_b, count, fused);
  (void)hipEventRecord(p->consumed[slot[0]], s->stream);
  (void)hipEventRecord(p->consumed[slot[1]], s->stream);
  p->frames += 2;
  return rc;
}

extern "C" int tsdf_hip_integrate_async(tsdf_handle h, const float *depth, const uint8_t *bgra,
                                        const float cam_from_vol[12]) {
  if (!h || !depth || !cam_from_vol) return TSDF_HIP_E_INVALID;
  if (h->p.integrate_color && !bgra) {
    tsdf_set_error("integrate_color is set but no colour image was given");
    return TSDF_HIP_E_INVALID;
  }
  float *sd = nullptr;
  uint8_t *sc = nullptr;
  const int rc = tsdf_hip_frame_begin(h, &sd, &sc);
  if (rc) return rc;
  const size_t npx = (size_t)h->p.image_width * h->p.image_height;
  memcpy(sd, depth, npx * 4);
  if (sc) memcpy(sc, bgra, npx * 4);
  return tsdf_hip_frame_commit(h, cam_from_vol);
}
