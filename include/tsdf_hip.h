/*
 * tsdf_hip.h -- C ABI of the MI355X (gfx950) TSDF fusion library (libtsdf_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes only, no C++ / torch types.
 * The C++ host shell (the headers under include/cpu_tsdf/, same class names and signatures as the
 * reference) and the Python binding (cpu_tsdf_amd/capi.py) both sit on top of it.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * sdmiller/cpu_tsdf tree).  All functions return 0 on success or a TSDF_HIP_E_* code;
 * the reference itself has no error reporting, the host shell maps
 * failures to `false` / empty results.
 *
 * Volume storage: flat SoA planes in HBM, x fastest:
 *     d  [nz_local][ny][pitch]  float   truncation-normalised distance, init -1
 *     w  [nz_local][ny][pitch]  float   weight, init 0                     (F32W layout)
 *     rgb[nz_local][ny][pitch]  uint32  r | g<<8 | b<<16 (only when integrate_color); in the PACKED layout
 *                                       byte 3 holds the observation count k, w = min(k, max_weight)
 *     k  [nz_local][ny][pitch]  uint8   the same count when PACKED without colour
 * pitch = nx rounded up to a multiple of 4.  A handle may own only a Z-slab
 * [z_begin, z_end) of the full grid (multi-GPU partitioning) plus `halo` extra planes on
 * each side that integrate never touches but raycast / marching cubes may read.
 */
#ifndef TSDF_HIP_H
#define TSDF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsdf_hip_volume *tsdf_handle;

enum {
  TSDF_HIP_OK = 0,
  TSDF_HIP_E_INVALID = 1,     /* bad argument / params */
  TSDF_HIP_E_NOMEM = 2,       /* hipMalloc failed */
  TSDF_HIP_E_HIP = 3,         /* any other HIP runtime error (see tsdf_hip_last_error) */
  TSDF_HIP_E_NODEVICE = 4,    /* no gfx950 device visible */
  TSDF_HIP_E_UNSUPPORTED = 5,
  TSDF_HIP_E_IO = 6,          /* file missing, unreadable, unwritable or not a .vol (see tsdf_hip_last_error) */
  /* statuses of tsdf_hip_align only: not failures of the library, the cloud cannot be aligned */
  TSDF_HIP_ALIGN_NO_POINTS = 7,      /* no point passed the gate at the current pose */
  TSDF_HIP_ALIGN_RANK_DEFICIENT = 8  /* the used points do not constrain all six freedoms (Cholesky failed) */
};

/* Summation order of the rigid transform g = T * (c,1), which decides the last ulp of the
 * camera-frame voxel centre (include/cpu_tsdf/impl/tsdf_volume_octree.hpp:145 calls
 * pcl::transformPoint, whose arithmetic lives in PCL, not in the reference tree). */
enum {
  TSDF_XFORM_PCL_SSE = 0,     /* x*c0 + (y*c1 + (z*c2 + c3))   PCL >= 1.10 Transformer<float>::se3, SSE2 build */
  TSDF_XFORM_LEFT_TO_RIGHT = 1 /* ((m0*x + m1*y) + m2*z) + m3    PCL scalar build / Eigen Affine3f * Vector3f */
};

/* How the weight is stored.  Every observation adds w_new = 1 and clamps at max_weight
 * (src/lib/octree.cpp:156-158; the depth/variance weightings of hpp:200-204 have no setter), so
 * w == min(k, max_weight) where k counts observations.  PACKED stores k in one byte -- byte 3 of the
 * colour word, or a uint8 plane without colour -- and saves a third of the HBM traffic of integrateCloud;
 * every entry point still speaks float weights.  It needs 0 <= max_weight <= 255 and weights of that form:
 * tsdf_hip_upload refuses anything else with TSDF_HIP_E_UNSUPPORTED (load such a volume with F32W).
 * AUTO = PACKED when max_weight allows it, else F32W. */
enum { TSDF_LAYOUT_AUTO = 0, TSDF_LAYOUT_F32W = 1, TSDF_LAYOUT_PACKED = 2 };

/* Which voxel class carries the colour (setColorMode, include/cpu_tsdf/tsdf_volume_octree.h:290 ->
 * OctreeNode::instantiateByTypeString, src/lib/octree.cpp:193-206).  Only read when integrate_color is set.
 *   RGB             RGBNode (octree.cpp:328-337): three truncated uint8 running means.  The default.
 *   RGB_NORMALIZED  RGBNormalized (octree.cpp:380-402): running means of r/i, g/i, b/i and of the intensity
 *                   i = sqrt(r^2+g^2+b^2) as four floats; the colour read back is (uint8)(r_n * i) etc.
 *                   Four more float planes per voxel, float weights (no PACKED layout), a plain per-voxel
 *                   kernel; tsdf_hip_upload of rgb and save/load are refused (the reference's own
 *                   serialisation of this class writes one byte of each float, octree.cpp:417-433).
 *   LAB             LABNode (octree.cpp:531-551): float running means of the CIE L*a*b* image of each pixel
 *                   (RGB2LAB, octree.cpp:436-481); the colour read back is LAB2RGB of the means
 *                   (octree.cpp:483-527).  Three more float planes, float weights, a plain kernel, no rgb
 *                   upload and no save/load, like RGB_NORMALIZED.  Both conversions go through std::pow in
 *                   the reference.  Here the sRGB curve (a function of one byte) is tabulated by the host's
 *                   own libm at create, and the cube roots run on the device in fp64 before the same rounding
 *                   to float: the L, A, B state equals the reference's bit for bit for every one of the 2^24
 *                   pixel colours (the GPU tests sweep them all); the bytes LAB2RGB returns may differ by 1
 *                   where (float) * 255 lands within an ulp of an integer (tolerance stated in
 *                   tests/test_lab_gpu.py: +-1, > 99.9 % identical). */
enum {
  TSDF_COLOR_RGB = 0,
  TSDF_COLOR_RGB_NORMALIZED = 1,
  TSDF_COLOR_LAB = 2
};

/* Everything TSDFVolumeOctree's setters configure before reset()
 * (src/lib/tsdf_volume_octree.cpp:54-85 defaults, :92-199 setters). */
typedef struct tsdf_params {
  int32_t res[3];             /* setResolution            tsdf_volume_octree.cpp:92-98   */
  float size[3];              /* setGridSize              :110-116 (metres)              */
  float max_dist_pos;         /* setDepthTruncationLimits :146-151                       */
  float max_dist_neg;
  float max_weight;           /* setWeightTruncationLimit :163-167                       */
  float min_sensor_dist;      /* setSensorDistanceBounds  tsdf_volume_octree.h:185-190   */
  float max_sensor_dist;
  double fx, fy, cx, cy;      /* setCameraIntrinsics      :176-186 (double, as stored)   */
  int32_t image_width;        /* setImageSize             :128-133                       */
  int32_t image_height;
  int32_t integrate_color;    /* setIntegrateColor        tsdf_volume_octree.h:172-173   */
  int32_t xform_order;        /* TSDF_XFORM_*                                            */
  int32_t z_begin, z_end;     /* Z-slab owned by this handle; 0,0 => whole grid          */
  int32_t halo;               /* extra planes kept below z_begin and above z_end         */
  int32_t device;             /* HIP ordinal, -1 => current device                       */
  int32_t layout;             /* TSDF_LAYOUT_*                                           */
  int32_t color_mode;         /* TSDF_COLOR_*: setColorMode, tsdf_volume_octree.h:290    */
} tsdf_params;

/* Fill *p with the reference constructor defaults (tsdf_volume_octree.cpp:54-85). */
void tsdf_hip_default_params(tsdf_params *p);

/* reset() -- tsdf_volume_octree.cpp:201-219: allocate the grid, every voxel (d=-1, w=0).
 * tsdf_hip_reset on a handle in use erases the voxels, the "band seen" flags and the implied-distance record, and drops the
 * distance field of tsdf_hip_esdf and the normals of tsdf_hip_march_normals.  The soup of the last tsdf_hip_march, the
 * indexed mesh made from it and the list of tsdf_hip_occupied are plain data and STAY on the handle: the fetches keep
 * returning the meshes of the volume as it was, and tsdf_hip_occupied_fetch names the same voxels and gathers the reset
 * values (d = -1, w = 0).  tsdf_hip_destroy ends everything. */
int tsdf_hip_create(const tsdf_params *p, tsdf_handle *out);
int tsdf_hip_reset(tsdf_handle h);
int tsdf_hip_destroy(tsdf_handle h);

/* One volume over several GPUs of ONE node, in one process, behind the same handle type -- the drop-in form of the
 * Z-slab partition: the handle owns n_devices Z-slab handles (contiguous, balanced ranges of z planes, one per entry
 * of `devices`, which may repeat an ordinal), each with tsdf_hip_render_halo(p) halo planes, and EVERY entry point
 * below that takes a handle works on it:
 *   integrate*      the frame fans out to every slab (from pinned host memory over each GPU's own PCIe link, or from
 *                   the GPU that holds it by peer copy over xGMI) and every slab integrates its own planes; no voxel
 *                   crosses a link.  n_observed is the sum over the slabs.
 *   march / fetch   one plane of halo per slab from its upper neighbour (peer copy), the slabs mesh concurrently, the
 *                   triangle lists are merged by the reference's order; the merged mesh lives on the host.
 *   raycast*        ray hand-off between the slabs on COMPACT lists: each slab keeps only the rays it is responsible
 *                   for and advances them on its own stream; a ray that needs another slab's voxel travels there
 *                   point-to-point (96 B), a finished ray goes to the first slab (36 B), which assembles the image
 *                   and applies the camera transform; tsdf_hip_multi_render_stats reports what moved.
 *   sample, lookup_rgb, download, upload, save, reset, synchronize, set_weighting, centers, layout: as for one handle.
 * Not available on such a handle (TSDF_HIP_E_UNSUPPORTED): set_stream, device_planes, get/set_planes_device,
 * raycast_begin/advance*, march_fetch_device -- they expose ONE device's memory.
 * p->z_begin / z_end must be 0 (the whole grid); p->device is ignored.  Every slab works on its own non-blocking
 * stream (also when ordinals repeat), every cross-slab dependency is an event.  Results are bit-identical to one
 * handle holding the whole grid -- tested with repeated ordinals on one GPU and, where more than one GPU is visible,
 * with distinct ordinals (tests/test_multi_gpu.py); the latter has not run on this project's one-GPU test boxes.  cpu_tsdf::TSDFVolumeOctree::setDevices() is the C++ face of it;
 * cpu_tsdf_amd/zslab.py is the multi-PROCESS form of the same partition (one rank per GPU, RCCL). */
int tsdf_hip_create_multi(const tsdf_params *p, const int32_t *devices, int n_devices, tsdf_handle *out);
/* Number of Z-slab handles behind h (1 for an ordinary handle) and the device / owned planes / halo of slab k. */
int tsdf_hip_slab_count(tsdf_handle h);
/* Report-only, multi-GPU handles: of the last tsdf_hip_raycast* call -- out[0] rounds, out[1] ray records handed from one
 * slab to another, out[2] bytes that moved between slabs (hand-offs + finished rays to the first slab), out[3] host
 * waits (one per slab and round: the slabs of a round run concurrently). */
int tsdf_hip_multi_render_stats(tsdf_handle h, uint64_t out[4]);
/* Report-only, multi-GPU handles: how the slabs reach each other.  Copies between two slabs' GPUs (the frame fan-out of
 * the device entry points, halo planes, ray records) are hipMemcpyPeerAsync where the driver grants peer access; a pair
 * it refuses -- said once on stderr at create -- goes through a pinned relay buffer on the host instead (device -> host
 * on the source GPU, host -> device on the receiver's stream, every step ordered by events: slower, never a hang).
 * TSDF_HIP_NO_PEER=1 in the environment at create routes EVERY cross-slab copy that way (how a one-GPU box tests it).
 * out[0] = refused device pairs, out[1] = 1 if everything is relayed, out[2] = bytes relayed since create. */
int tsdf_hip_multi_link_stats(tsdf_handle h, uint64_t out[3]);
/* Report-only, multi-GPU handles: per-slab k_integrate time.  While enabled, every slab's integrate launch is bracketed
 * by HIP events on that slab's stream; tsdf_hip_multi_kernel_ms synchronises slab k and returns the summed milliseconds
 * and the number of launches since timing was enabled (or last read).  With frame pairing and tsdf_hip_integrate_device2
 * the launches are the sweeps slab k really ran: 1 for a pair it fused, 2 for a pair it did not, 1 for a frame launched
 * on its own, none while a frame waits for its partner (the brackets then include the wait for the frame's copy). */
int tsdf_hip_multi_timing(tsdf_handle h, int enable);
int tsdf_hip_multi_kernel_ms(tsdf_handle h, int k, float *ms_sum, int32_t *launches);
int tsdf_hip_slab_info(tsdf_handle h, int k, int32_t *device, int32_t *z_begin, int32_t *z_end, int32_t *halo);

/* Host memory and the boundary.  Every entry point that takes or returns HOST arrays moves them through a pinned
 * two-slot bounce buffer owned by the handle (one extra host memcpy, the same cost whatever memory the caller hands
 * over) -- unless the caller's buffer is itself pinned or registered (hipHostMalloc, hipHostRegister, or
 * tsdf_hip_host_alloc below): that is detected (hipPointerGetAttributes) and the DMA engine reads / writes it
 * directly.  tsdf_hip_host_alloc gives callers without HIP of their own (the C++ shell, ctypes) such memory. */
int tsdf_hip_host_alloc(size_t bytes, void **out);
int tsdf_hip_host_free(void *p);

/* Work is queued on this hipStream_t (default: the null stream). */
int tsdf_hip_set_stream(tsdf_handle h, void *hip_stream);
int tsdf_hip_synchronize(tsdf_handle h);

/* integrateCloud -- include/cpu_tsdf/impl/tsdf_volume_octree.hpp:48-103 (+ updateVoxel :113-218).
 *   depth        image_height x image_width floats, row-major: pt.z of cloud(u,v); NaN = no return.
 *   bgra         same shape, 4 bytes/pixel in PCL PointXYZRGBA memory order (b,g,r,a); NULL unless
 *                integrate_color.
 *   cam_from_vol 3x4 row-major float: trans.inverse().cast<float>() exactly as hpp:54 computes it.
 *   n_observed   optional: number of voxels that reached addObservation this frame.
 * The host variant copies the frame to the device and synchronises; the device variant takes
 * device pointers, is asynchronous on the handle's stream and only synchronises when
 * n_observed != NULL.  The caller's device buffers must be complete when the call is made and stay untouched until
 * the work has finished (tsdf_hip_synchronize or any synchronising call): on a multi-GPU handle the other GPUs copy
 * the frame from them on their own streams. */
int tsdf_hip_integrate(tsdf_handle h, const float *depth, const uint8_t *bgra,
                       const float cam_from_vol[12], uint64_t *n_observed);
int tsdf_hip_integrate_device(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra,
                              const float cam_from_vol[12], uint64_t *n_observed);
/* Pipelined form of tsdf_hip_integrate for a stream of host frames: the frame is copied into a pinned
 * two-slot ring and the call returns; the upload overlaps the previous frame's kernel, so frames flow at the
 * kernel's rate.  The caller's buffers may be reused as soon as the call returns.  Same results; ordered
 * before every later call on this handle; asynchronous errors surface at the next synchronising call. */
int tsdf_hip_integrate_async(tsdf_handle h, const float *depth, const uint8_t *bgra,
                             const float cam_from_vol[12]);
/* The two halves of tsdf_hip_integrate_async, for a caller that can WRITE its frame straight into the pinned slot
 * (the C++ integrateCloud template strips the z / b,g,r fields of a pcl::PointCloud into it, in parallel) instead of
 * building planar images first: _begin returns the slot's host pointers (*depth: image_height x image_width floats,
 * *bgra: as many 4-byte pixels, NULL without integrate_color), waiting only for the kernel that read the slot two frames
 * ago; _commit uploads and queues the integrate launch, as tsdf_hip_integrate_async does.  One begin per commit. */
int tsdf_hip_frame_begin(tsdf_handle h, float **depth, uint8_t **bgra);
int tsdf_hip_frame_commit(tsdf_handle h, const float cam_from_vol[12]);

/* The `integrate` program's per-cloud preparation -- src/prog/integrate.cpp:559-618 and reprojectPoint
 * :201-207: scale by cloud_units, optionally turn (0,0,0) into NaN, optionally move the cloud by
 * poses[i].inverse() (world_to_cam: the first three rows of that matrix, row-major doubles, computed by
 * the caller's Eigen; NULL = clouds are already in the camera frame), then z-buffer the points into an
 * image_height x image_width organised frame (smallest z wins, the earlier point among equals) using the
 * volume's intrinsics AS FLOATS, as the program does.
 *   xyz / bgra   n points: 3 floats every xyz_stride floats, 4 bytes (b,g,r,a) every bgra_stride bytes
 *                (a PCL PointXYZRGBA array is xyz_stride 8, bgra at byte 16 with bgra_stride 32); bgra may be NULL.
 *   depth_out / bgra_out / n_valid   optional host copies of the frame (NaN = empty pixel) and the number
 *                of filled pixels; with all three NULL the call is asynchronous.
 * The frame stays in the handle; tsdf_hip_integrate_staged integrates it (same as tsdf_hip_integrate_device
 * on it), any number of times.  The staged frame is valid until the next call that writes the handle's frame
 * staging, or until tsdf_hip_reset; after that tsdf_hip_integrate_staged returns TSDF_HIP_E_INVALID ("no organised
 * frame is staged") until the next tsdf_hip_organize.  The writers: tsdf_hip_integrate; tsdf_hip_integrate_device[2]
 * on one handle when the colour image does not lie behind its depth image in one allocation (the repack);
 * tsdf_hip_integrate_device on a multi-GPU set always (the frame is copied into every slab's staging);
 * tsdf_hip_integrate_async / tsdf_hip_frame_commit on a set without frame pairing.  On one handle, and on a set with
 * frame pairing, the pipelined calls go through a ring of their own and leave the staged frame valid, as do
 * tsdf_hip_integrate_device2 on a set and every call that takes no frame (queries, download, upload, raycast, march,
 * shift, the setters). */
int tsdf_hip_organize(tsdf_handle h, const float *xyz, size_t xyz_stride, const uint8_t *bgra,
                      size_t bgra_stride, size_t n, float cloud_units, int zero_nans,
                      const double world_to_cam[12], float *depth_out, uint8_t *bgra_out, uint64_t *n_valid);
int tsdf_hip_integrate_staged(tsdf_handle h, const float cam_from_vol[12], uint64_t *n_observed);

/* Of the last tsdf_hip_integrate* call on this handle that asked for n_observed: out[0] = that count, out[1] = bytes
 * of voxel words whose VALUE changed (4 per distance / weight / colour word, 1 per count byte) -- with the bytes read
 * per observed voxel this is the algorithmic traffic of the chosen HBM layout (bench.py's roofline). */
int tsdf_hip_last_count_detail(tsdf_handle h, uint64_t out[2]);
/* Of the same call: out[0] = observed voxels whose DISTANCE word was not read, because the kernel could tell it from the
 * voxel's observation count (PACKED layout: in a cell of 64 x 4 x 1 voxels that no frame since the reset has observed
 * inside the truncation band, an observed voxel sits at max_dist_pos / max_dist_neg and an unobserved one at the reset
 * value) -- 4 bytes each that the launch did not move; out[1] = 1 if the launch was allowed to do so;
 * out[2] = bytes of the voxel planes the launch REQUESTED (it asks for a quad's words together with the frame pixels, so
 * also for quads none of whose voxels turns out to be observed; 0 for the plain kernels, which do not count). */
int tsdf_hip_last_read_detail(tsdf_handle h, uint64_t out[3]);

/* The two observation weightings of updateVoxel -- include/cpu_tsdf/impl/tsdf_volume_octree.hpp:200-204.  The
 * reference has no setter for them: weight_by_depth_ / weight_by_variance_ only become true through load()
 * (src/lib/tsdf_volume_octree.cpp:265-266); tsdf_hip_load applies what the file says.
 *   weight_by_depth     w_new *= (1 - std::min(pt.z / 10., 1.)) (:201-202).  Weights are then no longer counts:
 *                       needs the F32W layout (E_UNSUPPORTED on a PACKED handle; tsdf_hip_load with layout AUTO
 *                       picks F32W by itself) and TSDF_COLOR_RGB.  Integrated by a plain per-voxel kernel (exact
 *                       fp64 projection, IEEE divisions), every operation in the reference's order.
 *   weight_by_variance  w_new *= exp(logNormal(d_new, d, variance)) once a voxel has more than 5 samples (:203-204),
 *                       from OctreeNode::M_ / nsample_ (src/lib/octree.cpp:160-161,281-287): two more planes per voxel
 *                       (float M, int32 nsample), allocated when the flag is first set, zero like a fresh octree's,
 *                       updated by every observation integrated WHILE THE FLAG IS ON, carried by tsdf_hip_save /
 *                       tsdf_hip_load in the node records the reference keeps them in, and readable / writable through
 *                       tsdf_hip_*_variance_state.  A handle that has the planes and is switched back
 *                       (tsdf_hip_set_weighting(h, x, 0)) keeps them -- reset, shift and the block transfers go on
 *                       moving them; tsdf_hip_save writes them only while the flag is on -- but its frames no longer
 *                       update them: M / nsample stay what they were until the flag is set again.  (The reference updates them on every observation whatever
 *                       the flag says; it has no setter, so no sequence of its calls reaches this state.)  Needs
 *                       the F32W layout and TSDF_COLOR_RGB like weight_by_depth (tsdf_hip_load with AUTO picks F32W);
 *                       integrated by the same plain kernel.  std::exp(float) is the host libm's expf restated on the
 *                       device (glibc's table algorithm, in the FMA or the plain build's form, whichever this host
 *                       runs): equal on every float in +-(2^-26 .. 104), which tests/test_wvar_gpu.py sweeps. */
int tsdf_hip_set_weighting(tsdf_handle h, int weight_by_depth, int weight_by_variance);

/* OctreeNode::M_ / nsample_ of a block of voxels ([z][y][x]; either pointer may be NULL) -- include/cpu_tsdf/octree.h:
 * 164-165, the state weight_by_variance integrates with.  Only volumes that weight by variance keep it (E_INVALID
 * otherwise).  The reference exposes the members directly; tsdf_hip_save / tsdf_hip_load move them with the file. */
int tsdf_hip_download_variance_state(tsdf_handle h, int x0, int y0, int z0, int nx, int ny, int nz, float *M, int32_t *nsample);
int tsdf_hip_upload_variance_state(tsdf_handle h, int x0, int y0, int z0, int nx, int ny, int nz, const float *M,
                                   const int32_t *nsample);

/* renderView -- tsdf_volume_octree.cpp:278-421 (everything except the last line).
 *   rot        3x3 row-major float:  trans.rotation().cast<float>()      (:303)
 *   origin     3 floats:             trans.translation().cast<float>()   (:304)
 *              Both are computed by the caller with its own Eigen so the kernel sees exactly the
 *              numbers the reference would (Affine3d::rotation() runs an SVD inside Eigen).
 *   downsample downsampleBy
 *   out        (image_height/ds) x (image_width/ds) x 8 floats per pixel:
 *              x,y,z, nx,ny,nz, t_star, iterations -- in the VOLUME frame; the reference's final
 *              transformPointCloudWithNormals by trans^-1 (:422) is applied by the host shell.
 *              A miss has NaN x,y,z and a zero normal (PointNormal's default constructor). */
int tsdf_hip_raycast(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                     float *out);
/* The same with the reference's last line (:422) done in the kernel: cam_from_vol = the first three rows of
 * trans.inverse().matrix() (row-major doubles, from the caller's Eigen); points and normals come back in the
 * CAMERA frame, as renderView returns them.  For callers without PCL (the Python binding). */
int tsdf_hip_raycast_camera(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                            const double cam_from_vol[12], float *out);

/* renderView across Z-slab handles (one handle per GPU): ray hand-off.  The reference's ray loop
 * (tsdf_volume_octree.cpp:313-369) chooses each step from the voxel it last visited, so the loop state of a
 * ray travels between the slabs it crosses instead of the voxels.  One record of
 * TSDF_HIP_RAY_RECORD_INTS 32-bit words per ray, in DEVICE memory, row-major like the image:
 *   [0] status (1 suspended, 2 finished; 0 = "not touched" in a delta buffer)   [1] global z plane of the
 *   voxel the ray needs next, -1 before it needed any   [2] iterations   [3] hit_voxel   [4] t   [5..7] pt
 *   [8] last_d   [9] last_w   [10] step   [11] the ray's pixel index   [12] finish flag (the march is done, [4]
 *   holds t_star and only the normal is left: a hit whose extrapolated point lies in another slab)   [13..15] zero
 *   [16..23] the 8 output floats of tsdf_hip_raycast.
 * tsdf_hip_raycast_begin   writes the start record of every ray (identical on every rank).
 * tsdf_hip_raycast_advance zero-fills d_delta, then resumes every suspended ray of d_state that this
 *   handle is responsible for (needed plane inside its OWNED slab; or ray index % world == rank while the
 *   ray has not needed a voxel yet) until it finishes or needs another slab's voxel, and writes the new
 *   record to d_delta.  Exactly one rank touches a ray per round, so the caller merges with an integer
 *   SUM all-reduce of the deltas (RCCL) and overwrites the records whose status word is non-zero; it
 *   repeats until no record is suspended (at most world + 2 rounds).  The refinement walk and the trilinear samples of a hit read up
 *   to tsdf_hip_render_halo(params) planes beyond the owned slab: create the handles with that halo and
 *   refresh it (tsdf_hip_get/set_planes_device) before rendering.  Synchronises the stream. */
#define TSDF_HIP_RAY_RECORD_INTS 24
int tsdf_hip_raycast_begin(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                           int32_t *d_state);
int tsdf_hip_raycast_advance(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                             int rank, int world, const int32_t *d_state, int32_t *d_delta);
/* Scalable form: the caller keeps, per rank, a COMPACT list of the records it is responsible for (word 11 of a
 * record is the ray's pixel index, set by tsdf_hip_raycast_begin) and advances it in place; suspended records then
 * travel point-to-point to the owner of their next voxel, finished ones stay.  Traffic is proportional to the
 * rays that cross a slab boundary instead of to the image. */
int tsdf_hip_raycast_advance_list(tsdf_handle h, const float rot[9], const float origin[3], int downsample,
                                  int rank, int world, int32_t *d_records, size_t count);
int tsdf_hip_render_halo(const tsdf_params *p);

/* Placement of the voxel planes (not in the reference).  On MI355X the physical pages behind an allocation decide how
 * fast a streaming read-modify-write of it runs (a 2048^3 volume integrates in 17.9 ms or in 18.4-19.0 ms depending on
 * the allocation), so tsdf_hip_create allocates the planes of a volume of 4 GiB or more up to
 * `alloc_tries` times (TSDF_HIP_ALLOC_TRIES in the environment, default 3, 1 = off; a second candidate is only
 * tried while it fits next to the first), sweeps each candidate once and keeps the fastest.  The search ends early
 * at a candidate that streams at >= 5.55 TB/s (the fastest class) and goes on for up to alloc_tries more (8 at most)
 * while none has reached 5.15 TB/s.  This reports what happened: ms[i] = probe sweep of candidate i (negative = not
 * probed), *chosen = the one kept; returns the number of candidates tried. */
int tsdf_hip_alloc_probe(tsdf_handle h, float ms[8], int32_t *chosen);

/* The reference's integrateCloud visits only the voxels pcl::FrustumCulling keeps (getFrustumCulledVoxels,
 * tsdf_volume_octree.cpp:619-652, called at impl/tsdf_volume_octree.hpp:93-94): a pyramid of 1.1 x the field of view
 * AROUND THE OPTICAL AXIS between near = min_sensor_dist and far = max_sensor_dist, tested per voxel centre as
 * `pt.dot(plane) <= 0` for six planes (pt = (x, y, z, 1), the dot reduced as (p0 + p1) + (p2 + p3), fp32, no FMA).
 * For an ordinary camera that pyramid contains every ray of the image and the cull only removes voxels updateVoxel
 * rejects anyway; with a principal point more than ~10 % off centre, or a range plane cutting the volume, it decides
 * voxels.  To integrate exactly the reference's voxels in EVERY regime, hand the six planes of the frame's pose to
 * tsdf_hip_set_reference_cull before each integrate call -- cpu_tsdf::TSDFVolumeOctree::integrateCloud and the Python
 * binding do so by default (setReferenceCull(false) opts out).
 *   planes  l, r, t, b, far, near (the order of PCL's test), 4 floats each, in the VOLUME frame.  They are PCL / Eigen
 *           arithmetic on the forward pose `trans` (pcl::FrustumCulling::applyFilter with camera pose
 *           trans.cast<float>() * cam2robot, tsdf_volume_octree.cpp:633-646), so the caller computes them: the C++
 *           shell with the caller's Eigen, anyone else with tsdf_hip_reference_cull_planes.  NULL = no cull (the
 *           conservative superset: every voxel updateVoxel itself accepts).
 * Cost: none when the planes provably keep every voxel of the slab (eight corner voxels, evaluated per launch on the
 * host: the usual case -- the launch is then the ordinary one); otherwise the frame's ROW INTERVALS carry the cull
 * (k_rows: per voxel row the exact x range the six planes keep, found by bisection on the very float expression of the
 * per-voxel test) and k_integrate masks by interval -- a few per cent.  Non-finite planes and the RGB_NORMALIZED / LAB
 * kernels test the six planes per voxel.  The planes stay in force for every later integrate call on the handle: set
 * them per frame.  tests/test_oracle_golden.py pins the restatement against the compiled reference,
 * tests/test_index_box.py the intervals and tests/test_integrate_gpu.py the kernels against the restatement. */
int tsdf_hip_set_reference_cull(tsdf_handle h, const float planes[24]);
/* Two frames in one sweep (not in the reference; its integrateCloud takes one cloud).  Integrates frame A, then frame B
 * -- the same voxels, bit for bit, as two tsdf_hip_integrate_device calls in that order -- but where the handle and both
 * poses allow it (PACKED layout, nx a multiple of 4, every voxel of the slab inside the sensor range and the image for
 * BOTH poses: the camera-outside-the-volume case; the cull planes keeping the whole slab) one kernel reads each voxel's
 * words once, applies updateVoxel for A and then for B in registers and writes them back once: half the HBM bytes per
 * frame (k_integrate2).  Otherwise it IS two launches.  planes_a / planes_b: as
 * tsdf_hip_set_reference_cull (NULL = none); the handle keeps frame B's.  n_observed (nullable, 2 values): per frame, as
 * the single call reports; tsdf_hip_last_count_detail then describes the pair.  *fused (nullable): 1 if one sweep did
 * it.  Each frame's colour image must lie behind its depth image in one allocation (as tsdf_hip_integrate_device
 * prefers); device pointers, asynchronous unless n_observed.  On a multi-GPU set both frames go to every slab's ring
 * and every slab decides for itself; *fused = 1 when every slab swept once, n_observed = the slabs' sums. */
int tsdf_hip_integrate_device2(tsdf_handle h, const float *d_depth_a, const uint32_t *d_bgra_a, const float cam_from_vol_a[12],
                               const float *planes_a, const float *d_depth_b, const uint32_t *d_bgra_b,
                               const float cam_from_vol_b[12], const float *planes_b, uint64_t *n_observed, int32_t *fused);

/* Frame pairing for the pipelined host entry points (tsdf_hip_frame_begin / _commit, tsdf_hip_integrate_async); not in the
 * reference.  While on, a committed frame is uploaded at once but its kernel launch waits: when the NEXT frame is
 * committed the two are integrated by one tsdf_hip_integrate_device2-style call (one sweep of the volume for both where
 * the handle and both poses allow it, else two launches, frame order kept either way); any other entry point that reads
 * or writes the volume (synchronize, integrate, download, march, raycast, sample, save, reset, ...) first launches a
 * waiting frame on its own.  Results are identical to pairing off; what changes is when the kernels run (a stream of
 * frames: 11.2 instead of 12.7 ms per frame at 2048^3 + colour; without colour a pair is two launches of
 * the pipelined single-frame kernel, which is the faster way there since round 6).  Each frame keeps the cull planes that
 * were in force (tsdf_hip_set_reference_cull) when IT was committed.  Off by default.  On a multi-GPU set
 * (tsdf_hip_create_multi, round 6) every slab pairs the frames of its own ring: one sweep of a slab per pair where both
 * poses see all of THAT slab. */
int tsdf_hip_set_frame_pairing(tsdf_handle h, int on);

/* Host only: those six planes from the forward pose `trans` (row-major 4x4 doubles, camera -> volume, what
 * integrateCloud is called with) and the camera of `p` [PCL-recall: filters/impl/frustum_culling.hpp]. */
int tsdf_hip_reference_cull_planes(const tsdf_params *p, const double trans[16], float planes[24]);
/* 1 if that cull cannot change results for ANY pose with these parameters as far as the field of view goes (the
 * culling pyramid contains every ray of the image and max_sensor_dist is finite and moderate); 0 for a principal point
 * so far off centre, or a range so large (>= 1e15, inf), that the reference drops voxels which project into the image.
 * Report-only since the planes are applied per launch. */
int tsdf_hip_reference_cull_is_noop(const tsdf_params *p);

/* getFxn / getGradient / getHessian -- tsdf_volume_octree.cpp:655-828, batched.
 *   xyz n x 3 floats; val n floats (nullable); grad n x 3 (nullable); hess n x 9 row-major (nullable);
 *   ok n bytes: 1 where the reference returns true.  A Z-slab handle answers only for points whose lower-corner
 *   plane it owns (exactly one handle of a partition does; it needs plane z_end fresh in its halo). */
int tsdf_hip_sample(tsdf_handle h, const float *xyz, size_t n, float *val, float *grad,
                    float *hess, uint8_t *ok);

/* renderColoredView's colour lookup -- tsdf_volume_octree.cpp:443-448: for n points (volume frame) the voxel
 * Octree::getContainingVoxel returns (src/lib/octree.cpp:112-133,628-643) and its RGBNode colour (r,g,b; zeros
 * if the volume stores no colour).  found[i] = 0 where the reference gets NULL. */
int tsdf_hip_lookup_rgb(tsdf_handle h, const float *xyz, size_t n, uint8_t *rgb, uint8_t *found);

/* alignCloud -- NOT IN THE REFERENCE.  The reference has getFxn / getGradient so that a caller can optimise a pose against
 * the signed distance field; these entry points do that for a whole cloud on the device.
 *
 * tsdf_hip_align_system: the normal equations of  min_xi  sum_i getFxn(exp(xi) * T * p_i)^2  at xi = 0.
 *   xyz n x 3 floats (source frame); vol_from_src the rows of T = [R | t], cast to float as the reference casts poses
 *   (trans.cast<float>(), hpp:76).  Per point: q = R p + t in fp32, each row ((R0*p.x + R1*p.y) + R2*p.z) + t; val, g and
 *   ok are getFxnAndGradient of q, bit for bit what tsdf_hip_sample returns.
 *   GATE (an extension: the reference's getFxn ignores weights, so never-observed voxels -- d = -1, w = 0 -- would pull
 *   on the pose): a point is USED iff ok, all eight neighbour voxels have weight > min_weight (strictly; any layout), and
 *   fabsf(val) < r_max (a NaN fails).
 *   Terms, in fp64 from the float inputs: J = [q x g, g], the left-multiplied twist (omega, v) in the volume frame
 *   (r(exp(xi) q) ~ r + omega . (q x g) + v . g), r = val.  out[0..20] = the upper triangle of sum J J^T, row-major;
 *   out[21..26] = sum J r; out[27] = sum r^2; out[28] = the number of used points.
 *   used (n bytes, nullable) and xyz_vol (n x 3 floats, nullable) receive the gate's verdict and q per point.
 *   The summation order is a function of n alone (no floating-point atomics): two calls return identical bytes, and so
 *   do the host-pointer and the _device form.  A multi-GPU set exchanges the one-plane halo, every slab sums the points
 *   whose lower-corner plane it owns, the host adds the slab sums in slab order; `used` is the OR.
 * tsdf_hip_align_system_device: the cloud is already on the handle's device; synchronises the handle's stream for `out`.
 *   TSDF_HIP_E_UNSUPPORTED on a multi-GPU set.
 * tsdf_hip_align: Gauss-Newton around it.  Uploads the cloud once; per iteration runs the system kernels (232 bytes come
 *   back), solves the 6 x 6 by Cholesky in fp64 on the host, and updates T <- exp(delta) * T with the closed-form SE(3)
 *   exponential (Rodrigues; series below |omega| = 1e-12).  Stops after max_iterations steps or when |delta|_2 < min_step.
 *   iterations (nullable) receives the number of steps taken; cost_log (nullable, 2 * max_iterations doubles) sum r^2
 *   and the used count of every system it evaluated (entries beyond that are left alone).
 *   Returns TSDF_HIP_E_INVALID for n = 0, a NULL xyz / guess / refined, r_max <= 0 or NaN, a NaN min_weight,
 *   max_iterations < 1, min_step < 0 or NaN -- before any device is touched.  Returns TSDF_HIP_ALIGN_NO_POINTS where no
 *   point is used and TSDF_HIP_ALIGN_RANK_DEFICIENT where the factorisation fails (a pivot not above 1e-10 of the largest
 *   diagonal entry: a single plane); refined then holds the pose of the last good step (the guess, if none).
 * tsdf_hip_align_stats: report-only, of the last of the calls above on this handle: points, used (of the last system),
 *   iterations (steps; 0 for the system calls), device microseconds of the system kernels (handle's stream events).
 * Like every entry point that reads the volume, all of them first launch a frame held back by frame pairing. */
int tsdf_hip_align_system(tsdf_handle h, const float *xyz, size_t n, const double vol_from_src[12],
                          float min_weight, float r_max, double out[29], uint8_t *used, float *xyz_vol);
int tsdf_hip_align_system_device(tsdf_handle h, const float *d_xyz, size_t n, const double vol_from_src[12],
                                 float min_weight, float r_max, double out[29]);
int tsdf_hip_align(tsdf_handle h, const float *xyz, size_t n, const double guess[12], float min_weight, float r_max,
                   int max_iterations, double min_step, double refined[12], int32_t *iterations, double *cost_log);
int tsdf_hip_align_stats(tsdf_handle h, uint64_t out[4]);

/* MarchingCubesTSDFOctree::reconstruct -- src/lib/marching_cubes_tsdf_octree.cpp:108-236
 * (+ pcl::MarchingCubes::createSurface).  color_mode: 0 none, 1 setColorByRGB, 2 setColorByConfidence.
 * tsdf_hip_march runs the kernels and reports the triangle count; tsdf_hip_march_fetch copies
 * n_tri*9 floats (3 vertices, volume frame) and, if rgb != NULL, n_tri*9 bytes (r,g,b per vertex) and,
 * if cell != NULL, n_tri uint64 cell keys ((x<<42)|(y<<21)|z of the base voxel).  Triangles come
 * out in the reference's order (octree pre-order = Morton order with x as the high bit). */
int tsdf_hip_march(tsdf_handle h, float w_min, int color_mode, uint64_t *n_tri);
int tsdf_hip_march_fetch(tsdf_handle h, float *verts, uint8_t *rgb, uint64_t *cell);
/* Report-only: device milliseconds of the last tsdf_hip_march by phase -- ms[0] classify (k_mc_classify), ms[1] count
 * read-back + sort + scan, ms[2] emit (k_mc_emit) -- and the number of active cells. */
int tsdf_hip_march_timing(tsdf_handle h, float ms[3], uint64_t *n_cells);
/* Report-only: out[0] active cells, out[1] triangles, out[2] bytes of the distance plane the classify pass of the last
 * tsdf_hip_march REQUESTED (with the band flags of integrateCloud deciding, it reads only the quads an in-band
 * observation is near: src/lib/marching_cubes_tsdf_octree.cpp:179-236 visits every leaf), out[3] bit 0: the flags were
 * in use (0: every plane was read -- after an upload / load the flags say nothing until reset); out[3] bit 1: the
 * weight test (marching_cubes_tsdf_octree.cpp:98, w < w_min) was not evaluated because it could not fail -- PACKED counts,
 * planes written only by integrateCloud since the reset, no halo plane, w_min <= min(1, max_weight): a corner with
 * |d| < 1 has been observed, and an observation counts.  On a multi-GPU set out[0..2] are the sums over the slabs and
 * out[3] is combined bit by bit: a bit is set when EVERY slab set it.  (The slabs of a set leave the weight test out on
 * their halo plane too, while all slabs' planes were written only by integrateCloud since the reset: the halo is then a
 * fresh copy of such a plane.) */
int tsdf_hip_march_stats(tsdf_handle h, uint64_t out[4]);
/* The same copies into DEVICE buffers of the caller, asynchronous on the handle's stream (multi-GPU mesh merge:
 * the buffers go straight to RCCL). */
int tsdf_hip_march_fetch_device(tsdf_handle h, float *d_verts, uint8_t *d_rgb, uint64_t *d_cell);

/* cleanupMesh -- src/prog/integrate.cpp:152-214 (the `integrate` program's --cleanup): which faces of a triangle mesh
 * survive the removal of small islands.  Two faces are LINKED when their centroids -- ((v0 + v1) + v2) / 3.f per
 * component, in float -- lie in neighbouring cells (the 27 around a face's own) of a grid of edge face_dist, cell =
 * floor((double)c / (double)face_dist), and (ex*ex + ey*ey) + ez*ez < (float)((double)face_dist * face_dist) in float,
 * strictly.  A face is removed iff its connected group of linked faces has at most min_neighbors members; a face whose
 * centroid is not finite links to nothing and is a group of one.  keep[f] (one byte per face, 1 = survives) equals, face
 * for face, what cpu_tsdf::mesh_post::cleanupMesh (csrc/prog/mesh_post.h) drops on the host.
 *   verts, faces   HOST arrays (pinned memory is used directly): n_verts x 3 floats, n_faces x 3 vertex indices;
 *                  faces == NULL = triangle soup, face f using vertices 3f, 3f + 1, 3f + 2.
 * E_INVALID: face_dist not finite or <= 0, min_neighbors < 0, more than 2^31 faces (face indices are 32-bit), a vertex
 * index >= n_verts, NULL where data is needed.  n_faces == 0 is OK and touches no device.
 * Cost: a face evaluates link tests until it has min_neighbors links, so at most (faces in its 27 cells) tests, and on a
 * surface a few times min_neighbors.  A min_neighbors in the range of the cell population on a dense mesh (thousands, with
 * hundreds of faces per cell) makes every face walk all its candidates in ONE kernel launch -- as slow as the host pass per
 * face, and long enough to matter on a GPU shared with others; the defaults of the reference (0.02, 5) are far from it. */
int tsdf_hip_mesh_cleanup(int device, const float *verts, uint64_t n_verts, const uint32_t *faces /* NULL = soup */,
                          uint64_t n_faces, float face_dist, int min_neighbors, uint8_t *keep, uint64_t *n_kept);
/* The same on the DEVICE-RESIDENT result of the last tsdf_hip_march, in place (integrate.cpp:152-214 applied before the
 * mesh leaves the GPU; an extension: the reference cleans the final PolygonMesh on the host): vertices, colours and cell
 * keys are compacted together, order kept; tsdf_hip_march_fetch / _fetch_device then return the *n_tri surviving
 * triangles.  E_INVALID before the first tsdf_hip_march on the handle, and after one that failed.  A second call with the same arguments removes
 * nothing.  On a multi-GPU handle the merged mesh (host) goes through tsdf_hip_mesh_cleanup on the first slab's device;
 * the result equals one handle holding the whole grid. */
int tsdf_hip_march_cleanup(tsdf_handle h, float face_dist, int min_neighbors, uint64_t *n_tri);
/* Report-only, of the last cleanup (either entry point) on the calling thread: out[0] = faces in, out[1] = faces removed,
 * out[2] = link tests evaluated (the host pass of integrate.cpp:173-206 evaluates one per candidate of every face; here a
 * face stops at min_neighbors links), out[3] = device microseconds: the two intervals of device work (HIP events on the
 * stream) before and after the host reads the cell count in between; that read and all transfers are excluded. */
int tsdf_hip_mesh_cleanup_stats(uint64_t out[4]);

/* flattenVertices -- src/prog/integrate.cpp:103-150 (the `integrate` program's --flatten), as
 * cpu_tsdf::mesh_post::flattenVertices (csrc/prog/mesh_post.h) defines it: the vertices closer than min_dist are merged and
 * the faces re-indexed.  Two vertices are NEIGHBOURS when both are finite, lie in neighbouring cells (the 27 around a
 * vertex's own) of a grid of edge min_dist, cell = floor((double)v / (double)min_dist), and
 * (ex*ex + ey*ey) + ez*ez < min((float)((double)min_dist * min_dist), min_dist) in float, strictly (the reference compares
 * the SQUARED distance with min_dist once more, :124).  The host pass visits the vertices in index order; its result is a
 * function of the input alone, by three rules:
 *   1. vertex i is a SEED -- it opens an output vertex -- iff no earlier seed is its neighbour.  A vertex that is not finite
 *      has no neighbour, not even itself: always a seed.
 *   2. remap[j] of a seed is its own output vertex; of any other vertex, the output vertex of the HIGHEST-indexed seed
 *      among its neighbours (the loop lets every seed overwrite the entry of every neighbour: the last writer wins).
 *   3. the output index of a seed is the number of seeds before it.
 * Faces are re-indexed through remap; a face with two equal corners is dropped, face order is kept.  Output vertex o is
 * input vertex seeds[o], bit for bit.
 *   verts, faces   HOST arrays (pinned memory is used directly): n_verts x 3 floats, n_faces x 3 vertex indices;
 *                  faces == NULL = triangle soup, face f using vertices 3f, 3f + 1, 3f + 2.
 *   remap          n_verts entries: the output vertex of each input vertex; nullable.
 *   seeds          room for n_verts entries, the first *n_out_verts are filled: the input vertex of each output vertex;
 *                  nullable.
 *   out_faces      room for n_faces x 3 entries, the first *n_out_faces x 3 are filled; nullable.
 * E_INVALID: min_dist not finite or <= 0, device < 0, more than 2^31 vertices or faces (indices are 32-bit), NULL where
 * data is needed (verts; n_out_verts with seeds, n_out_faces with out_faces), a soup with fewer than 3 * n_faces vertices,
 * a face naming a vertex >= n_verts.  All of these but the last are checked before any device call.  n_verts == 0 (with no
 * face) is OK and touches no device.
 * Cost: rule 1 is iterated to its fixed point -- an undecided vertex is merged as soon as one earlier neighbour is a seed,
 * and a seed as soon as all earlier neighbours are merged; one kernel launch per round over the still undecided vertices.
 * Rounds = the depth of the longest index-ordered chain of near vertices: a handful on a marched mesh (its clusters are the
 * 2-8 exact copies of a shared edge vertex), n for n vertices strung out in index order at just under min_dist. */
int tsdf_hip_mesh_flatten(int device, const float *verts, uint64_t n_verts, const uint32_t *faces /* NULL = soup */,
                          uint64_t n_faces, float min_dist, uint32_t *remap, uint32_t *seeds, uint64_t *n_out_verts,
                          uint32_t *out_faces, uint64_t *n_out_faces);
/* The same on the DEVICE-RESIDENT result of the last tsdf_hip_march (after an optional tsdf_hip_march_cleanup; an extension:
 * the reference flattens the final PolygonMesh on the host).  The soup STAYS: the indexed mesh -- *n_verts vertices,
 * *n_faces faces -- lives in buffers of its own, and tsdf_hip_march_fetch / _fetch_device keep returning the soup.
 * E_INVALID before the first tsdf_hip_march on the handle, and after one that failed.  A later tsdf_hip_march or
 * tsdf_hip_march_cleanup invalidates the indexed mesh.  On a multi-GPU handle the merged mesh (host) goes through
 * tsdf_hip_mesh_flatten on the first slab's device; the result equals one handle holding the whole grid. */
int tsdf_hip_march_flatten(tsdf_handle h, float min_dist, uint64_t *n_verts, uint64_t *n_faces);
/* The indexed mesh of the last tsdf_hip_march_flatten (each pointer nullable): verts n_verts x 3 floats (volume frame), rgb
 * n_verts x 3 bytes -- the colour of the output vertex's SEED vertex; an extension: the reference converts to PointXYZ and
 * loses the colours -- faces n_faces x 3 vertex indices, cell[f] the cell key of surviving face f.  E_INVALID while there
 * is no valid indexed mesh, and for rgb after a march without a colour mode. */
int tsdf_hip_march_fetch_indexed(tsdf_handle h, float *verts, uint8_t *rgb, uint32_t *faces, uint64_t *cell);
/* Report-only, of the last flatten (either entry point) on the calling thread: out[0] = vertices in, out[1] = vertices out,
 * out[2] = seed rounds (launches of rule 1 that found an undecided vertex), out[3] = device microseconds from the first
 * kernel to the last (HIP events on the stream; the host's reads of the undecided count between batches of rounds fall
 * inside, the transfers of the host-array entry point do not). */
int tsdf_hip_mesh_flatten_stats(uint64_t out[4]);

/* decimateMesh -- vertex clustering (Rossignac-Borrel); an extension with no counterpart in the reference.  A grid of edge
 * cell_size is laid over the mesh, every occupied cell keeps ONE vertex, and the faces are re-indexed.  The result is
 * defined by the sequential host pass cpu_tsdf::mesh_post::decimateArrays (csrc/prog/mesh_post.h) and equals it bit for bit:
 *   1. a finite vertex belongs to the cell floor((double)v / (double)cell_size) per axis; the vertices of one cell are one
 *      cluster.  A vertex with a component that is not finite is a cluster of its own.  A finite vertex in a cell outside
 *      [-2^20, 2^20) on any axis (the 21-bit cell key would alias) refuses the call: E_INVALID, the text names the extent,
 *      nothing is written.
 *   2. clusters are ordered by their lowest-indexed member; remap[i] is the output index of the cluster of vertex i.
 *   3. the output vertex of a cluster of one is that vertex, bit for bit (NaN payloads survive).  Otherwise, per component, a
 *      double sum starting at +0.0 takes the members one add at a time in ascending input index, is divided by
 *      (double)count and rounded to float once.
 *   4. the colour is (2 * sum + count) / (2 * count) per channel, in integers.
 *   5. faces are re-indexed through remap; a face with two equal corners is dropped; of the remaining faces whose sorted
 *      corner triples are equal, whatever their orientation, only the one with the lowest index survives, as it is.  Face
 *      order is kept.
 *   verts, rgb, faces   HOST arrays (pinned memory is used directly, pageable memory is staged): n_verts x 3 floats,
 *                  n_verts x 3 bytes or NULL, n_faces x 3 vertex indices; faces == NULL = triangle soup, face f using vertices
 *                  3f, 3f + 1, 3f + 2.
 *   remap          n_verts entries; nullable.
 *   out_verts, out_rgb, counts   room for n_verts entries (x 3 floats, x 3 bytes, x 1), the first *n_out_verts are filled:
 *                  position, colour and number of members of each output vertex; each nullable.
 *   out_faces      room for n_faces x 3 entries, the first *n_out_faces x 3 are filled; nullable; may be `faces` itself.
 * E_INVALID: cell_size not finite or <= 0, device < 0, more than 2^31 vertices or faces (indices are 32-bit), NULL where data
 * is needed (verts; rgb with out_rgb; n_out_verts with out_verts / out_rgb / counts; n_out_faces with out_faces), a soup with
 * fewer than 3 * n_faces vertices, a face naming a vertex >= n_verts, the extent of rule 1.  All of these but the last two are
 * checked before any device call.  n_verts == 0 (with no face) is OK and touches no device.  E_NOMEM, with the bytes in
 * tsdf_hip_last_error, when the working set does not fit.
 * Cost: two radix sorts of the faces, one of the vertices, and the reduction of rule 3, in which ONE lane walks each cluster
 * so that the adds keep the host's order: tens to a few hundred members on a marched mesh, but a cell_size that puts all
 * vertices into one cell makes one lane walk the whole mesh in one kernel launch, as slow as the host pass. */
int tsdf_hip_mesh_decimate(int device, const float *verts, const uint8_t *rgb /* nullable */, uint64_t n_verts,
                           const uint32_t *faces /* NULL = soup */, uint64_t n_faces, float cell_size, uint32_t *remap,
                           float *out_verts, uint8_t *out_rgb, uint32_t *counts, uint64_t *n_out_verts, uint32_t *out_faces,
                           uint64_t *n_out_faces);
/* The same on the DEVICE-RESIDENT soup of the last tsdf_hip_march (after an optional tsdf_hip_march_cleanup).  It writes the
 * indexed-mesh buffers tsdf_hip_march_flatten uses: tsdf_hip_march_fetch_indexed then returns the decimated mesh, rgb being
 * rule 4's mean and cell[f] the cell key of surviving face f.  The soup STAYS.  A later tsdf_hip_march, _march_cleanup,
 * _march_flatten or _march_decimate replaces or invalidates the indexed mesh, as documented for flatten.  E_INVALID before
 * the first tsdf_hip_march on the handle, and after one that failed.  On a multi-GPU handle the merged mesh (host) goes
 * through the host-array route on the first slab's device; the result equals one handle holding the whole grid. */
int tsdf_hip_march_decimate(tsdf_handle h, float cell_size, uint64_t *n_verts, uint64_t *n_faces);
/* Report-only, of the last decimate (either entry point) on the calling thread: out[0] = vertices in, out[1] = vertices out,
 * out[2] = faces dropped as duplicates (the degenerate drops are faces in - faces out - out[2]), out[3] = device
 * microseconds from the first kernel to the last (HIP events on the stream; the host's read of the cluster count falls
 * inside, the transfers of the host-array entry point do not). */
int tsdf_hip_mesh_decimate_stats(uint64_t out[4]);

/* smoothMesh -- Taubin's lambda | mu smoothing of an INDEXED mesh (umbrella operator, uniform weights, Jacobi steps); an
 * extension with no counterpart in the reference.  The vertices move, nothing else changes.  The result is defined by the
 * sequential host pass cpu_tsdf::mesh_post::smoothArrays (csrc/prog/mesh_post.h) and equals it bit for bit:
 *   1. N(i), the neighbours of vertex i, are the j != i such that some face has both i and j among its corners, in ascending
 *      index; deg(i) = |N(i)|.  A degenerate face (a, a, b) still contributes a-b; duplicate faces contribute once.
 *   2. the multiplicity of the undirected edge {a, b}, a != b, is the number of corner pairs (0,1), (1,2), (2,0) of all faces
 *      that name it.  A BOUNDARY edge has multiplicity exactly 1 (a face given twice: 2, three faces on one edge: 3 -- neither
 *      is boundary).
 *   3. fixed[i], decided once from the input positions, is the OR of 1: a component of vertex i or of one of its neighbours
 *      is not finite; 2: deg(i) == 0; 4: keep_boundary != 0 and i is an endpoint of a boundary edge.  A vertex with
 *      fixed[i] != 0 keeps its three words bit for bit through every step (NaN payloads and -0.0 survive).
 *   4. one step with factor f (the float widened to double): every vertex reads the positions of the step before.  Per
 *      component of a vertex that is not fixed: a double sum starting at +0.0 takes (double)x_j one add at a time over N(i)
 *      in ascending index, m = s / (double)deg(i), p = (double)x_i, x'_i = (float)(p + f * (m - p)) -- the subtraction, the
 *      product, the sum and the cast each rounded once, no FMA.
 *   5. one iteration is a step with lambda and then, iff mu != 0, a step with mu.  iterations == 0 returns the input.
 *   verts, faces   HOST arrays (pinned memory is used directly, pageable memory is staged): n_verts x 3 floats, n_faces x 3
 *                  vertex indices.  faces is required: a triangle soup shares no vertices -- flatten or decimate first.
 *   out_verts      n_verts x 3 floats; may be `verts` itself.
 *   fixed, degree  n_verts entries each: rule 3's bits and deg(i); each nullable.
 * E_INVALID: lambda not finite or outside (0, 1], mu not finite or outside [-1, 0], iterations outside [0, 1000], more than
 * 2^31 vertices or faces (and more than 715827882 faces: the 6 directed edge entries per face are indexed with 32 bits), NULL
 * verts, out_verts or faces, device < 0, a face naming a vertex >= n_verts (nothing is written then).  All of these but the
 * last are checked before any device call.  n_verts == 0 (with no face) is OK and touches no device.  E_NOMEM, with the bytes
 * in tsdf_hip_last_error, when the mesh or the working set (41 n_verts + 102 n_faces bytes and the sort's temporary storage)
 * does not fit.  (Positions that overflow to infinity in a later step are not fixed: what follows from them is NaN, whose
 * sign and payload are the arithmetic unit's.)
 * Cost: one radix sort of the 6 n_faces directed edge keys builds the neighbour table, once.  Then 1 or 2 kernel launches per
 * iteration, all queued without a host read in between, in which ONE lane walks each vertex's neighbour list so that the
 * adds keep the host's order.  A marched mesh has degree 4-8; a vertex with thousands of neighbours makes one lane walk
 * them all, twice per iteration. */
int tsdf_hip_mesh_smooth(int device, const float *verts, uint64_t n_verts, const uint32_t *faces, uint64_t n_faces,
                         float lambda, float mu, int iterations, int keep_boundary, float *out_verts /* may be verts */,
                         uint8_t *fixed /* nullable */, uint32_t *degree /* nullable */);
/* The same, in place, on the handle's INDEXED mesh: the one the last tsdf_hip_march_flatten or tsdf_hip_march_decimate made.
 * tsdf_hip_march_fetch_indexed then returns the moved vertices; rgb, faces and cell are unchanged, and the soup STAYS.  A
 * second call smooths further.  *n_fixed (nullable): the vertices rule 3 fixed.  E_INVALID while there is no valid indexed
 * mesh (the rules are those documented for flatten: a later tsdf_hip_march or tsdf_hip_march_cleanup invalidates it), and
 * for the arguments as above.  On a multi-GPU handle the host-held merged mesh goes through tsdf_hip_mesh_smooth on the
 * first slab's device; the result equals one handle holding the whole grid. */
int tsdf_hip_march_smooth(tsdf_handle h, float lambda, float mu, int iterations, int keep_boundary, uint64_t *n_fixed /* nullable */);
/* Report-only, of the last smooth (either entry point) on the calling thread: out[0] = vertices, out[1] = unique undirected
 * edges, out[2] = fixed vertices, out[3] = device microseconds from the first kernel to the last (HIP events on the stream;
 * no host read falls inside, nor do the transfers of the host-array entry point). */
int tsdf_hip_mesh_smooth_stats(uint64_t out[4]);

/* meshNormals -- area-weighted per-vertex normals of a triangle mesh, from the mesh itself (after decimate or smooth have
 * moved the vertices, the TSDF gradient no longer describes it); an extension with no counterpart in the reference.  The
 * result is defined by the sequential host pass cpu_tsdf::mesh_post::normalArrays (csrc/prog/mesh_post.h) and equals it word
 * for word:
 *   1. the face vector of f = (a, b, c): e1 = (double)p_b - (double)p_a, e2 = (double)p_c - (double)p_a componentwise,
 *      g_f = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), every difference, product and subtraction rounded
 *      once, no FMA.  |g_f| is twice the face's area: the weighting is by area.  A face with a repeated index, or whose
 *      corners are distinct vertices at one position, gives the exact zero vector.  A face with a coordinate that is not
 *      finite at any corner is SKIPPED: it adds nothing and is counted.  No finite input overflows (|g| < 1e78).
 *   2. per component s_i = +0.0; then, over the faces that name i in ascending face index, s_i += g_f once per corner that
 *      names i (a face (i, i, b) adds its zero vector twice, a face given twice adds twice).  The order of the adds is part
 *      of the definition.
 *   3. l2 = (sx sx + sy sy) + sz sz, each operation rounded once, l = sqrt(l2), the IEEE square root.  l2 == 0: the normal
 *      is three +0.0f.  Otherwise n_i = ((float)(sx / l), (float)(sy / l), (float)(sz / l)): divisions, not a product with a
 *      reciprocal.
 *   4. flags[i] is the OR of 1: no face names i; 2: rule 3 wrote zero (every vertex with bit 1 has it); 4: a face that names
 *      i was skipped.
 *   5. ORIENTATION: the normal points to the side from which the corners a -> b -> c appear counter-clockwise, along
 *      (p_b - p_a) x (p_c - p_a).  On a mesh of tsdf_hip_march that is the direction of increasing d: out of the surface,
 *      into observed free space.
 *   verts, faces   HOST arrays (pinned memory is used directly, pageable memory is staged): n_verts x 3 floats, n_faces x 3
 *                  vertex indices.  faces == NULL: a triangle SOUP -- n_verts is a multiple of 3, face f has the corners
 *                  3f, 3f + 1, 3f + 2, and n_faces is n_verts / 3 (or 0: no face at all).
 *   out_normals    n_verts x 3 floats.       flags   n_verts bytes, rule 4's bits; nullable.
 * E_INVALID, checked before any device call: NULL verts or out_normals with n_verts > 0, device < 0, more than 2^31 vertices
 * or more than 1431655765 faces (the 3 n_faces entries of the inverted index are indexed with 32 bits), a soup whose n_verts
 * is not a multiple of 3 or whose n_faces is neither 0 nor n_verts / 3.  E_INVALID with nothing written: a face naming a
 * vertex >= n_verts.  n_verts == 0 (with no face) is OK and touches no device.  E_NOMEM, with the bytes in
 * tsdf_hip_last_error, when the mesh (25 bytes per vertex, 12 per face) or the working set (4 bytes per vertex, 80 per face
 * and the sort's temporary storage; a soup needs none) does not fit.
 * Cost: one radix sort of the 3 n_faces keys vertex << 32 | face builds the inverted index; then ONE lane walks each
 * vertex's faces so that the adds keep the host's order: a lane's time is its vertex's valence, 4-8 on a marched mesh; a
 * vertex named by thousands of faces makes one lane walk them all.  A soup needs no sort: one kernel, one lane per face. */
int tsdf_hip_mesh_normals(int device, const float *verts, uint64_t n_verts, const uint32_t *faces /* NULL = soup */,
                          uint64_t n_faces, float *out_normals, uint8_t *flags /* nullable */);
/* The same for the handle's mesh: the INDEXED mesh of the last tsdf_hip_march_flatten / _march_decimate (moved by
 * _march_smooth or not) while one is valid, otherwise the soup of the last tsdf_hip_march / _march_cleanup.  *n_verts
 * (nullable) says which: the indexed mesh's vertex count, or 3 x the soup's triangle count; *n_zero (nullable): the vertices
 * whose normal is zero.  The normals live in a buffer of their own on the handle; the mesh itself (positions, colours, faces,
 * cells, the soup) is not touched.  Every later tsdf_hip_march, _march_cleanup, _march_flatten, _march_decimate or
 * _march_smooth drops them (whether or not it succeeds), and so do tsdf_hip_reset and tsdf_hip_destroy.  E_INVALID when no
 * march has run.  On a multi-GPU handle the host-held merged mesh goes through tsdf_hip_mesh_normals on the first slab's
 * device; the result equals one handle holding the whole grid. */
int tsdf_hip_march_normals(tsdf_handle h, uint64_t *n_verts /* nullable */, uint64_t *n_zero /* nullable */);
/* The normals tsdf_hip_march_normals left on the handle: as many rows of 3 floats as its *n_verts said, in the order of the
 * vertices tsdf_hip_march_fetch_indexed or tsdf_hip_march_fetch returns.  E_INVALID while there are none. */
int tsdf_hip_march_fetch_normals(tsdf_handle h, float *normals);
/* Report-only, of the last normals pass (either entry point) on the calling thread: out[0] = vertices, out[1] = skipped
 * faces, out[2] = zero normals, out[3] = device microseconds from the first kernel to the last (HIP events on the stream; no
 * host read falls inside, nor do the transfers of the host-array entry point). */
int tsdf_hip_mesh_normals_stats(uint64_t out[4]);

/* getOccupiedVoxelIndices -- src/lib/tsdf_volume_octree.cpp:590-609 (+ OctreeNode::getLeaves, src/lib/octree.cpp:99-109):
 * the voxels with w > 0 && fabsf(d) < 1, d and w being the floats tsdf_hip_download returns (PACKED layout:
 * w = min(k, max_weight); a NaN distance is not listed), in the reference's leaf order: ascending key
 * spread3(x) << 2 | spread3(y) << 1 | spread3(z) (spread3 puts bit i at bit 3i) -- octree pre-order with the children as
 * split() makes them (octree.cpp:257-264) on a cubic power-of-two grid, and the same key on any other grid, as
 * tsdf_hip_march orders its cells.
 *   box    x0, y0, z0, nx, ny, nz (global voxel indices), inside the planes the handle OWNS (a Z-slab handle never lists
 *          its halo; E_INVALID otherwise); NULL = all owned planes.
 *   *n     the number of listed voxels (uint64: not capped at 2^32).
 * tsdf_hip_occupied scans (one streaming pass over the distance plane; while only integrateCloud has written the planes
 * since the reset and max_dist_pos >= max_dist_neg, cells of 64 x 4 x 1 voxels that no frame observed inside the truncation
 * band are not read) and sorts; E_NOMEM, with the bytes needed in tsdf_hip_last_error, if the two key
 * buffers (8 bytes per listed voxel each) do not fit -- a smaller box then works.  The unsorted keys borrow
 * tsdf_hip_march's cell buffer and the sort's temporary storage the handle's scratch; the sorted list has a buffer of its
 * own, so the result stays valid until the next tsdf_hip_occupied on the handle (a march or a download in between does not
 * disturb it).  The voxels' VALUES are gathered when they are fetched:
 * tsdf_hip_occupied_fetch copies, for the listed voxels in order, idx (n x 3 int32: x, y, z), d, w (n floats each) and rgb
 * (n x 3 bytes r,g,b) to the host; any pointer may be NULL.  d / w / rgb are bit for bit what tsdf_hip_download gives for
 * those voxels at the time of the fetch.  rgb is zeros for a volume without colour and E_UNSUPPORTED for
 * TSDF_COLOR_RGB_NORMALIZED / TSDF_COLOR_LAB, whose exact bytes need the host's pow: use tsdf_hip_lookup_rgb there.
 * E_INVALID before the first tsdf_hip_occupied.
 * tsdf_hip_occupied_fetch_device writes DEVICE buffers of the caller (rgb as uint32 r | g<<8 | b<<16), asynchronous on the
 * handle's stream.
 * On a multi-GPU handle every slab scans the planes it owns concurrently and the slab lists are merged by key on the host
 * (z is the low bit of each triple: the slabs interleave); the result equals one handle holding the whole grid;
 * _fetch_device is E_UNSUPPORTED there, like tsdf_hip_march_fetch_device. */
int tsdf_hip_occupied(tsdf_handle h, const int32_t box[6], uint64_t *n);
int tsdf_hip_occupied_fetch(tsdf_handle h, int32_t *idx, float *d, float *w, uint8_t *rgb);
int tsdf_hip_occupied_fetch_device(tsdf_handle h, int32_t *d_idx, float *d_d, float *d_w, uint32_t *d_rgb);
/* Report-only, of the last tsdf_hip_occupied: out[0] = listed voxels, out[1] = bytes of the distance plane the scan
 * requested, out[2] = 1 if the band flags decided what to read (0: every quad of the box was read -- after an upload / load /
 * plane copy / tsdf_hip_device_planes, with the plain RGB_NORMALIZED / LAB / weighting kernels, or with
 * max_dist_pos < max_dist_neg, where free space itself lies inside the band), out[3] = its device microseconds (scan +
 * sort, HIP events).  Multi-GPU: sums over the slabs, flags only if on every slab, the slowest slab's time. */
int tsdf_hip_occupied_stats(tsdf_handle h, uint64_t out[4]);
/* Report-only: device milliseconds by phase, as tsdf_hip_march_timing -- ms[0] the scan, ms[1] count read-back + sort,
 * ms[2] the gather kernel of the fetches since that call. */
int tsdf_hip_occupied_timing(tsdf_handle h, float ms[3]);

/* shiftVolume -- NOT IN THE REFERENCE (its octree has a fixed root, like this grid).  Moves the volume's window by whole
 * voxels, in place on the device, so that a dense grid can follow the camera.
 *   shift  (sx, sy, sz): the window moves by that many voxels along +x, +y, +z of the volume frame.  Afterwards voxel
 *          (x, y, z) holds what voxel (x + sx, y + sy, z + sz) held before, if that index lies in the grid, and the reset
 *          state, exactly as tsdf_hip_reset writes it, otherwise.  Everything a voxel owns moves with it: d, the weight (w, or
 *          the count in byte 3 of the colour word / the count plane of the PACKED layout), rgb, the float colour state of
 *          RGB_NORMALIZED / LAB, and M / nsample where allocated.  Pitch padding is not part of the contract.
 * A zero shift returns OK without touching the device.  |s| >= res on any axis is legal and leaves every voxel in the reset
 * state.  E_INVALID for a NULL handle or shift.  Like every entry point that reads or writes the planes, the call first
 * launches a frame held back by frame pairing.  Asynchronous on the handle's stream, like tsdf_hip_integrate_device without
 * n_observed.  No second copy of the volume is made: the planes are moved in batches whose sources a launch never writes
 * (DESIGN.md 3.15); the only scratch is one copy of the band flags (1/256 byte per voxel).
 * The "band seen" flags move with the data (a cell's new flag is the OR of the flags of the cells its voxels came from), so
 * what tsdf_hip_march, tsdf_hip_occupied and the PACKED integrate launches skip because of them they still skip afterwards.
 * A list made by tsdf_hip_occupied before the shift names old indices: tsdf_hip_occupied_fetch* return E_INVALID until the
 * next tsdf_hip_occupied.  The mesh of the last tsdf_hip_march is plain data and stays: it describes the volume BEFORE the
 * shift.
 * The caller's bookkeeping: the volume frame has moved by t = (sx * size[0] / res[0], sy * size[1] / res[1],
 * sz * size[2] / res[2]) in its own coordinates.  A camera pose `trans` (camera -> volume) that was right before the shift
 * is Translation(-t) * trans afterwards, and a global transform G (volume -> world) becomes G * Translation(t);
 * cpu_tsdf::TSDFVolumeOctree::shiftVolume does the latter.
 * A handle that owns part of the grid (z_begin / z_end, with its halo) shifts every allocated plane, halo included, when
 * sz == 0, and returns E_UNSUPPORTED when sz != 0: planes would have to cross processes (cpu_tsdf_amd/zslab.py has no shift).
 * On a multi-GPU set the result equals one handle holding the whole grid: the z part moves planes between the slabs (each
 * slab pulls from slabs that have not shifted yet, ascending for sz > 0), the x / y part runs on every slab by itself, and
 * the halos are stale afterwards (refreshed by the next call that needs them).
 * tsdf_hip_shift_stats: report-only, of the last tsdf_hip_shift on the handle: out[0] = voxels that kept a value, out[1] =
 * voxels reset (of the allocated planes: out[0] + out[1] = nx * ny * planes), out[2] = 1 if the band flags were carried over
 * (they described the planes before and do after), out[3] = device microseconds (HIP events on the handle's stream; the call
 * waits for the second event, i.e. for the shift to finish).  Multi-GPU: counts of the whole grid, flags only if every slab
 * carried them, the slowest slab's time. */
int tsdf_hip_shift(tsdf_handle h, const int32_t shift[3]);
int tsdf_hip_shift_stats(tsdf_handle h, uint64_t out[4]);

/* mergeVolume -- NOT IN THE REFERENCE (its volumes can only be fused frame by frame).  Resamples volume `src` at the voxel
 * centres of volume `dst` under a rigid transform and adds the samples to dst as weighted observations, on the device: what
 * joining submaps, changing a volume's resolution, and re-centring one by a fraction of a voxel or a rotation all come to.
 *   src_from_dst  the first three rows, row-major, of the transform that takes dst volume coordinates to src volume
 *                 coordinates (the caller's Eigen computes it, as for cam_from_vol); cast to float as the reference casts poses.
 *   min_weight    the gate's threshold, >= 0.
 *   n_merged      nullable; the number of dst voxels that received an observation.  The call is asynchronous on dst's stream
 *                 unless it is given.
 * RULE, per voxel (x, y, z) of dst:
 *   c   = (ctr_x[x], ctr_y[y], ctr_z[z]): dst's own centre tables (tsdf_hip_centers; what integrateCloud projects).
 *   q_r = ((M[r][0] * c.x + M[r][1] * c.y) + M[r][2] * c.z) + M[r][3] in fp32, M = (float)src_from_dst: tsdf_hip_align_system's order.
 *   ok, val = getFxn(q) on src, bit for bit what tsdf_hip_sample(src, q) returns.
 *   GATE: the voxel is merged iff ok, all eight neighbour voxels of q in src have weight > min_weight (strictly; any layout),
 *   val is not NaN, and src has a voxel that CONTAINS q -- the one tsdf_hip_lookup_rgb finds (Octree::getContainingVoxel),
 *   always one of the eight.  w_s and the colour c_s are that voxel's (not a blend of the eight: only so does merging two
 *   volumes fused from disjoint frames on one grid give the weights, and to rounding the distances, of fusing all frames).
 *   UPDATE = RGBNode::addObservation(val, w_s, max_weight of dst, c_s) (src/lib/octree.cpp:153-163, 329-337): colour first,
 *   per channel (uint8)((w * c + w_s * c_s) / (w + w_s)) with the old w, and only if BOTH volumes store colour (else dst's
 *   colour stays); then d = (d * w + val * w_s) / (w + w_s) in fp32 in that order with IEEE division; then w += w_s, clamped
 *   to dst's max_weight.  w_s > min_weight >= 0 keeps 0 / 0 out.  M_ / nsample_ are not touched.  A voxel that is not merged is
 *   neither read nor written.
 *   Consequences of getFxn's neighbour rule (getNeighbors wants the voxel of q and the next one up along every axis): a dst
 *   voxel whose q lies in the last half voxel of src along an axis, or whose upper neighbours are unobserved, is not merged --
 *   under the identity on equal grids that is the top plane, row and column, and every voxel next to an unobserved one on its
 *   upper side.  Where q hits a src voxel centre exactly, the seven upper neighbours enter val with interpolation weight 0
 *   (val is that voxel's d, up to the rounding of c^3 * d / c^3: exact for a dyadic voxel size) but still have to pass the gate.
 * CONVENTIONS: dst may be any grid (non-cubic, any resolution); only a box of dst voxels that encloses src's bounding box
 * (transformed in fp64, padded by two voxels) is visited, and a src that does not reach dst returns OK with 0 merged, touching
 * nothing.  Both handles first launch a frame held back by frame pairing.  The kernel runs on dst's stream after everything
 * queued on src's stream so far, and work queued on src's stream afterwards waits for it.  src is unchanged in every respect
 * (tsdf_hip_destroy(src) waits on src's stream, and with it for a merge that is still reading it).
 * Afterwards dst's "band seen" flags no longer describe its planes, exactly as after tsdf_hip_upload: tsdf_hip_march,
 * tsdf_hip_occupied and the PACKED integrate launches read everything until the next tsdf_hip_reset.  A list made by
 * tsdf_hip_occupied stays valid, as after an upload (its values are gathered at the fetch).
 * TSDF_HIP_E_INVALID: a NULL handle or matrix, dst == src, a matrix entry that is not finite, min_weight negative or NaN.
 * TSDF_HIP_E_UNSUPPORTED, with the reason in tsdf_hip_last_error:
 *   - either handle is a multi-GPU set or owns only part of its grid (z_begin / z_end);
 *   - the handles are on different devices;
 *   - src's res[0..2] or size[0..2] are not all equal (getFxn's weights assume cubic voxels);
 *   - max_dist_pos or max_dist_neg differ (d is stored divided by max_dist_neg);
 *   - either volume uses TSDF_COLOR_RGB_NORMALIZED or TSDF_COLOR_LAB, or weights by depth or by variance;
 *   - dst is PACKED and src is not PACKED with the same max_weight (only then does every merged weight have a count).
 * Nothing on the device is touched before all of these checks have passed.
 * tsdf_hip_merge_stats: report-only, of the last tsdf_hip_merge with the handle as dst: out[0] = voxels in the launch box,
 * out[1] = voxels merged, out[2] = 1 if dst's band flags were live and had to be dropped, out[3] = device microseconds of the
 * kernel (HIP events on dst's stream; the call waits for the second event, i.e. for the merge to finish). */
int tsdf_hip_merge(tsdf_handle dst, tsdf_handle src, const double src_from_dst[12], float min_weight, uint64_t *n_merged);
int tsdf_hip_merge_stats(tsdf_handle dst, uint64_t out[4]);

/* computeDistanceField -- NOT IN THE REFERENCE (its volumes only know the truncated distance d, which says nothing outside
 * the band of +- one truncation distance).  The exact Euclidean distance transform of the volume's zero crossing, computed
 * on the device, kept on the handle and readable as a whole field, into device buffers and by batched point queries.
 *   box         x0, y0, z0, nx, ny, nz (voxel indices) inside the grid; NULL = the whole grid.
 *   r_max       >= 0, in voxels.  0 = unlimited; otherwise every d2 above r_max^2 becomes TSDF_HIP_ESDF_FAR.
 *   min_weight  >= 0: a voxel counts as observed iff its weight is above it (strictly).
 *   n_sites     nullable; the number of sites in the box.
 * RULE.  d_v and w_v are the floats tsdf_hip_download returns for voxel v (PACKED layout: w = min(k, max_weight)).
 *   valid(v) := w_v > min_weight and d_v is not NaN.      neg(v) := valid(v) and d_v < 0  (-0.0 is not negative).
 *   SITE: a voxel v inside the box is a site iff valid(v) and some 6-neighbour u inside the GRID has valid(u) and
 *   neg(u) != neg(v).  u may lie outside the box; it may not lie outside the grid (a voxel on the grid border has no
 *   neighbour beyond it).  Both voxels of a crossing edge are therefore sites.  The "band seen" flags are not consulted.
 *   d2, for EVERY voxel v of the box: the minimum over the sites s in the box of |v - s|^2 in voxel units, an exact uint32.
 *   With r_max > 0 any value above r_max^2 becomes TSDF_HIP_ESDF_FAR; with r_max == 0 a voxel is FAR only if the box holds
 *   no site.
 *   dist(v) = sgn * voxel * sqrtf((float)d2): sgn = -1 iff neg(v), else +1 (unobserved voxels are positive: a caller that
 *   must tell "unknown" apart reads w); FAR gives sgn * INFINITY; voxel is the fp32 voxel edge size[0] / res[0] that getFxn
 *   scales by on this handle (tsdf_voxel_edge in the library's tsdf_common.h, sample_point's `c`); sqrtf is the correctly
 *   rounded one and the product one fp32 multiplication, so the field is bit for bit
 *   np.sqrt(d2.astype(np.float32)) * np.float32(voxel), negated where neg(v).
 * LIFETIME, as tsdf_hip_occupied's list: the field describes the volume AT THE TIME OF THE CALL -- the sign as well, which
 * is recorded then -- and stays valid, and STALE BY DESIGN, across later integrates, marches, uploads and downloads, and
 * across a tsdf_hip_merge with the handle as dst or as src.  It is dropped by tsdf_hip_reset, tsdf_hip_destroy and the next
 * tsdf_hip_esdf on the handle that is not refused.  After tsdf_hip_shift the fetches and the sample return E_INVALID until
 * the field has been computed again: the indices moved.  The same after tsdf_hip_deintegrate / _deintegrate_device (a frame
 * is taken back to correct it: a field that still shows it is ended, not left stale), and before the first tsdf_hip_esdf.
 * Like every entry point that reads the planes, the call first launches a frame held back by frame pairing.  The volume's
 * planes and "band seen" flags are neither written nor invalidated, and the results tsdf_hip_march and tsdf_hip_occupied
 * keep on the handle survive the call.  The call waits for its kernels.
 *   tsdf_hip_esdf_fetch         d2 and dist of the box to the host, [z][y][x] of the box; either may be NULL.
 *   tsdf_hip_esdf_fetch_device  the same into DEVICE buffers of the caller, asynchronous on the handle's stream.
 *   tsdf_hip_esdf_sample        per point (n x 3 floats, volume coordinates) the value of the voxel that CONTAINS it -- the
 *                               voxel tsdf_hip_lookup_rgb finds (Octree::getContainingVoxel); no interpolation.  found = 1
 *                               iff that voxel exists and lies in the box; otherwise found = 0 and dist = NaN.
 *   tsdf_hip_esdf_stats         report-only, of the last tsdf_hip_esdf: out[0] = voxels of the box, out[1] = sites, out[2] =
 *                               bytes of device memory the field and its scratch hold (d2: 4 per voxel; the sign plane: one
 *                               bit per voxel; the envelopes of the y / z passes: up to 8 per voxel, at most 1 GiB), out[3]
 *                               = device microseconds of the three passes (HIP events).
 * TSDF_HIP_E_INVALID: a NULL handle; a box outside the grid or with a non-positive extent; r_max < 0; min_weight negative
 * or NaN.  TSDF_HIP_E_UNSUPPORTED, with the reason in tsdf_hip_last_error: a multi-GPU set; a handle that owns only part
 * of its grid (distances cross slab borders); res[0..2] or size[0..2] not all equal; a box of more than 16384 voxels along
 * an axis.  TSDF_HIP_E_NOMEM, with the bytes needed in tsdf_hip_last_error, if the field and its scratch do not fit -- a
 * smaller box then works.  Every refusal but the last comes before the device is touched. */
#define TSDF_HIP_ESDF_FAR 0xFFFFFFFFu
int tsdf_hip_esdf(tsdf_handle h, const int32_t box[6], int32_t r_max, float min_weight, uint64_t *n_sites);
int tsdf_hip_esdf_fetch(tsdf_handle h, uint32_t *d2, float *dist);
int tsdf_hip_esdf_fetch_device(tsdf_handle h, uint32_t *d_d2, float *d_dist);
int tsdf_hip_esdf_sample(tsdf_handle h, const float *xyz, size_t n, float *dist, uint8_t *found);
int tsdf_hip_esdf_stats(tsdf_handle h, uint64_t out[4]);

/* deintegrateCloud -- NOT IN THE REFERENCE (its running averages only grow).  Takes a frame back out of the volume: the
 * first half of correcting a frame's pose after a loop closure (remove it under the old pose, integrate it under the new
 * one; BundleFusion, Dai et al. 2017, section 6) without a reset and a second pass over the whole sequence.
 *   depth, bgra, cam_from_vol   as for tsdf_hip_integrate (host frame, through the handle's staging; the call waits) and
 *                               tsdf_hip_integrate_device (device frame); bgra is needed iff integrate_color.
 *   n_removed                   nullable; the number of voxels whose weight went down (out[1] below).  Without it the
 *                               device call is asynchronous on the handle's stream and nothing is counted.
 * RULE.  The frame, the pose and the reference-cull planes in force on the handle (tsdf_hip_set_reference_cull) SELECT
 * exactly the voxels tsdf_hip_integrate would bring to addObservation, with the same d_new -- the same transform order,
 * fp64 projection, sensor range, image bounds, NaN test, d_new < -max_dist_neg rejection, max_dist_pos clamp and division
 * by max_dist_neg: one copy of the device code serves both -- and, with colour, the same pixel colour c_obs.
 * Per selected voxel with stored d, w (PACKED: w = min(k, max_weight)) and colour bytes c, every operation in fp32 and
 * rounded on its own (no contraction), IEEE division:
 *   w == 0            nothing is written.
 *   W = ceilf(w), w' = W - 1.  Weights below saturation are integers (W == w); at saturation W = ceil(max_weight) = kmax,
 *                     so the PACKED count (k' = k - 1) and the F32W weight (w' = W - 1) agree for every max_weight.
 *   w' <= 0           the voxel returns to the state tsdf_hip_reset leaves: d = -1, w = 0 / k = 0, colour bytes 0.
 *   otherwise         d' = d where d and d_new have the same bits (a mean of equal values does not move: free space stays
 *                     exactly at the hinge value), else d' = (d * W - d_new) / w';
 *                     per colour channel x = (W * c - c_obs) / w', c' = (uint8)(min(max(x, 0), 255) + 0.5f) -- nearest,
 *                     because the forward update truncated and a second truncation would bias dark;
 *                     w / k <- w'.
 * Below saturation the weights are exactly those of the other frames alone, and d and the colour are their mean up to
 * rounding (DESIGN.md 3.21 has the figures of the host model).  SATURATION: a voxel at max_weight has forgotten how many frames it saw; it loses one count like any
 * other, which weights the removed frame at 1 / kmax of the stored mean.  That is an approximation, and the only one.
 * Nothing checks that the frame was ever integrated: removing a stranger subtracts it all the same.
 * The "band seen" flags and the implied-distance record SURVIVE (unlike tsdf_hip_merge): the kernel sets a cell's flag where
 * it lowers a weight with an observation inside the band (d_new off the hinge value), the rule the integrate kernels set it
 * by, so tsdf_hip_march, tsdf_hip_occupied and the PACKED integrate launches go on skipping what they skipped.  Where the
 * handle's record does not cover this call's hinge value (F32W layout, non-integer max_weight, truncation limits changed
 * since the reset) every lowered weight sets its cell's flag; where the flags are already inexact none are kept.
 * Like every writer of the planes the call first launches a frame held back by frame pairing.  Unlike the other writers
 * (integrate, upload, merge, which leave a distance field of tsdf_hip_esdf valid and stale) it ENDS that field: the fetches
 * and the sample return E_INVALID until the next tsdf_hip_esdf.  A list of tsdf_hip_occupied and the meshes of
 * tsdf_hip_march stay, as after an integrate.  It covers exactly the planes the handle's integrate launches write (Z-slab
 * handles work; their halo planes are the caller's to refresh, as after an integrate).  A pose with a non-finite entry
 * selects nothing: OK, 0.
 * TSDF_HIP_E_INVALID: a NULL handle, frame or pose; integrate_color without bgra.
 * TSDF_HIP_E_UNSUPPORTED, with the reason in tsdf_hip_last_error and the planes untouched: weight_by_depth or
 * weight_by_variance on, or the variance state allocated; TSDF_COLOR_RGB_NORMALIZED / TSDF_COLOR_LAB; a multi-GPU set
 * (tsdf_hip_create_multi: a follow-up).
 * tsdf_hip_deintegrate_stats: report-only.  out[0] = voxels the frame selected, out[1] = voxels whose weight went down,
 * out[2] = of those, voxels that returned to unobserved -- all three of the last call that passed n_removed; out[3] =
 * device microseconds of the last call's kernel (HIP events on the stream; waits for the second one; 0 if none ran). */
int tsdf_hip_deintegrate(tsdf_handle h, const float *depth, const uint8_t *bgra, const float cam_from_vol[12], uint64_t *n_removed);
int tsdf_hip_deintegrate_device(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float cam_from_vol[12],
                                uint64_t *n_removed);
int tsdf_hip_deintegrate_stats(tsdf_handle h, uint64_t out[4]);

/* reintegrateCloud -- NOT IN THE REFERENCE.  Re-poses a fused frame in ONE sweep of the volume: both halves of correcting a
 * frame's pose after a loop closure, for a caller who gets a corrected pose from a pose graph.
 *   depth, bgra                 the frame, as for tsdf_hip_deintegrate (host frame: uploaded once through the handle's staging,
 *                               the call waits; device frame: tsdf_hip_reintegrate_device); bgra is needed iff integrate_color.
 *   cam_from_vol_old, planes_old   the pose the frame was integrated under and the reference-cull planes it had then
 *   cam_from_vol_new, planes_new   the corrected pose and its planes; either planes pointer may be NULL: no cull for that pose
 *   n                           nullable, 2 values: n[0] = voxels whose weight the removal lowered, n[1] = voxels the new
 *                               pose brought to addObservation.  Without it the device call is asynchronous on the
 *                               handle's stream and nothing is counted.
 * DEFINITION.  The call leaves d, w / k and rgb of every voxel, bit for bit, as tsdf_hip_deintegrate(h, frame, old) with
 * planes_old in force followed by tsdf_hip_integrate(h, frame, new) with planes_new in force leaves them.  Removal: the RULE
 * above tsdf_hip_deintegrate (W = ceilf(w), the equal-bits clause, colour rounded to nearest, the reset state at w' <= 0).
 * Addition: OctreeNode / RGBNode::addObservation with w_new = 1, as tsdf_hip_integrate applies it.  Each half selects its
 * voxels as its own call does, with its own pose and its own six planes; voxels are independent of each other, so one
 * kernel applies the removal and then the addition to a voxel in registers and writes each word once.
 * COST (one MI355X): 0.97 x the time of the two calls where a pose's cull planes bite and tsdf_hip_integrate runs its
 * plain kernel; 1.1-1.26 x where neither pose's planes bite and tsdf_hip_integrate runs its fast kernel -- there the two calls
 * are the quicker way and keep the flags as well.
 * SATURATION: the caveat of tsdf_hip_deintegrate is inherited -- a voxel at max_weight has forgotten how many frames it saw
 * and loses one count like any other before the new observation is added.  Nothing checks that the frame was ever
 * integrated under the old pose.
 * STATE.  The "band seen" flags and the implied-distance record SURVIVE in every regime (the two calls lose the flags where
 * the cull bites and the integrate goes through the plain kernel): the removal half sets a cell's flag as
 * tsdf_hip_deintegrate does, deciding from the record as it stands before the call; the addition half sets it where the new
 * pose observes a d_new off the hinge value; a voxel observed at exactly the hinge value in a flag-0 cell ends there.  The
 * record is updated for the addition as by an integrate launch that keeps the flags.  After the call the planes in force on
 * the handle are planes_new (NULL: none), as tsdf_hip_integrate_device2 keeps frame B's.  Like every writer of the planes the
 * call first launches a frame held back by frame pairing and invalidates the distance field of tsdf_hip_esdf; it covers the
 * planes the handle's integrate launches write (Z-slab handles work).
 * A pose with a non-finite entry selects nothing: old not finite, the call is a tsdf_hip_integrate; new not finite, a
 * tsdf_hip_deintegrate; both, nothing is written: OK, counts 0.
 * TSDF_HIP_E_INVALID, before any device is touched: a NULL handle, frame, old or new pose; integrate_color without bgra.
 * TSDF_HIP_E_UNSUPPORTED, with the reason in tsdf_hip_last_error, the voxel planes and the cull planes untouched: the handles
 * tsdf_hip_deintegrate refuses -- weight_by_depth or weight_by_variance on, or the variance state allocated;
 * TSDF_COLOR_RGB_NORMALIZED / TSDF_COLOR_LAB; a multi-GPU set (tsdf_hip_create_multi: still open).
 * tsdf_hip_reintegrate_stats: report-only.  out[0] = voxels the old pose selected, out[1] = voxels whose weight went down,
 * out[2] = of those, voxels the removal took back to unobserved, out[3] = voxels the new pose observed, out[4] = voxels both
 * poses selected -- all five of the last call that passed n; out[5] = device microseconds of the last call's kernel (HIP
 * events on the stream; waits for the second one; 0 if none ran). */
int tsdf_hip_reintegrate(tsdf_handle h, const float *depth, const uint8_t *bgra, const float cam_from_vol_old[12], const float *planes_old,
                         const float cam_from_vol_new[12], const float *planes_new, uint64_t *n);
int tsdf_hip_reintegrate_device(tsdf_handle h, const float *d_depth, const uint32_t *d_bgra, const float cam_from_vol_old[12],
                                const float *planes_old, const float cam_from_vol_new[12], const float *planes_new, uint64_t *n);
int tsdf_hip_reintegrate_stats(tsdf_handle h, uint64_t out[6]);

#define TSDF_HIP_RAYS_AS_GIVEN 1
/* castRays -- NOT IN THE REFERENCE (its only ray query is renderView, the rays of one pinhole image).  Casts n arbitrary rays
 * into the fused volume on the GPU: line of sight between points, a simulated lidar or second camera, picking, view scoring.
 *   org, dir       n x 3 floats each, volume frame: ray i is o_i + t * u_i.  u_i is used AS GIVEN: not normalised, not checked
 *                  for length.  The step rule below is the reference's only for unit directions.
 *   t_range        n x 2 floats tmin_i, tmax_i (in units of |u_i|), or NULL: min_sensor_dist / max_sensor_dist for every ray
 *   flags          bit 0, TSDF_HIP_RAYS_AS_GIVEN: "my rays are already coherent, march them in my order".  Without it the
 *                  library may march them in any order; the results are per ray and never depend on it.  Today the bit
 *                  changes nothing: the library always marches in the given order, because sorting the rays first did not
 *                  pay even for randomly permuted rays (DESIGN.md 3.23's measurement).  Any other bit: E_INVALID.
 *   out            n x 8 floats: x, y, z, nx, ny, nz, t*, iterations of ray i, volume frame
 *   rgb            nullable, n x 3 bytes;  status: nullable, n bytes
 * DEFINITION.  out[8 i ..] is exactly what k_raycast<false> -- tsdf_hip_raycast, renderView, tsdf_volume_octree.cpp:290-421 --
 * writes for a pixel whose rotated direction du equals u_i, with the origin o_i and the sensor range [tmin_i, tmax_i]; every
 * other constant of the loop (the first step, the refinement step, the leaf size, max_dist_neg) comes from the handle as for
 * tsdf_hip_raycast.  Both kernels run one copy of the loop.  A miss has NaN x, y, z and a zero normal, t and iterations as
 * the loop left them; a hit whose neighbourhood is not valid has NaN normals.
 * Colour: the bytes tsdf_hip_lookup_rgb returns at the hit point (the voxel that contains it), read in the same kernel; 0, 0, 0
 * for a miss, where that lookup finds no voxel, and on a volume without colour.
 * status: 0 miss, 1 hit (x, y, z finite), 2 not admitted, 3 stopped by the trip cap.
 * ADMISSION AND TERMINATION.  renderView's loop ends only through float progress of t; here termination does not depend on
 * float arithmetic.  A ray is refused (status 2: NaN x, y, z, a zero normal, t = tmin_i, iterations 0, no voxel touched) when
 * one of its 8 inputs is not finite, or when cap = 16 + 2 * ceil((tmax - tmin) / (leaf / 4)), computed in double, exceeds
 * 2^24.  tmax <= tmin is admitted: the loop does not run, as in the reference.  An integer trip counter covers main-loop and
 * refinement-walk iterations together and stands in the condition of both loops; a ray that reaches cap ends as a miss with
 * status 3, t and iterations as at that moment.  `iterations` stays the reference's count (main loop only).  A ray that makes
 * the reference's forward progress (at least leaf / 4 per main-loop iteration) never reaches its cap.
 * Host form: staged through the handle's scratch and pinned stage, waits.  tsdf_hip_cast_rays_device: the same with device
 * pointers on the handle's device, asynchronous on the handle's stream.
 * Like every reader the call first launches a frame held back by frame pairing.
 * TSDF_HIP_E_INVALID, before any device is touched: a NULL handle, org, dir or out; n == 0; n >= 2^31; unknown flag bits.
 * TSDF_HIP_E_UNSUPPORTED, with the reason in tsdf_hip_last_error: a multi-GPU set (tsdf_hip_create_multi) -- cast into one
 * whole-grid handle; a Z-slab handle that does not hold the whole grid; rgb != NULL on a TSDF_COLOR_LAB volume, whose exact
 * bytes need the host's pow (pass NULL and use tsdf_hip_lookup_rgb).  A refusal writes nothing.
 * tsdf_hip_cast_rays_stats: report-only, of the last call on the handle; synchronises.  out[0] = rays, out[1] = hits (status
 * 1), out[2] = rays ended with status 2 or 3, out[3] = device microseconds of the call's kernels (HIP events on the stream). */
int tsdf_hip_cast_rays(tsdf_handle h, const float *org, const float *dir, const float *t_range, size_t n, int flags, float *out,
                       uint8_t *rgb, uint8_t *status);
int tsdf_hip_cast_rays_device(tsdf_handle h, const float *d_org, const float *d_dir, const float *d_t_range, size_t n, int flags,
                              float *d_out, uint8_t *d_rgb, uint8_t *d_status);
int tsdf_hip_cast_rays_stats(tsdf_handle h, uint64_t out[4]);

/* Block transfer of raw voxels (parity tests, save/load, halo exchange).  Coordinates are global
 * grid indices; the block must lie inside the handle's slab + halo.  Any pointer may be NULL.
 * rgb is 3 bytes per voxel (r,g,b).  *_device variants take device pointers (rgb then 4 bytes). */
int tsdf_hip_download(tsdf_handle h, int x0, int y0, int z0, int nx, int ny, int nz, float *d,
                      float *w, uint8_t *rgb);
int tsdf_hip_upload(tsdf_handle h, int x0, int y0, int z0, int nx, int ny, int nz, const float *d,
                    const float *w, const uint8_t *rgb);

/* The float colour state of the voxels of planes z0 .. z0+nz (nz * ny * nx floats): plane_index 0..3 = r_n_, g_n_,
 * b_n_, i_ of RGBNormalized (octree.h:217-222) or 0..2 = L_, A_, B_ of LABNode (octree.h:296-298).  The reference has
 * no accessor for it (the members are public); the parity tests read it.  Single-device handles only. */
int tsdf_hip_download_color_state(tsdf_handle h, int plane_index, int z0, int nz, float *out);

/* save / load -- src/lib/tsdf_volume_octree.cpp:222-275 (+ Octree::serialize / deserialize,
 * src/lib/octree.cpp:289-304,360-367,645-678): the reference's .vol checkpoint, readable and writable by both
 * sides.  The dense grid becomes an octree whose uniform subtrees are single leaves (lossless for every
 * reader that looks voxels up by position); both directions stream the grid through host memory in cubic
 * blocks (tuning "vol_chunk", 256), so host memory stays at one block whatever the resolution.  Needs a
 * cubic power-of-two grid and a handle that owns all of it.
 *   meta      what the file carries that a tsdf_params does not; NULL on save = max_cell_size of one voxel,
 *             not empty, no depth/variance weighting, identity transform.
 * tsdf_hip_load makes a NEW handle from the file's header; `defaults` supplies what the file does not hold
 * (device, layout, xform_order; NULL = tsdf_hip_default_params).  With layout AUTO a file whose weights
 * are not min(k, max_weight) is read again into the F32W layout; PACKED fails with E_UNSUPPORTED. */
typedef struct tsdf_vol_meta {
  float max_cell_size[3];      /* setMaxVoxelSize, tsdf_volume_octree.h:166 (unused by a dense grid) */
  int32_t is_empty;            /* tsdf_volume_octree.h:286,356 */
  int32_t weight_by_depth;     /* :358 */
  int32_t weight_by_variance;
  double global_transform[16]; /* setGlobalTransform :132, row-major */
} tsdf_vol_meta;
int tsdf_hip_save(tsdf_handle h, const char *filename, const tsdf_vol_meta *meta);
int tsdf_hip_load(const char *filename, const tsdf_params *defaults, tsdf_handle *out, tsdf_params *params_out,
                  tsdf_vol_meta *meta_out);
/* The same into a multi-GPU set (tsdf_hip_create_multi). */
int tsdf_hip_load_multi(const char *filename, const tsdf_params *defaults, const int32_t *devices, int n_devices,
                        tsdf_handle *out, tsdf_params *params_out, tsdf_vol_meta *meta_out);

/* The same writer and reader for a volume that is not one handle (Z-slabs on several GPUs): the voxels
 * move through callbacks, one cubic block of `edge`^3 voxels at a time (d, w: edge^3 floats; rgb: 3 edge^3
 * bytes, NULL without colour; x fastest).  A callback returns 0 to go on; anything else aborts the call,
 * which then returns that value.  No device is touched by these two functions themselves.
 *   tsdf_hip_save_blocks  p describes the whole grid (res, size, ... ; slab fields ignored).  `fetch` is
 *                         called once per block and once more for each block that is not uniform.
 *   tsdf_hip_load_blocks  `on_header` receives the file's parameters (fields the file does not carry are
 *                         taken from `defaults`, NULL = tsdf_hip_default_params) before the first block;
 *                         then `store` is called exactly once per block.  store == NULL reads the header only. */
typedef int (*tsdf_block_fn)(void *user, int x0, int y0, int z0, int edge, float *d, float *w, uint8_t *rgb);
typedef int (*tsdf_header_fn)(void *user, const tsdf_params *p, const tsdf_vol_meta *meta);
int tsdf_hip_save_blocks(const tsdf_params *p, const tsdf_vol_meta *meta, const char *filename,
                         tsdf_block_fn fetch, void *user);
int tsdf_hip_load_blocks(const char *filename, const tsdf_params *defaults, tsdf_header_fn on_header,
                         tsdf_block_fn store, void *user);

/* Whole planes [z0, z0+nz) to / from packed DEVICE buffers ([nz][ny][nx]; rgb as uint32 r|g<<8|b<<16),
 * asynchronous on the handle's stream.  This is the halo-exchange primitive: the buffers are what the
 * caller hands to RCCL send/recv.  Planes may lie in the halo.  Any pointer may be NULL. */
int tsdf_hip_get_planes_device(tsdf_handle h, int z0, int nz, float *d, float *w, uint32_t *rgb);
int tsdf_hip_set_planes_device(tsdf_handle h, int z0, int nz, const float *d, const float *w,
                               const uint32_t *rgb);

/* Raw device pointers of the SoA planes and their geometry: element index of voxel (x,y,z_global) =
 * ((z_global - z_first)*ny + y)*pitch + x.  In the PACKED layout *w is NULL (see tsdf_hip_layout) and the
 * count sits in byte 3 of *rgb; without colour neither is exposed -- use the get/set_planes calls. */
int tsdf_hip_device_planes(tsdf_handle h, float **d, float **w, uint32_t **rgb, int64_t *pitch,
                           int32_t *z_first, int32_t *nz_alloc);

/* TSDF_LAYOUT_F32W or TSDF_LAYOUT_PACKED: what AUTO resolved to for this handle. */
int tsdf_hip_layout(tsdf_handle h);

/* Voxel-centre tables actually used by the kernels: the reference's octree node centres
 * (src/lib/octree.cpp:244-266 split arithmetic) for each axis.  out has res[axis] floats. */
int tsdf_hip_centers(tsdf_handle h, int axis, float *out);

/* Report: the last integrate launch on this handle (slab 0 of a set) -- out[0] = the kernel: 0 k_integrate's general
 * instance, 1 its ALLIN instance (the host proved from the slab's eight corner voxels that EVERY voxel is inside the sensor
 * range and projects inside the image with a pixel to spare -- the camera-outside-the-volume case -- so the per-voxel range /
 * image-bounds tests are compiled out), 2 k_integrate2 (two frames in one sweep) -- in the low byte; bit 8 (0x100) is set
 * when the ALLIN launch ran the software-pipelined row loop (k_integrate_p: PACKED layout without colour); out[1] = 1 with the certified fp32
 * projection; out[2] = 0 no row intervals, 1 row intervals + block flags (the frame sees part of the slab), 2 the same with
 * the reference's frustum cull carried in the intervals; out[3] = blocks launched (0: nothing could be observed). */
int tsdf_hip_last_launch_info(tsdf_handle h, int32_t out[4]);

const char *tsdf_hip_error_string(int code);
const char *tsdf_hip_last_error(void);
int tsdf_hip_device_count(void);
/* ABI version of this header. */
int tsdf_hip_abi_version(void);
#define TSDF_HIP_ABI_VERSION 14

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_H */
