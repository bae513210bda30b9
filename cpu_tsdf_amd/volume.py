"""Python-side mirror of the reference's ``TSDFVolumeOctree`` / ``MarchingCubesTSDFOctree`` interface
for the accelerated path, on top of the C ABI (``include/tsdf_hip.h``).

Method names, argument meaning and defaults follow the reference
(``include/cpu_tsdf/tsdf_volume_octree.h``, ``src/lib/tsdf_volume_octree.cpp:54-199``): configure
with setters, then ``reset()``, then ``integrateCloud`` per frame.  The organised point cloud of the
reference becomes a ``(H, W)`` float32 depth image (``pt.z``; NaN = no return) plus an optional
``(H, W, 4)`` uint8 image in PCL ``PointXYZRGBA`` byte order.  All compute happens in HIP kernels; a
missing ``libtsdf_hip.so`` or GPU raises.
"""
import ctypes as C

import numpy as np

from . import capi
from .synth import cam_from_vol_f32, eigen_affine_inverse


class NonCubicQueryWarning(UserWarning):
    """renderView / getFxn / reconstruct on a non-cubic setGridSize: answered on the flat grid's geometry (see
    TSDFVolumeOctree._cubic_for_queries)."""


class AlignmentError(RuntimeError):
    """alignCloud could not go on: ``code`` is capi.ALIGN_NO_POINTS or capi.ALIGN_RANK_DEFICIENT, ``refined`` the pose of
    the last good step (the guess, if none), ``iterations`` the steps taken, ``cost_log`` as alignCloud returns it."""

    def __init__(self, code, refined, iterations, cost_log):
        self.code, self.refined, self.iterations, self.cost_log = code, refined, iterations, cost_log
        what = "no point passed the gate" if code == capi.ALIGN_NO_POINTS else "the cloud does not constrain all six freedoms"
        super().__init__(f"alignCloud: {what} (after {iterations} steps)")


def backproject(depth, fx, fy, cx, cy):
    """A depth image (H, W; NaN = no return) as the cloud alignCloud / alignmentSystem take: per pixel
    ((u - cx) / fx * z, (v - cy) / fy * z, z) in float64, rounded to float32; NaN pixels are dropped."""
    z = np.asarray(depth, dtype=np.float64)
    v, u = np.mgrid[0:z.shape[0], 0:z.shape[1]]
    keep = ~np.isnan(z)
    z, u, v = z[keep], u[keep].astype(np.float64), v[keep].astype(np.float64)
    return np.ascontiguousarray(np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1), dtype=np.float32)


class TSDFVolumeOctree:
    """Drop-in for ``cpu_tsdf::TSDFVolumeOctree`` (flat SoA grid in HBM instead of an octree)."""

    def __init__(self):
        self._p = capi.default_params()  # reference constructor defaults, tsdf_volume_octree.cpp:54-85
        self._h = None
        self._global_transform = np.eye(4)
        self._is_empty = True
        self._stream = None

    # -- configuration (tsdf_volume_octree.cpp:92-199, tsdf_volume_octree.h:101-190) ----------------
    def setResolution(self, xres, yres, zres):
        self._p.res[:] = (int(xres), int(yres), int(zres))

    def getResolution(self):
        return tuple(self._p.res)

    def setGridSize(self, xsize, ysize, zsize):
        self._p.size[:] = (float(xsize), float(ysize), float(zsize))

    def getGridSize(self):
        return tuple(self._p.size)

    def setImageSize(self, width, height):
        self._p.image_width, self._p.image_height = int(width), int(height)

    def getImageSize(self):
        return self._p.image_width, self._p.image_height

    def setDepthTruncationLimits(self, max_dist_pos, max_dist_neg):
        self._p.max_dist_pos, self._p.max_dist_neg = float(max_dist_pos), float(max_dist_neg)

    def getDepthTruncationLimits(self):
        return self._p.max_dist_pos, self._p.max_dist_neg

    def setWeightTruncationLimit(self, max_weight):
        self._p.max_weight = float(max_weight)

    def getWeightTruncationLimit(self):
        return self._p.max_weight

    def setGlobalTransform(self, trans):
        self._global_transform = np.array(trans, dtype=np.float64).reshape(4, 4)

    def getGlobalTransform(self):
        return self._global_transform.copy()

    def setCameraIntrinsics(self, fx, fy, cx, cy):
        self._p.fx, self._p.fy, self._p.cx, self._p.cy = float(fx), float(fy), float(cx), float(cy)

    def getCameraIntrinsics(self):
        return self._p.fx, self._p.fy, self._p.cx, self._p.cy

    def setMaxVoxelSize(self, x, y, z):
        """Accepted for interface compatibility; a dense grid has no coarse cells."""
        self._max_cell = (float(x), float(y), float(z))

    def setNumRandomSplts(self, n):
        """Accepted for interface compatibility; there is no pre-split pass on a dense grid."""
        self._num_random_splits = int(n)

    def setIntegrateColor(self, flag):
        self._p.integrate_color = 1 if flag else 0

    def setColorMode(self, color_mode):
        """tsdf_volume_octree.h:290: "RGB" (default), "RGBNormalized" or "LAB" (OctreeNode::instantiateByTypeString,
        octree.cpp:193-206)."""
        modes = {"RGB": capi.COLOR_RGB, "RGBNormalized": capi.COLOR_RGB_NORMALIZED, "LAB": capi.COLOR_LAB}
        if color_mode not in modes:
            raise ValueError(f"colour mode {color_mode!r} does not exist in the HIP volume (have {sorted(modes)})")
        self._p.color_mode = modes[color_mode]

    def setSensorDistanceBounds(self, min_sensor_dist, max_sensor_dist):
        self._p.min_sensor_dist, self._p.max_sensor_dist = float(min_sensor_dist), float(max_sensor_dist)

    def getSensorDistanceBounds(self):
        return self._p.min_sensor_dist, self._p.max_sensor_dist

    def setTransformOrder(self, order):
        """Not in the reference: which PCL ``transformPoint`` summation order to mirror."""
        self._p.xform_order = int(order)

    def setLayout(self, layout):
        """Not in the reference: capi.LAYOUT_AUTO / LAYOUT_F32W / LAYOUT_PACKED (include/tsdf_hip.h)."""
        self._p.layout = int(layout)

    def getLayout(self):
        """What AUTO resolved to (needs reset())."""
        return int(capi.load().tsdf_hip_layout(self._need()))

    def setZSlab(self, z_begin, z_end, halo=0, device=-1):
        """Not in the reference: own only planes [z_begin, z_end) (multi-GPU Z-slab partition)."""
        self._p.z_begin, self._p.z_end, self._p.halo, self._p.device = int(z_begin), int(z_end), int(halo), int(device)

    def setDevices(self, devices):
        """Not in the reference: spread the volume over several GPUs of this node (tsdf_hip_create_multi): Z-slabs, one
        per entry of `devices` (ordinals may repeat); every method then drives all of them from this one process.
        None / [] = one handle on setZSlab's device."""
        self._devices = [int(d) for d in devices] if devices else None

    def slabs(self):
        """[(device, z_begin, z_end, halo)] of the handle(s) behind this volume."""
        lib, h = capi.load(), self._need()
        out = []
        for k in range(lib.tsdf_hip_slab_count(h)):
            v = [C.c_int32() for _ in range(4)]
            capi.check(lib.tsdf_hip_slab_info(h, k, *[C.byref(x) for x in v]), "slab_info")
            out.append(tuple(x.value for x in v))
        return out

    def renderStats(self):
        """Multi-GPU volumes: (rounds, records handed between slabs, bytes moved between slabs, host waits) of the last
        renderView / renderColoredView."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_multi_render_stats(self._need(), out), "multi_render_stats")
        return tuple(int(v) for v in out)

    def setStream(self, stream_ptr):
        self._stream = stream_ptr
        if self._h:
            capi.check(capi.load().tsdf_hip_set_stream(self._h, C.c_void_p(stream_ptr)), "set_stream")

    def isEmpty(self):
        return self._is_empty

    # -- lifetime ------------------------------------------------------------------------------------
    def reset(self):
        """tsdf_volume_octree.cpp:201-219."""
        lib = capi.load()
        if self._h:
            capi.check(lib.tsdf_hip_destroy(self._h), "destroy")
            self._h = None
        h = C.c_void_p()
        devs = getattr(self, "_devices", None)
        # weight_by_depth_ / weight_by_variance_ (only load() sets them, as in the reference) survive a reset there too
        weighting = tuple(int(v) for v in getattr(self, "_weighting", (0, 0)))
        if any(weighting) and self._p.layout == capi.LAYOUT_AUTO:
            self._p.layout = capi.LAYOUT_F32W
        if devs:
            arr = (C.c_int32 * len(devs))(*devs)
            capi.check(lib.tsdf_hip_create_multi(C.byref(self._p), arr, len(devs), C.byref(h)), "create_multi")
        else:
            capi.check(lib.tsdf_hip_create(C.byref(self._p), C.byref(h)), "create")
        self._h = h
        if any(weighting):
            capi.check(lib.tsdf_hip_set_weighting(h, *weighting), "set_weighting")
        if self._stream is not None and not getattr(self, "_devices", None):  # (a stream belongs to one device)
            capi.check(lib.tsdf_hip_set_stream(self._h, C.c_void_p(self._stream)), "set_stream")
        if getattr(self, "_frame_pairing", False):  # (a multi-GPU set pairs too since round 6: every slab its own ring)
            capi.check(lib.tsdf_hip_set_frame_pairing(self._h, 1), "set_frame_pairing")
        self._is_empty = True

    def close(self):
        if self._h:
            capi.load().tsdf_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need(self):
        if not self._h:
            raise RuntimeError("call reset() first")
        return self._h

    def synchronize(self):
        capi.check(capi.load().tsdf_hip_synchronize(self._need()), "synchronize")

    # -- hot path ------------------------------------------------------------------------------------
    def setReferenceCull(self, flag):
        """Not in the reference's API, but its behaviour: integrateCloud there only visits the voxels pcl::FrustumCulling
        keeps (getFrustumCulledVoxels, tsdf_volume_octree.cpp:619-652).  Default True: every integrate call hands the six
        planes of its pose to the library (tsdf_hip_set_reference_cull), which applies them wherever they can decide a
        voxel -- this volume's voxels are the reference's in every regime.  False: no cull (every voxel updateVoxel
        itself accepts; identical for ordinary cameras, see referenceCullIsNoop())."""
        self._reference_cull = bool(flag)

    def _apply_reference_cull(self, trans):
        lib, h = capi.load(), self._need()
        if getattr(self, "_reference_cull", True):
            planes = reference_cull_planes(self._p, trans)
            capi.check(lib.tsdf_hip_set_reference_cull(h, capi.as_f32p(planes)), "set_reference_cull")
            self._cull_set = True
        elif getattr(self, "_cull_set", False):
            capi.check(lib.tsdf_hip_set_reference_cull(h, None), "set_reference_cull")
            self._cull_set = False

    def integrateCloud(self, depth, bgra=None, trans=None, count=False, pipelined=False):
        """``integrateCloud(cloud, normals, trans)`` (impl/tsdf_volume_octree.hpp:48-103).  Returns True
        (as the reference always does), or the number of observed voxels when ``count`` is set.
        ``pipelined``: return as soon as the frame sits in pinned staging (tsdf_hip_integrate_async); the upload
        overlaps the previous frame's kernel and every later call on this volume is ordered after it."""
        h = self._need()
        trans = np.eye(4) if trans is None else np.asarray(trans, dtype=np.float64)
        depth = capi.f32c(depth)
        if depth.shape != (self._p.image_height, self._p.image_width):
            raise ValueError("depth image must be (image_height, image_width)")
        self._apply_reference_cull(trans)
        T = cam_from_vol_f32(trans)
        n = C.c_uint64(0)
        col = None
        if self._p.integrate_color:
            if bgra is None:
                raise ValueError("integrate_color is set: a (H, W, 4) uint8 bgra image is required")
            col = np.ascontiguousarray(bgra, dtype=np.uint8)
            if col.shape != (self._p.image_height, self._p.image_width, 4):
                raise ValueError("bgra image must be (image_height, image_width, 4)")
        if pipelined and not count:
            capi.check(capi.load().tsdf_hip_integrate_async(h, capi.as_f32p(depth), capi.as_u8p(col) if col is not None else None,
                                                            capi.as_f32p(T)), "integrate_async")
            self._is_empty = False
            return True
        capi.check(
            capi.load().tsdf_hip_integrate(h, capi.as_f32p(depth), capi.as_u8p(col) if col is not None else None,
                                           capi.as_f32p(T), C.byref(n) if count else None), "integrate")
        self._is_empty = False
        return int(n.value) if count else True

    def integrateCloudDevice(self, depth_ptr, bgra_ptr, trans, count=False):
        """Same, with device pointers (frames already resident in HBM); asynchronous unless count."""
        h = self._need()
        self._apply_reference_cull(np.asarray(trans, dtype=np.float64))
        T = cam_from_vol_f32(np.asarray(trans, dtype=np.float64))
        n = C.c_uint64(0)
        capi.check(
            capi.load().tsdf_hip_integrate_device(h, C.c_void_p(depth_ptr), C.c_void_p(bgra_ptr) if bgra_ptr else None,
                                                  capi.as_f32p(T), C.byref(n) if count else None), "integrate_device")
        self._is_empty = False
        return int(n.value) if count else True

    def setFramePairing(self, flag):
        """Not in the reference: pipelined integrateCloud calls (pipelined=True) are integrated two per kernel sweep where
        both poses see the whole volume (tsdf_hip_set_frame_pairing); a frame waits for its partner until the next
        integrateCloud or any other call on the volume.  Same voxels, bit for bit."""
        self._frame_pairing = bool(flag)
        if self._h:
            capi.check(capi.load().tsdf_hip_set_frame_pairing(self._h, int(self._frame_pairing)), "set_frame_pairing")

    def integrateCloudDevice2(self, frame_a, frame_b, count=False):
        """Two frames in one call (tsdf_hip_integrate_device2): each frame = (depth_ptr, bgra_ptr, trans), device pointers
        with the colour image behind the depth image in one allocation.  The voxels are those of two integrateCloudDevice
        calls in this order; where both poses see the whole slab one kernel sweep does both.  Returns (fused, counts):
        counts = the two frames' observed voxels when `count`, else None."""
        h = self._need()
        args = []
        for dp, cp, trans in (frame_a, frame_b):
            trans = np.asarray(trans, dtype=np.float64)
            planes = reference_cull_planes(self._p, trans) if getattr(self, "_reference_cull", True) else None
            args.append((C.c_void_p(dp), C.c_void_p(cp) if cp else None, np.ascontiguousarray(cam_from_vol_f32(trans).reshape(12)), planes))
        n = (C.c_uint64 * 2)()
        fused = C.c_int32(0)
        (da, ca, ta, pa), (db, cb, tb, pb) = args
        capi.check(capi.load().tsdf_hip_integrate_device2(
            h, da, ca, capi.as_f32p(ta), capi.as_f32p(pa) if pa is not None else None,
            db, cb, capi.as_f32p(tb), capi.as_f32p(pb) if pb is not None else None,
            n if count else None, C.byref(fused)), "integrate_device2")
        self._cull_set = args[1][3] is not None
        self._is_empty = False
        return bool(fused.value), ([int(n[0]), int(n[1])] if count else None)

    def organize(self, xyz, bgra=None, cloud_units=1.0, zero_nans=False, world_to_cam=None, fetch=True):
        """The `integrate` program's per-cloud preparation (src/prog/integrate.cpp:559-618) on the GPU: scale,
        (0,0,0) -> NaN, optional world -> camera transform (4x4 = poses[i].inverse()), z-buffer reprojection
        into an organised frame that stays staged in the volume for integrateStaged().  xyz (n, >=3) float32,
        bgra (n, >=4) uint8 in PCL b,g,r,a order.  Returns (depth, bgra, n_valid) when `fetch`."""
        h = self._need()
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n, stride = xyz.shape
        col = np.ascontiguousarray(bgra, dtype=np.uint8) if bgra is not None else None
        H, W = self._p.image_height, self._p.image_width
        depth = np.empty((H, W), np.float32) if fetch else None
        out_c = np.empty((H, W, 4), np.uint8) if fetch else None
        nv = C.c_uint64(0)
        tf = None
        if world_to_cam is not None:
            tf = np.ascontiguousarray(np.asarray(world_to_cam, dtype=np.float64)[:3, :4])
        capi.check(capi.load().tsdf_hip_organize(
            h, capi.as_f32p(xyz), stride, capi.as_u8p(col) if col is not None else None,
            col.shape[1] if col is not None else 0, n, float(cloud_units), int(bool(zero_nans)),
            tf.ctypes.data_as(C.POINTER(C.c_double)) if tf is not None else None,
            capi.as_f32p(depth) if fetch else None, capi.as_u8p(out_c) if fetch else None,
            C.byref(nv) if fetch else None), "organize")
        return (depth, out_c, int(nv.value)) if fetch else None

    def integrateStaged(self, trans=None, count=False):
        """integrateCloud on the frame the last organize() left in the volume."""
        trans = np.eye(4) if trans is None else np.asarray(trans, dtype=np.float64)
        self._apply_reference_cull(trans)  # (as integrateCloud does: the planes belong to this frame's pose)
        T = np.ascontiguousarray(cam_from_vol_f32(trans).reshape(12))
        c = C.c_uint64(0)
        capi.check(capi.load().tsdf_hip_integrate_staged(self._need(), capi.as_f32p(T), C.byref(c) if count else None),
                   "integrate_staged")
        self._is_empty = False
        return int(c.value) if count else True

    def _cubic_for_queries(self, who):
        """The C++ shell REFUSES the queries on a non-cubic setGridSize (TSDFVolumeOctree::cubicForQueries,
        csrc/host/tsdf_volume_octree.cpp: the reference looks per-axis voxel indices, tsdf_volume_octree.cpp:553-574, up in an
        octree that is a cube of edge size_x, octree.cpp:244-266 -- a mixture of two geometries a flat grid does not
        reproduce).  This front end is also what the Z-slab hosts, the bench's slabs and the full-size tests drive, whose
        grids are deliberately flat and non-cubic, so it answers on the flat-grid geometry -- and says so: a
        NonCubicQueryWarning, once per call site (the two front ends used to disagree silently).
        ``strict_noncubic = True`` on the object turns the warning into the C++ shell's refusal (ValueError)."""
        sx, sy, sz = (float(v) for v in self._p.size)
        if sx == sy and sx == sz:
            return
        msg = (f"TSDFVolumeOctree.{who}: grid size {sx:g} x {sy:g} x {sz:g} is not a cube: the reference mixes per-axis closed-form "
               "indices with an octree that is a cube of edge size_x; this answer is for the flat grid's own geometry "
               "(the C++ drop-in refuses this call)")
        if getattr(self, "strict_noncubic", False):
            raise ValueError(msg)
        import warnings
        warnings.warn(msg, NonCubicQueryWarning, stacklevel=3)

    def renderView(self, trans=None, downsampleBy=1, camera_frame=True, pinned=False):
        """tsdf_volume_octree.cpp:278-424.  Returns (H/ds, W/ds, 8) float32: xyz, normal, t*, iterations.
        With camera_frame (the reference's behaviour) xyz/normal are moved back by trans^-1 (:422).
        pinned: the result is a view of a pinned buffer owned by this volume, which the GPU writes by DMA (no host
        copy); it is overwritten by the next pinned renderView of the same size."""
        self._cubic_for_queries("renderView")
        h = self._need()
        trans = np.eye(4) if trans is None else np.asarray(trans, dtype=np.float64)
        ds = int(downsampleBy)
        nh, nw = self._p.image_height // ds, self._p.image_width // ds
        if pinned:
            cache = self.__dict__.setdefault("_pinned_views", {})
            if (nh, nw) not in cache:
                cache[(nh, nw)] = capi.PinnedArray((nh, nw, 8), np.float32)
            out = cache[(nh, nw)].array
        else:
            out = np.empty((nh, nw, 8), dtype=np.float32)
        rot = np.ascontiguousarray(trans[:3, :3].astype(np.float32).reshape(9))
        org = np.ascontiguousarray(trans[:3, 3].astype(np.float32))
        if camera_frame:  # the final transformPointCloudWithNormals(trans^-1) (:422) runs in the kernel
            inv = np.ascontiguousarray(eigen_affine_inverse(trans)[:3, :4], dtype=np.float64)
            capi.check(capi.load().tsdf_hip_raycast_camera(h, capi.as_f32p(rot), capi.as_f32p(org), ds,
                                                           inv.ctypes.data_as(C.POINTER(C.c_double)), capi.as_f32p(out)),
                       "raycast_camera")
        else:
            capi.check(capi.load().tsdf_hip_raycast(h, capi.as_f32p(rot), capi.as_f32p(org), ds, capi.as_f32p(out)),
                       "raycast")
        return out

    def renderColoredView(self, trans=None, downsampleBy=1):
        """tsdf_volume_octree.cpp:426-450: renderView plus, per hit, the colour of the voxel that contains it
        (one batched device lookup).  Returns (cloud (H/ds, W/ds, 8) in the camera frame, rgb (H/ds, W/ds, 3) uint8);
        misses keep 0,0,0; a volume without integrateColor answers 127,127,127 like the reference's NOCOLOR octree."""
        trans = np.eye(4) if trans is None else np.asarray(trans, dtype=np.float64)
        cloud = self.renderView(trans, downsampleBy, camera_frame=True)
        rgb = np.zeros(cloud.shape[:2] + (3,), dtype=np.uint8)
        hit = ~np.isnan(cloud[..., 2])
        if hit.any():
            # :441  v_t = trans.cast<float>() * point  (Eigen: each coefficient m0*x + (m1*y + m2*z) + t [Eigen-recall])
            m = trans.astype(np.float32)
            p = cloud[..., :3][hit]
            q = np.empty_like(p)
            for r in range(3):
                q[:, r] = (m[r, 0] * p[:, 0] + (m[r, 1] * p[:, 1] + m[r, 2] * p[:, 2])) + m[r, 3]
            q = np.ascontiguousarray(q, dtype=np.float32)
            c = np.empty((len(q), 3), np.uint8)
            found = np.empty(len(q), np.uint8)
            capi.check(capi.load().tsdf_hip_lookup_rgb(self._need(), capi.as_f32p(q), len(q), capi.as_u8p(c), capi.as_u8p(found)),
                       "lookup_rgb")
            if not self._p.integrate_color:
                c[:] = 127
            c[found == 0] = 0
            rgb[hit] = c
        return cloud, rgb

    def castRays(self, origins, directions, t_range=None, want_rgb=False, as_given=False):
        """Not in the reference: cast n arbitrary rays into the fused volume on the GPU (tsdf_hip_cast_rays; the definition,
        the admission rule and every refusal are in include/tsdf_hip.h).  ``origins`` / ``directions``: (n, 3) in the volume
        frame, directions used as given (the step rule is the reference's only for unit directions); ``t_range``: (n, 2)
        tmin, tmax per ray, None = the sensor distance bounds.  Returns (out (n, 8) float32: xyz, normal, t*, iterations --
        what ``renderView(camera_frame=False)`` returns for a pixel with that direction, origin and range --, status (n,)
        uint8: 0 miss, 1 hit, 2 not admitted, 3 stopped by the trip cap[, rgb (n, 3) uint8 with ``want_rgb``: the colour of
        the voxel that contains the hit, 0 otherwise; 127,127,127 on a volume without integrateColor, as
        ``renderColoredView``]).  ``as_given``: the rays are already coherent, march them in this order; the results never
        depend on it (and today neither does the order: DESIGN.md 3.23).  One device, a whole-grid volume; no rgb on a "LAB"
        volume."""
        self._cubic_for_queries("castRays")
        h = self._need()
        org = capi.f32c(origins).reshape(-1, 3)
        u = capi.f32c(directions).reshape(-1, 3)
        n = len(org)
        if len(u) != n:
            raise ValueError("origins and directions must have the same length")
        rng = None
        if t_range is not None:
            rng = capi.f32c(t_range).reshape(-1, 2)
            if len(rng) != n:
                raise ValueError("t_range must be (n, 2)")
        out = np.empty((n, 8), np.float32)
        status = np.empty(n, np.uint8)
        rgb = np.empty((n, 3), np.uint8) if want_rgb else None
        capi.check(
            capi.load().tsdf_hip_cast_rays(h, capi.as_f32p(org), capi.as_f32p(u), capi.as_f32p(rng) if rng is not None else None, n,
                                           capi.RAYS_AS_GIVEN if as_given else 0, capi.as_f32p(out), capi.as_u8p(rgb) if want_rgb else None,
                                           capi.as_u8p(status)), "cast_rays")
        if not want_rgb:
            return out, status
        if not self._p.integrate_color:  # the reference's NOCOLOR octree answers 127,127,127 wherever it finds a voxel
            half = [np.float32(s) / np.float32(2) for s in self._p.size]
            found = (status == 1) & (np.abs(out[:, 0]) <= half[0]) & (np.abs(out[:, 1]) <= half[1]) & (np.abs(out[:, 2]) <= half[2])
            rgb[found] = 127
        return out, status, rgb

    def castRaysDevice(self, org_ptr, dir_ptr, t_range_ptr, n, out_ptr, rgb_ptr=0, status_ptr=0, as_given=False):
        """Same, with device pointers on the volume's device (t_range_ptr, rgb_ptr, status_ptr may be 0); asynchronous on the
        volume's stream.  The colour bytes are the library's (0 on a volume without colour)."""
        self._cubic_for_queries("castRays")
        capi.check(
            capi.load().tsdf_hip_cast_rays_device(self._need(), C.c_void_p(org_ptr), C.c_void_p(dir_ptr),
                                                  C.c_void_p(t_range_ptr) if t_range_ptr else None, int(n),
                                                  capi.RAYS_AS_GIVEN if as_given else 0, C.c_void_p(out_ptr),
                                                  C.c_void_p(rgb_ptr) if rgb_ptr else None, C.c_void_p(status_ptr) if status_ptr else None),
            "cast_rays_device")
        return True

    def castRaysStats(self):
        """Report-only, of the last castRays / castRaysDevice: (rays, hits, rays ended with status 2 or 3, device microseconds
        of the call's kernels).  Waits for it to finish."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_cast_rays_stats(self._need(), out), "cast_rays_stats")
        return tuple(int(v) for v in out)

    def getFxn(self, pts):
        """Batched ``getFxn`` (tsdf_volume_octree.cpp:655-672): returns (ok, val)."""
        ok, val, _, _ = self.sample(pts, want_grad=False, want_hess=False)
        return ok, val

    def getGradient(self, pts):
        """Batched ``getGradient`` (tsdf_volume_octree.cpp:681-700): returns (ok, grad (n,3))."""
        ok, _, grad, _ = self.sample(pts, want_hess=False)
        return ok, grad

    def getHessian(self, pts):
        """Batched ``getHessian`` (:703-726): returns (ok, hessian (n,3,3))."""
        ok, _, _, hess = self.sample(pts, want_grad=False)
        return ok, hess

    def getFxnAndGradient(self, pts):
        """:728-738 -- (ok, val, grad)."""
        ok, val, grad, _ = self.sample(pts, want_hess=False)
        return ok, val, grad

    def getFxnGradientAndHessian(self, pts):
        """:740-752 -- (ok, val, grad, hessian)."""
        return self.sample(pts)

    def getVoxelCenter(self, x, y, z):
        """tsdf_volume_octree.cpp:553-560: (i + 0.5) * size / (double)res - size/2 in double, stored as float
        (the closed form; the integrate kernel uses the octree's node centres instead, see centers())."""
        out = []
        for i, a in zip((x, y, z), range(3)):
            size = np.float32(self._p.size[a])
            off = np.float32(np.float64(size) / 2.0)
            out.append(np.float32((np.float64(i) + 0.5) * np.float64(size) / np.float64(self._p.res[a]) - np.float64(off)))
        return tuple(out)

    def getVoxelIndex(self, x, y, z):
        """tsdf_volume_octree.cpp:562-574: (has_voxel, (ix, iy, iz)) with floor(((double)v + size/2) / size * res)."""
        idx = []
        for v, a in zip((x, y, z), range(3)):
            size = np.float64(np.float32(self._p.size[a]))
            q = np.floor((np.float64(np.float32(v)) + size / 2.0) / size * np.float64(self._p.res[a]))
            idx.append(int(q) if np.isfinite(q) and abs(q) < 2 ** 31 else -2 ** 31)  # cvttsd2si on overflow / NaN
        ok = all(0 <= i < r for i, r in zip(idx, self._p.res))
        return ok, tuple(idx)

    def sample(self, pts, want_grad=True, want_hess=True):
        """getFxn / getGradient / getHessian (tsdf_volume_octree.cpp:655-828), batched."""
        self._cubic_for_queries("getFxn / getGradient / getHessian")
        h = self._need()
        pts = capi.f32c(pts).reshape(-1, 3)
        n = pts.shape[0]
        val = np.empty(n, dtype=np.float32)
        grad = np.empty((n, 3), dtype=np.float32) if want_grad else None
        hess = np.empty((n, 9), dtype=np.float32) if want_hess else None
        ok = np.empty(n, dtype=np.uint8)
        capi.check(
            capi.load().tsdf_hip_sample(h, capi.as_f32p(pts), n, capi.as_f32p(val),
                                        capi.as_f32p(grad) if grad is not None else None,
                                        capi.as_f32p(hess) if hess is not None else None, capi.as_u8p(ok)), "sample")
        return ok.astype(bool), val, grad, (hess.reshape(n, 3, 3) if hess is not None else None)

    # -- alignCloud (not in the reference; include/tsdf_hip.h) ---------------------------------------------------------
    @staticmethod
    def _pose12(trans, who):
        m = np.asarray(trans, dtype=np.float64)
        if m.shape not in ((4, 4), (3, 4)):
            raise ValueError(f"{who}: a pose is a 4 x 4 (or 3 x 4) matrix, got shape {m.shape}")
        return np.ascontiguousarray(m[:3, :4]).reshape(12)

    def alignmentSystem(self, points, trans, min_weight=0.0, r_max=0.9, want_used=False, want_points=False):
        """The normal equations of  min_xi sum_i getFxn(exp(xi) * trans * p_i)^2  at xi = 0, reduced on the GPU
        (tsdf_hip_align_system): out (29,) float64 = the 21 upper-triangle entries of sum J J^T (row-major), the 6 of
        sum J r, sum r^2, the number of used points; J = [q x g, g], q = trans * p, r = getFxn(q), g = getGradient(q).
        A point is used iff getFxn succeeds, its eight neighbour voxels all have w > min_weight, and |r| < r_max.
        Returns out, then -- if asked for -- used (n,) bool and the transformed points (n, 3) float32."""
        self._cubic_for_queries("alignmentSystem")
        h = self._need()
        pts = capi.f32c(points).reshape(-1, 3)
        n = pts.shape[0]
        T = self._pose12(trans, "alignmentSystem")
        out = np.empty(29, np.float64)
        used = np.empty(n, np.uint8) if want_used else None
        q = np.empty((n, 3), np.float32) if want_points else None
        f64p = C.POINTER(C.c_double)
        capi.check(capi.load().tsdf_hip_align_system(h, capi.as_f32p(pts), n, T.ctypes.data_as(f64p), float(min_weight), float(r_max),
                                                     out.ctypes.data_as(f64p), capi.as_u8p(used) if want_used else None,
                                                     capi.as_f32p(q) if want_points else None), "align_system")
        res = (out,)
        if want_used:
            res += (used.astype(bool),)
        if want_points:
            res += (q,)
        return res[0] if len(res) == 1 else res

    def alignCloud(self, points, guess, max_iterations=10, min_weight=0.0, r_max=0.9, min_step=1e-7):
        """Register a cloud to the fused surface: Gauss-Newton on the signed distance field (tsdf_hip_align), starting
        from `guess` (source -> volume).  Returns (refined 4 x 4, iterations, cost_log (k, 2): sum r^2 and the used count
        of every system evaluated).  Raises AlignmentError -- carrying the pose of the last good step, the steps taken
        and the cost log -- where no point is used or the cloud does not constrain all six freedoms."""
        self._cubic_for_queries("alignCloud")
        h = self._need()
        pts = capi.f32c(points).reshape(-1, 3)
        n = pts.shape[0]
        T = self._pose12(guess, "alignCloud")
        max_iterations = int(max_iterations)
        refined = np.empty(12, np.float64)
        log = np.full((max(max_iterations, 1), 2), np.nan)
        it = C.c_int32(0)
        f64p = C.POINTER(C.c_double)
        rc = capi.load().tsdf_hip_align(h, capi.as_f32p(pts), n, T.ctypes.data_as(f64p), float(min_weight), float(r_max), max_iterations,
                                        float(min_step), refined.ctypes.data_as(f64p), C.byref(it), log.ctypes.data_as(f64p))
        out = np.eye(4)
        out[:3, :4] = refined.reshape(3, 4)
        log = log[~np.isnan(log[:, 1])]
        if rc in (capi.ALIGN_NO_POINTS, capi.ALIGN_RANK_DEFICIENT):
            raise AlignmentError(rc, out, int(it.value), log)
        capi.check(rc, "align")
        return out, int(it.value), log

    # -- raw access (parity tests, save) -------------------------------------------------------------
    def download(self, x0=0, y0=0, z0=None, nx=None, ny=None, nz=None, want_rgb=None):
        h = self._need()
        rx, ry, rz = self._p.res
        zb = self._p.z_begin
        ze = self._p.z_end if (self._p.z_begin or self._p.z_end) else rz
        z0 = zb if z0 is None else z0
        nx = rx - x0 if nx is None else nx
        ny = ry - y0 if ny is None else ny
        nz = ze - z0 if nz is None else nz
        d = np.empty((nz, ny, nx), dtype=np.float32)
        w = np.empty((nz, ny, nx), dtype=np.float32)
        want_rgb = bool(self._p.integrate_color) if want_rgb is None else want_rgb
        rgb = np.empty((nz, ny, nx, 3), dtype=np.uint8) if want_rgb else None
        capi.check(
            capi.load().tsdf_hip_download(h, x0, y0, z0, nx, ny, nz, capi.as_f32p(d), capi.as_f32p(w),
                                          capi.as_u8p(rgb) if rgb is not None else None), "download")
        return d, w, rgb

    def getOccupiedVoxelIndices(self, box=None, want=()):
        """tsdf_volume_octree.cpp:590-609: the voxels with w > 0 and |d| < 1, in the reference's leaf order (octree
        pre-order = Morton order, x the high bit), found and sorted on the GPU (tsdf_hip_occupied).  Returns idx, an
        (n, 3) int32 array of (x, y, z) -- or, with ``want`` naming any of "d", "w", "rgb", the tuple (idx, *those arrays
        in the order asked): the listed voxels' values as download() gives them.  ``box`` = (x0, y0, z0, nx, ny, nz)
        restricts the query to a block of the planes this volume owns.  Works on setDevices volumes too."""
        lib, h = capi.load(), self._need()
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [k for k in want if k not in ("d", "w", "rgb")]
        if bad:
            raise ValueError(f"getOccupiedVoxelIndices: unknown attribute(s) {bad} (have 'd', 'w', 'rgb')")
        b = (C.c_int32 * 6)(*[int(v) for v in box]) if box is not None else None
        n = C.c_uint64(0)
        capi.check(lib.tsdf_hip_occupied(h, b, C.byref(n)), "occupied")
        n = int(n.value)
        idx = np.empty((n, 3), np.int32)
        out = {"d": np.empty(n, np.float32) if "d" in want else None, "w": np.empty(n, np.float32) if "w" in want else None,
               "rgb": np.empty((n, 3), np.uint8) if "rgb" in want else None}
        capi.check(lib.tsdf_hip_occupied_fetch(h, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                               capi.as_f32p(out["d"]) if out["d"] is not None else None,
                                               capi.as_f32p(out["w"]) if out["w"] is not None else None,
                                               capi.as_u8p(out["rgb"]) if out["rgb"] is not None else None), "occupied_fetch")
        return (idx,) + tuple(out[k] for k in want) if want else idx

    def occupiedStats(self):
        """Report-only, of the last getOccupiedVoxelIndices: (listed voxels, distance bytes the scan requested, 1 if the
        band flags decided what to read, device microseconds of scan + sort)."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_occupied_stats(self._need(), out), "occupied_stats")
        return tuple(int(v) for v in out)

    def shiftVolume(self, sx, sy, sz):
        """Not in the reference: move the volume's window by whole voxels along +x, +y, +z of the volume frame, in place on
        the GPU (tsdf_hip_shift).  Afterwards voxel (x, y, z) holds what (x + sx, y + sy, z + sz) held, or the reset state
        where that lies outside the grid; the band flags move along, so reconstruct / getOccupiedVoxelIndices /
        integrateCloud keep their skips.  Returns ``moved`` (3 float64): the translation of the volume frame in its own
        coordinates, s * size / res.  The world stays where it is: the global transform becomes G * Translation(moved),
        so reconstruct() returns the surviving surface where it was.  What the caller owes in return: a pose handed to
        integrateCloud / renderView / alignCloud afterwards is Translation(-moved) * trans_old.  Works on setDevices
        volumes; a setZSlab volume shifts along x and y only."""
        h = self._need()
        s = (C.c_int32 * 3)(int(sx), int(sy), int(sz))
        capi.check(capi.load().tsdf_hip_shift(h, s), "shift")
        moved = np.array([int(s[a]) * float(self._p.size[a]) / int(self._p.res[a]) for a in range(3)], dtype=np.float64)
        t = np.eye(4)
        t[:3, 3] = moved
        self._global_transform = self._global_transform @ t
        return moved

    def shiftStats(self):
        """Report-only, of the last shiftVolume: (voxels that kept a value, voxels reset, 1 if the band flags were carried
        over, device microseconds).  Waits for the shift to finish."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_shift_stats(self._need(), out), "shift_stats")
        return tuple(int(v) for v in out)

    def mergeVolume(self, src, dst_from_src=None, min_weight=0.0, count=False):
        """Not in the reference: resample volume ``src`` at this volume's voxel centres and add the samples as weighted
        observations, on the GPU (tsdf_hip_merge; the rule and every refusal are in include/tsdf_hip.h).  ``dst_from_src``
        (4 x 4 or 3 x 4) takes src volume coordinates to this volume's; None = the two global transforms,
        getGlobalTransform()^-1 * src.getGlobalTransform().  A voxel is merged iff getFxn(src, q) succeeds at its centre q,
        the eight neighbour voxels there all have w > min_weight, and src has a voxel containing q, whose weight and colour
        the observation carries.  Returns True, or the number of merged voxels when ``count`` is set (the call then waits).
        src is unchanged; this volume's band flags are dropped as by upload().  One device, whole-grid volumes, "RGB"
        colour, no depth / variance weighting, src cubic; a PACKED volume takes a PACKED src with the same weight limit."""
        h, hs = self._need(), src._need()
        if dst_from_src is None:
            m = np.linalg.inv(self._global_transform) @ src._global_transform
        else:
            m = np.asarray(dst_from_src, dtype=np.float64)
            if m.shape not in ((4, 4), (3, 4)):
                raise ValueError(f"mergeVolume: a transform is a 4 x 4 (or 3 x 4) matrix, got shape {m.shape}")
            m = np.vstack([m[:3, :4], [0.0, 0.0, 0.0, 1.0]])
        with np.errstate(all="ignore"):
            try:
                inv = np.linalg.inv(m)
            except np.linalg.LinAlgError:
                raise ValueError("mergeVolume: dst_from_src cannot be inverted") from None
        T = np.ascontiguousarray(inv[:3, :4]).reshape(12)
        n = C.c_uint64(0)
        capi.check(capi.load().tsdf_hip_merge(h, hs, T.ctypes.data_as(C.POINTER(C.c_double)), float(min_weight),
                                              C.byref(n) if count else None), "merge")
        self._is_empty = self._is_empty and src._is_empty
        return int(n.value) if count else True

    def mergeStats(self):
        """Report-only, of the last mergeVolume into this volume: (voxels in the launch box, voxels merged, 1 if live band
        flags had to be dropped, device microseconds).  Waits for the merge to finish."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_merge_stats(self._need(), out), "merge_stats")
        return tuple(int(v) for v in out)

    def deintegrateCloud(self, depth, bgra=None, trans=None, count=False):
        """Not in the reference: take a frame back out of the volume on the GPU (tsdf_hip_deintegrate; the rule and every
        refusal are in include/tsdf_hip.h) -- ``integrateCloud``'s arguments, with the pose the frame was integrated under.
        The frame, the pose and the reference cull select exactly the voxels integrateCloud observed, with the same
        distance and colour; each loses one count and that observation from its running means, and a voxel whose weight
        reaches 0 returns to the reset state.  A voxel at the weight limit has forgotten how many frames it saw and loses
        one count like any other.  The band flags survive: reconstruct / getOccupiedVoxelIndices / integrateCloud keep
        their skips.  Returns True, or the number of voxels whose weight went down when ``count`` is set.  "RGB" colour,
        no depth / variance weighting, not on setDevices volumes."""
        h = self._need()
        trans = np.eye(4) if trans is None else np.asarray(trans, dtype=np.float64)
        depth = capi.f32c(depth)
        if depth.shape != (self._p.image_height, self._p.image_width):
            raise ValueError("depth image must be (image_height, image_width)")
        col = None
        if self._p.integrate_color:
            if bgra is None:
                raise ValueError("integrate_color is set: a (H, W, 4) uint8 bgra image is required")
            col = np.ascontiguousarray(bgra, dtype=np.uint8)
            if col.shape != (self._p.image_height, self._p.image_width, 4):
                raise ValueError("bgra image must be (image_height, image_width, 4)")
        self._apply_reference_cull(trans)
        T = cam_from_vol_f32(trans)
        n = C.c_uint64(0)
        capi.check(
            capi.load().tsdf_hip_deintegrate(h, capi.as_f32p(depth), capi.as_u8p(col) if col is not None else None,
                                             capi.as_f32p(T), C.byref(n) if count else None), "deintegrate")
        return int(n.value) if count else True

    def deintegrateCloudDevice(self, depth_ptr, bgra_ptr, trans, count=False):
        """Same, with device pointers (the frame already resident in HBM); asynchronous unless count."""
        h = self._need()
        self._apply_reference_cull(np.asarray(trans, dtype=np.float64))
        T = cam_from_vol_f32(np.asarray(trans, dtype=np.float64))
        n = C.c_uint64(0)
        capi.check(
            capi.load().tsdf_hip_deintegrate_device(h, C.c_void_p(depth_ptr), C.c_void_p(bgra_ptr) if bgra_ptr else None,
                                                    capi.as_f32p(T), C.byref(n) if count else None), "deintegrate_device")
        return int(n.value) if count else True

    def deintegrateStats(self):
        """Report-only: (voxels the frame selected, voxels whose weight went down, of those the voxels that returned to
        unobserved -- all three of the last deintegrateCloud with ``count`` --, device microseconds of the last one's
        kernel).  Waits for it to finish."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_deintegrate_stats(self._need(), out), "deintegrate_stats")
        return tuple(int(v) for v in out)

    def _repose_args(self, old_trans, new_trans):
        """(T_old, planes_old, T_new, planes_new) of a re-pose: float32 arrays, planes None with setReferenceCull off."""
        out = []
        for trans in (old_trans, new_trans):
            trans = np.eye(4) if trans is None else np.asarray(trans, dtype=np.float64)
            planes = reference_cull_planes(self._p, trans) if getattr(self, "_reference_cull", True) else None
            out += [np.ascontiguousarray(cam_from_vol_f32(trans).reshape(12)), planes]
        return out

    def reintegrateCloud(self, depth, bgra=None, old_trans=None, new_trans=None, count=False):
        """Not in the reference: re-pose a fused frame in one sweep of the volume on the GPU (tsdf_hip_reintegrate; the
        definition and every refusal are in include/tsdf_hip.h) -- what a corrected pose from a pose graph asks of the map.
        The voxels come out, bit for bit, as ``deintegrateCloud(depth, bgra, old_trans)`` followed by
        ``integrateCloud(depth, bgra, new_trans)`` leaves them, each half with the reference-cull planes of its own pose
        (setReferenceCull, on by default), but every word is read and written once, and the band flags survive where the
        two calls lose them: reconstruct / getOccupiedVoxelIndices / integrateCloud keep their skips.  The saturation caveat
        of deintegrateCloud is inherited.  Returns True, or (voxels whose weight went down, voxels observed under the new
        pose) when ``count`` is set.  "RGB" colour, no depth / variance weighting, not on setDevices volumes."""
        h = self._need()
        depth = capi.f32c(depth)
        if depth.shape != (self._p.image_height, self._p.image_width):
            raise ValueError("depth image must be (image_height, image_width)")
        col = None
        if self._p.integrate_color:
            if bgra is None:
                raise ValueError("integrate_color is set: a (H, W, 4) uint8 bgra image is required")
            col = np.ascontiguousarray(bgra, dtype=np.uint8)
            if col.shape != (self._p.image_height, self._p.image_width, 4):
                raise ValueError("bgra image must be (image_height, image_width, 4)")
        To, po, Tn, pn = self._repose_args(old_trans, new_trans)
        n = (C.c_uint64 * 2)()
        capi.check(
            capi.load().tsdf_hip_reintegrate(h, capi.as_f32p(depth), capi.as_u8p(col) if col is not None else None,
                                             capi.as_f32p(To), capi.as_f32p(po) if po is not None else None,
                                             capi.as_f32p(Tn), capi.as_f32p(pn) if pn is not None else None,
                                             n if count else None), "reintegrate")
        self._cull_set = pn is not None
        self._is_empty = False
        return (int(n[0]), int(n[1])) if count else True

    def reintegrateCloudDevice(self, depth_ptr, bgra_ptr, old_trans, new_trans, count=False):
        """Same, with device pointers (the frame already resident in HBM); asynchronous unless count."""
        h = self._need()
        To, po, Tn, pn = self._repose_args(old_trans, new_trans)
        n = (C.c_uint64 * 2)()
        capi.check(
            capi.load().tsdf_hip_reintegrate_device(h, C.c_void_p(depth_ptr), C.c_void_p(bgra_ptr) if bgra_ptr else None,
                                                    capi.as_f32p(To), capi.as_f32p(po) if po is not None else None,
                                                    capi.as_f32p(Tn), capi.as_f32p(pn) if pn is not None else None,
                                                    n if count else None), "reintegrate_device")
        self._cull_set = pn is not None
        self._is_empty = False
        return (int(n[0]), int(n[1])) if count else True

    def reintegrateStats(self):
        """Report-only: (voxels the old pose selected, voxels whose weight went down, of those the voxels the removal took
        back to unobserved, voxels the new pose observed, voxels both poses selected -- all five of the last
        reintegrateCloud with ``count`` --, device microseconds of the last one's kernel).  Waits for it to finish."""
        out = (C.c_uint64 * 6)()
        capi.check(capi.load().tsdf_hip_reintegrate_stats(self._need(), out), "reintegrate_stats")
        return tuple(int(v) for v in out)

    def computeDistanceField(self, r_max=0, min_weight=0.0, box=None):
        """Not in the reference: the exact Euclidean distance transform of the volume's zero crossing, on the GPU
        (tsdf_hip_esdf; the rule and every refusal are in include/tsdf_hip.h).  A voxel of ``box`` = (x0, y0, z0, nx, ny, nz)
        (None: the whole grid) is a site iff it is observed (w > min_weight, d not NaN) and a 6-neighbour inside the grid is
        observed with the other sign of d; every voxel of the box then gets the squared distance, in voxels, to the nearest
        site of the box -- exact integers, FAR (0xFFFFFFFF) above ``r_max``^2 when r_max > 0.  Returns the number of sites.
        The field stays on the volume, describing it as it was at this call, until reset(), close() or the next
        computeDistanceField; after shiftVolume it has to be computed again.  One device, a whole-grid volume with cubic
        voxels on a cubic grid."""
        b = (C.c_int32 * 6)(*[int(v) for v in box]) if box is not None else None
        n = C.c_uint64(0)
        capi.check(capi.load().tsdf_hip_esdf(self._need(), b, int(r_max), float(min_weight), C.byref(n)), "esdf")
        self._esdf_shape = tuple(int(v) for v in (box[5], box[4], box[3])) if box is not None else tuple(int(v) for v in self._p.res)[::-1]
        return int(n.value)

    def getDistanceField(self):
        """(d2, dist) of the last computeDistanceField, each of shape (nz, ny, nx) of its box: d2 uint32 squared voxel
        distances (FAR = 0xFFFFFFFF), dist float32 metres = sgn * voxel * sqrt(d2), negative where the voxel was observed with
        d < 0, +-inf where FAR."""
        shape = getattr(self, "_esdf_shape", (0, 0, 0))
        d2, dist = np.empty(shape, np.uint32), np.empty(shape, np.float32)
        capi.check(capi.load().tsdf_hip_esdf_fetch(self._need(), d2.ctypes.data_as(C.POINTER(C.c_uint32)), capi.as_f32p(dist)), "esdf_fetch")
        return d2, dist

    def getDistance(self, points):
        """(dist, found) for an (n, 3) array of points in volume coordinates: the distance-field value of the voxel that
        contains each point (no interpolation).  found is False, and dist NaN, where no voxel contains the point or that
        voxel lies outside the field's box."""
        pts = capi.f32c(points).reshape(-1, 3)
        n = len(pts)
        dist, found = np.empty(n, np.float32), np.empty(n, np.uint8)
        if n:
            capi.check(capi.load().tsdf_hip_esdf_sample(self._need(), capi.as_f32p(pts), n, capi.as_f32p(dist), capi.as_u8p(found)), "esdf_sample")
        return dist, found.astype(bool)

    def distanceFieldStats(self):
        """Report-only, of the last computeDistanceField: (voxels of the box, sites, bytes of device memory the field and
        its scratch hold, device microseconds of the three passes)."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.load().tsdf_hip_esdf_stats(self._need(), out), "esdf_stats")
        return tuple(int(v) for v in out)

    def occupiedTiming(self):
        """Report-only: device milliseconds (scan, sort, gather) of the last getOccupiedVoxelIndices."""
        ms = (C.c_float * 3)()
        capi.check(capi.load().tsdf_hip_occupied_timing(self._need(), ms), "occupied_timing")
        return tuple(float(v) for v in ms)

    def referenceCullIsNoop(self):
        """Not in the reference: True if its frustum cull (tsdf_volume_octree.cpp:619-652) cannot change results for the
        configured camera, i.e. this volume's voxels equal the reference's (tsdf_hip_reference_cull_is_noop)."""
        return bool(capi.load().tsdf_hip_reference_cull_is_noop(C.byref(self._p)))

    def downloadColorState(self, z0=None, nz=None):
        """Not in the reference (its members are public): the float colour state of "RGBNormalized" (r_n, g_n, b_n, i)
        or "LAB" (L, A, B) voxels as an array (planes, nz, ny, nx)."""
        h = self._need()
        rx, ry, rz = self._p.res
        zb = self._p.z_begin
        ze = self._p.z_end if (self._p.z_begin or self._p.z_end) else rz
        z0 = zb if z0 is None else z0
        nz = ze - z0 if nz is None else nz
        planes = {capi.COLOR_RGB_NORMALIZED: 4, capi.COLOR_LAB: 3}.get(self._p.color_mode, 0)
        out = np.empty((planes, nz, ry, rx), dtype=np.float32)
        for c in range(planes):
            capi.check(capi.load().tsdf_hip_download_color_state(h, c, z0, nz, capi.as_f32p(out[c])), "colour state")
        return out

    def setWeighting(self, by_depth=False, by_variance=False):
        """Not in the reference (its two flags only arrive through load()): hpp:200-204 on this volume from the next
        reset() on -- F32W layout, plain kernel; tests use it."""
        self._weighting = (bool(by_depth), bool(by_variance))

    def downloadVarianceState(self):
        """(M, nsample) of every voxel: OctreeNode::M_ / nsample_ (octree.h:164-165), kept by volumes that weight by variance."""
        rx, ry, rz = self._p.res
        M, ns = np.empty((rz, ry, rx), np.float32), np.empty((rz, ry, rx), np.int32)
        capi.check(capi.load().tsdf_hip_download_variance_state(self._need(), 0, 0, 0, rx, ry, rz, capi.as_f32p(M),
                                                                ns.ctypes.data_as(C.POINTER(C.c_int32))), "download_variance_state")
        return M, ns

    def uploadVarianceState(self, M, nsample):
        rx, ry, rz = self._p.res
        M, ns = np.ascontiguousarray(M, np.float32), np.ascontiguousarray(nsample, np.int32)
        assert M.shape == ns.shape == (rz, ry, rx)
        capi.check(capi.load().tsdf_hip_upload_variance_state(self._need(), 0, 0, 0, rx, ry, rz, capi.as_f32p(M),
                                                              ns.ctypes.data_as(C.POINTER(C.c_int32))), "upload_variance_state")

    def upload(self, d=None, w=None, rgb=None, x0=0, y0=0, z0=0):
        h = self._need()
        ref = d if d is not None else (w if w is not None else rgb)
        nz, ny, nx = ref.shape[:3]
        d = capi.f32c(d) if d is not None else None
        w = capi.f32c(w) if w is not None else None
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8) if rgb is not None else None
        capi.check(
            capi.load().tsdf_hip_upload(h, x0, y0, z0, nx, ny, nz, capi.as_f32p(d) if d is not None else None,
                                        capi.as_f32p(w) if w is not None else None,
                                        capi.as_u8p(rgb) if rgb is not None else None), "upload")
        self._is_empty = False

    # -- save / load: tsdf_volume_octree.cpp:222-275 ---------------------------------------------------
    def save(self, filename):
        """The reference's .vol checkpoint (tsdf_hip_save); streamed, host memory stays at one 256^3 block."""
        m = capi.TsdfVolMeta()
        # setMaxVoxelSize, else the reference's default 0.5 m (tsdf_volume_octree.cpp:72-74) -- what the C++ class writes
        cell = getattr(self, "_max_cell", None) or (0.5, 0.5, 0.5)
        m.max_cell_size[:] = cell
        m.is_empty = int(self._is_empty)
        m.weight_by_depth, m.weight_by_variance = (int(v) for v in getattr(self, "_weighting", (0, 0)))
        m.global_transform[:] = [float(v) for v in self._global_transform.reshape(16)]
        capi.check(capi.load().tsdf_hip_save(self._need(), str(filename).encode(), C.byref(m)), "save")

    def load(self, filename):
        """Replace this volume by the one in `filename` (written by either side).  Device, layout and
        transform order stay as set on this object."""
        lib = capi.load()
        h, p, m = C.c_void_p(), capi.TsdfParams(), capi.TsdfVolMeta()
        defaults = capi.TsdfParams.from_buffer_copy(self._p)
        defaults.z_begin = defaults.z_end = defaults.halo = 0
        devs = getattr(self, "_devices", None)
        if devs:
            arr = (C.c_int32 * len(devs))(*devs)
            capi.check(lib.tsdf_hip_load_multi(str(filename).encode(), C.byref(defaults), arr, len(devs), C.byref(h), C.byref(p),
                                               C.byref(m)), "load_multi")
        else:
            capi.check(lib.tsdf_hip_load(str(filename).encode(), C.byref(defaults), C.byref(h), C.byref(p), C.byref(m)), "load")
        self.close()
        asked = self._p.layout
        self._h, self._p = h, p
        if not (asked == capi.LAYOUT_AUTO and p.layout == capi.LAYOUT_F32W and 0 <= p.max_weight <= 255):
            self._p.layout = asked
        if self._stream is not None and not getattr(self, "_devices", None):  # (a stream belongs to one device)
            capi.check(lib.tsdf_hip_set_stream(self._h, C.c_void_p(self._stream)), "set_stream")
        self._max_cell = tuple(m.max_cell_size)
        self._is_empty = bool(m.is_empty)
        # hpp:200-204: the handle integrates depth-weighted / refuses to integrate variance-weighted from here on
        self._weighting = (bool(m.weight_by_depth), bool(m.weight_by_variance))
        self._global_transform = np.array(list(m.global_transform), dtype=np.float64).reshape(4, 4)

    def centers(self, axis):
        out = np.empty(self._p.res[axis], dtype=np.float32)
        capi.check(capi.load().tsdf_hip_centers(self._need(), axis, capi.as_f32p(out)), "centers")
        return out

    def device_planes(self):
        d, w, rgb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        pitch, zf, nza = C.c_int64(), C.c_int32(), C.c_int32()
        capi.check(
            capi.load().tsdf_hip_device_planes(self._need(), C.byref(d), C.byref(w), C.byref(rgb), C.byref(pitch),
                                               C.byref(zf), C.byref(nza)), "device_planes")
        return d.value, w.value, rgb.value, pitch.value, zf.value, nza.value


class MarchingCubesTSDFOctree:
    """Drop-in for ``cpu_tsdf::MarchingCubesTSDFOctree`` (include/cpu_tsdf/marching_cubes_tsdf_octree.h)."""

    def __init__(self):
        self._w_min = 2.5  # marching_cubes_tsdf_octree.h:58
        self._by_rgb = False
        self._by_conf = False
        self._vol = None
        self._cleanup = None
        self._flatten = None
        self._decimate = None
        self._smooth = None
        self._normals = False

    def setCleanup(self, face_dist=0.02, min_neighbors=5):
        """Extension (no reference counterpart on the class): reconstruct() drops the faces in connected groups of at most
        `min_neighbors` faces -- the `integrate` program's --cleanup (src/prog/integrate.cpp:152-214) -- on the GPU, between
        the march and the fetch (tsdf_hip_march_cleanup).  It acts in the VOLUME frame, before the global transform, and,
        unlike the program's pass, keeps the colours."""
        face_dist, min_neighbors = float(face_dist), int(min_neighbors)
        if not (np.isfinite(face_dist) and face_dist > 0) or min_neighbors < 0:
            raise ValueError("setCleanup: face_dist must be finite and positive, min_neighbors >= 0")
        self._cleanup = (face_dist, min_neighbors)

    def clearCleanup(self):
        self._cleanup = None

    def setFlatten(self, min_dist=0.0001):
        """Extension (no reference counterpart on the class): reconstruct() merges the vertices closer than `min_dist` -- the
        `integrate` program's --flatten (src/prog/integrate.cpp:103-150) -- on the GPU, between the march and the fetch
        (tsdf_hip_march_flatten), and returns the INDEXED mesh.  It acts in the VOLUME frame, before the global transform,
        and, unlike the program's pass, keeps the colours: an output vertex has the colour of its seed vertex.  With
        setCleanup as well, the cleanup runs FIRST, on the soup, and flatten second.  The `integrate` program uses the other
        order, as the reference does (flatten, then cleanup on the indexed mesh), which is why it goes through the
        host-array entry points (tsdf_hip_mesh_flatten, tsdf_hip_mesh_cleanup) instead."""
        min_dist = float(min_dist)
        if not (np.isfinite(min_dist) and min_dist > 0):
            raise ValueError("setFlatten: min_dist must be finite and positive")
        self._flatten = min_dist

    def clearFlatten(self):
        self._flatten = None

    def setDecimate(self, cell_size):
        """Extension (no reference counterpart): reconstruct() decimates the mesh by vertex clustering on a grid of edge
        `cell_size` (metres, VOLUME frame, before the global transform) -- on the GPU, between the march and the fetch
        (tsdf_hip_march_decimate) -- and returns the INDEXED mesh: one vertex per occupied cell, the mean of the cell's
        vertices (colours: the rounded mean), faces re-indexed, degenerate and duplicate faces dropped (include/tsdf_hip.h
        states the rules).  With setCleanup as well, the cleanup runs FIRST, on the soup.  With setFlatten as well,
        decimate runs and flatten is skipped: clustering already merges what flatten would."""
        cell_size = float(cell_size)
        if not (np.isfinite(cell_size) and cell_size > 0):
            raise ValueError("setDecimate: cell_size must be finite and positive")
        self._decimate = cell_size

    def clearDecimate(self):
        self._decimate = None

    def setSmooth(self, iterations, lam=0.5, mu=-0.53, keep_boundary=True):
        """Extension (no reference counterpart): reconstruct() smooths the INDEXED mesh last -- Taubin's lambda | mu:
        `iterations` times a step with `lam` and, iff mu != 0, a step with `mu`; keep_boundary fixes the endpoints of boundary
        edges (tsdf_hip_march_smooth; include/tsdf_hip.h states the rules).  It acts in the VOLUME frame, before the global
        transform, and moves the vertices only.  With neither setFlatten nor setDecimate, flatten runs first at its default
        min_dist: a soup has no shared vertices to smooth over."""
        iterations, lam, mu = int(iterations), float(lam), float(mu)
        if not (np.isfinite(lam) and 0 < lam <= 1) or not (np.isfinite(mu) and -1 <= mu <= 0) or not 0 <= iterations <= 1000:
            raise ValueError("setSmooth: lam must be in (0, 1], mu in [-1, 0], iterations in [0, 1000]")
        self._smooth = (iterations, lam, mu, bool(keep_boundary))

    def clearSmooth(self):
        self._smooth = None

    def setNormals(self, on=True):
        """Extension (no reference counterpart): reconstruct() computes area-weighted vertex normals LAST of all -- after
        cleanup, flatten / decimate and smooth -- from the mesh it returns, the soup included (tsdf_hip_march_normals;
        include/tsdf_hip.h states the rule and the orientation: out of the surface, into observed free space), and adds
        "normals" (float32, one row per returned vertex) to its dict.  They are computed in the VOLUME frame and turned by the
        global transform's rotation."""
        self._normals = bool(on)

    def setInputTSDF(self, volume):
        self._vol = volume

    def setMinWeight(self, w_min):
        self._w_min = float(w_min)

    def setColorByRGB(self, flag):
        self._by_rgb = bool(flag)

    def setColorByConfidence(self, flag):
        self._by_conf = bool(flag)

    def reconstruct(self, want_cells=False):
        """marching_cubes_tsdf_octree.cpp:108-143.  Returns dict(vertices (3n,3) float32 after the global
        transform, polygons (n,3) int32 = [3i,3i+1,3i+2], rgb (3n,3) uint8 or None, cells).  With setFlatten: the indexed
        mesh -- vertices (m,3), polygons (k,3) int32 into them, rgb (m,3) or None, cells (k,); with setDecimate and with
        setSmooth likewise.  With setNormals: also normals, float32, one row per returned vertex."""
        vol = self._vol
        vol._cubic_for_queries("MarchingCubesTSDFOctree.reconstruct")
        h = vol._need()
        lib = capi.load()
        mode = 2 if self._by_conf else (1 if self._by_rgb else 0)
        n = C.c_uint64(0)
        capi.check(lib.tsdf_hip_march(h, self._w_min, mode, C.byref(n)), "march")
        if self._cleanup is not None:
            capi.check(lib.tsdf_hip_march_cleanup(h, self._cleanup[0], self._cleanup[1], C.byref(n)), "march_cleanup")
        if self._decimate is not None or self._flatten is not None or self._smooth is not None:
            return self._fetch_indexed(vol, h, mode, want_cells)
        nt = int(n.value)
        verts = np.empty((nt * 3, 3), dtype=np.float32)
        rgb = np.empty((nt * 3, 3), dtype=np.uint8) if mode else None
        cells = np.empty(nt, dtype=np.uint64) if want_cells else None
        if nt:
            capi.check(
                lib.tsdf_hip_march_fetch(h, capi.as_f32p(verts), capi.as_u8p(rgb) if rgb is not None else None,
                                         cells.ctypes.data_as(C.POINTER(C.c_uint64)) if cells is not None else None),
                "march_fetch")
        g = vol.getGlobalTransform()
        if not np.array_equal(g, np.eye(4)):
            verts = transform_points_f64(verts, g)
        polys = np.arange(nt * 3, dtype=np.int32).reshape(nt, 3)
        out = {"vertices": verts, "polygons": polys, "rgb": rgb, "cells": cells}
        if self._normals:
            out["normals"] = self._fetch_normals(h, nt * 3, g)
        return out

    def _fetch_indexed(self, vol, h, mode, want_cells):
        lib = capi.load()
        m, k = C.c_uint64(0), C.c_uint64(0)
        if self._decimate is not None:
            capi.check(lib.tsdf_hip_march_decimate(h, self._decimate, C.byref(m), C.byref(k)), "march_decimate")
        else:
            capi.check(lib.tsdf_hip_march_flatten(h, 0.0001 if self._flatten is None else self._flatten, C.byref(m), C.byref(k)), "march_flatten")
        if self._smooth is not None:
            it, lam, mu, keep = self._smooth
            capi.check(lib.tsdf_hip_march_smooth(h, lam, mu, it, 1 if keep else 0, None), "march_smooth")
        m, k = int(m.value), int(k.value)
        verts = np.empty((m, 3), dtype=np.float32)
        rgb = np.empty((m, 3), dtype=np.uint8) if mode else None
        faces = np.empty((k, 3), dtype=np.uint32)
        cells = np.empty(k, dtype=np.uint64) if want_cells else None
        if m:
            capi.check(
                lib.tsdf_hip_march_fetch_indexed(h, capi.as_f32p(verts), capi.as_u8p(rgb) if rgb is not None else None,
                                                 faces.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 cells.ctypes.data_as(C.POINTER(C.c_uint64)) if cells is not None else None),
                "march_fetch_indexed")
        g = vol.getGlobalTransform()
        if not np.array_equal(g, np.eye(4)):
            verts = transform_points_f64(verts, g)
        out = {"vertices": verts, "polygons": faces.astype(np.int32), "rgb": rgb, "cells": cells}
        if self._normals:
            out["normals"] = self._fetch_normals(h, m, g)
        return out

    @staticmethod
    def _fetch_normals(h, n_expected, g):
        lib = capi.load()
        n = C.c_uint64(0)
        capi.check(lib.tsdf_hip_march_normals(h, C.byref(n), None), "march_normals")
        if int(n.value) != n_expected:
            raise RuntimeError(f"march_normals describes {int(n.value)} vertices, the mesh has {n_expected}")
        normals = np.zeros((n_expected, 3), dtype=np.float32)
        if n_expected:
            capi.check(lib.tsdf_hip_march_fetch_normals(h, capi.as_f32p(normals)), "march_fetch_normals")
        if not np.array_equal(g[:3, :3], np.eye(3)):  # turned like the vertices, in the C++ class' order of operations
            r, n64 = np.asarray(g, np.float64)[:3, :3], normals.astype(np.float64)
            normals = (n64[:, 0:1] * r[:, 0] + (n64[:, 1:2] * r[:, 1] + n64[:, 2:3] * r[:, 2])).astype(np.float32)
        return normals


def cleanup_mesh(vertices, polygons=None, face_dist=0.02, min_neighbors=5, device=0):
    """Which faces survive the `integrate` program's --cleanup (src/prog/integrate.cpp:152-214), computed on the GPU
    (tsdf_hip_mesh_cleanup): a boolean keep mask, one entry per face.  vertices (n, 3) float32; polygons (m, 3) vertex
    indices, or None for a triangle soup (face f = vertices 3f, 3f+1, 3f+2)."""
    verts = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = None if polygons is None else np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    if faces is None and len(verts) % 3:
        raise ValueError("cleanup_mesh: a triangle soup needs 3 vertices per face")
    n_faces = len(verts) // 3 if faces is None else len(faces)
    keep = np.zeros(n_faces, dtype=np.uint8)
    kept = C.c_uint64(0)
    capi.check(
        capi.load().tsdf_hip_mesh_cleanup(int(device), capi.as_f32p(verts), len(verts),
                                          faces.ctypes.data_as(C.POINTER(C.c_uint32)) if faces is not None else None, n_faces,
                                          float(face_dist), int(min_neighbors), capi.as_u8p(keep), C.byref(kept)), "mesh_cleanup")
    return keep.astype(bool)


def flatten_mesh(vertices, polygons=None, min_dist=0.0001, device=0):
    """The `integrate` program's --flatten (src/prog/integrate.cpp:103-150) computed on the GPU (tsdf_hip_mesh_flatten):
    vertices closer than min_dist are merged, faces re-indexed, a face with two equal corners dropped.  vertices (n, 3)
    float32; polygons (k0, 3) vertex indices, or None for a triangle soup (face f = vertices 3f, 3f+1, 3f+2).  Returns
    dict(vertices (m, 3) float32, polygons (k, 3) int32, remap (n,) uint32: output vertex of each input vertex, seeds (m,)
    uint32: input vertex of each output vertex)."""
    verts = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = None if polygons is None else np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    if faces is None and len(verts) % 3:
        raise ValueError("flatten_mesh: a triangle soup needs 3 vertices per face")
    n_faces = len(verts) // 3 if faces is None else len(faces)
    u32p = C.POINTER(C.c_uint32)
    remap = np.zeros(len(verts), dtype=np.uint32)
    seeds = np.zeros(len(verts), dtype=np.uint32)
    out_faces = np.zeros((n_faces, 3), dtype=np.uint32)
    m, k = C.c_uint64(0), C.c_uint64(0)
    capi.check(
        capi.load().tsdf_hip_mesh_flatten(int(device), capi.as_f32p(verts), len(verts),
                                          faces.ctypes.data_as(u32p) if faces is not None else None, n_faces, float(min_dist),
                                          remap.ctypes.data_as(u32p), seeds.ctypes.data_as(u32p), C.byref(m),
                                          out_faces.ctypes.data_as(u32p), C.byref(k)), "mesh_flatten")
    seeds = seeds[:int(m.value)].copy()
    return {"vertices": verts[seeds], "polygons": out_faces[:int(k.value)].astype(np.int32), "remap": remap, "seeds": seeds}


def decimate_mesh(vertices, polygons=None, colors=None, cell_size=None, device=0):
    """Vertex clustering on the GPU (tsdf_hip_mesh_decimate; include/tsdf_hip.h states the rules): one output vertex per
    occupied cell of a grid of edge `cell_size` -- the mean of the cell's vertices, and of their colours -- faces re-indexed,
    degenerate and duplicate faces dropped.  vertices (n, 3) float32; polygons (k0, 3) vertex indices, or None for a triangle
    soup (face f = vertices 3f, 3f+1, 3f+2); colors (n, 3) uint8 or None.  Returns dict(vertices (m, 3) float32, polygons
    (k, 3) int32, rgb (m, 3) uint8 or None, remap (n,) uint32: output vertex of each input vertex, counts (m,) uint32:
    members of each output vertex)."""
    if cell_size is None:
        raise ValueError("decimate_mesh: cell_size is required")
    verts = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = None if polygons is None else np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    rgb = None if colors is None else np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    if faces is None and len(verts) % 3:
        raise ValueError("decimate_mesh: a triangle soup needs 3 vertices per face")
    if rgb is not None and len(rgb) != len(verts):
        raise ValueError("decimate_mesh: one colour per vertex")
    n_faces = len(verts) // 3 if faces is None else len(faces)
    u32p = C.POINTER(C.c_uint32)
    remap = np.zeros(len(verts), dtype=np.uint32)
    out_verts = np.zeros((len(verts), 3), dtype=np.float32)
    out_rgb = np.zeros((len(verts), 3), dtype=np.uint8) if rgb is not None else None
    counts = np.zeros(len(verts), dtype=np.uint32)
    out_faces = np.zeros((n_faces, 3), dtype=np.uint32)
    m, k = C.c_uint64(0), C.c_uint64(0)
    capi.check(
        capi.load().tsdf_hip_mesh_decimate(int(device), capi.as_f32p(verts), capi.as_u8p(rgb) if rgb is not None else None, len(verts),
                                           faces.ctypes.data_as(u32p) if faces is not None else None, n_faces, float(cell_size),
                                           remap.ctypes.data_as(u32p), capi.as_f32p(out_verts),
                                           capi.as_u8p(out_rgb) if out_rgb is not None else None, counts.ctypes.data_as(u32p), C.byref(m),
                                           out_faces.ctypes.data_as(u32p), C.byref(k)), "mesh_decimate")
    m, k = int(m.value), int(k.value)
    return {"vertices": out_verts[:m].copy(), "polygons": out_faces[:k].astype(np.int32), "rgb": out_rgb[:m].copy() if out_rgb is not None else None,
            "remap": remap, "counts": counts[:m].copy()}


def smooth_mesh(vertices, polygons, lam=0.5, mu=-0.53, iterations=10, keep_boundary=True, device=0):
    """Taubin's lambda | mu smoothing of an indexed mesh on the GPU (tsdf_hip_mesh_smooth; include/tsdf_hip.h states the
    rules): `iterations` times a step with `lam` and, iff mu != 0, a step with `mu`, over the neighbours the faces define.
    vertices (n, 3) float32; polygons (k, 3) vertex indices -- required: a triangle soup shares no vertices, flatten or
    decimate it first.  Returns dict(vertices (n, 3) float32, fixed (n,) uint8: 1 = not finite or next to such a vertex, 2 = in
    no face, 4 = on a boundary edge with keep_boundary, degree (n,) uint32: neighbours of each vertex)."""
    if polygons is None:
        raise ValueError("smooth_mesh: polygons are required (a triangle soup shares no vertices: flatten or decimate first)")
    verts = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    out = np.zeros_like(verts)
    fixed = np.zeros(len(verts), dtype=np.uint8)
    degree = np.zeros(len(verts), dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    capi.check(
        capi.load().tsdf_hip_mesh_smooth(int(device), capi.as_f32p(verts), len(verts), faces.ctypes.data_as(u32p), len(faces), float(lam), float(mu),
                                         int(iterations), 1 if keep_boundary else 0, capi.as_f32p(out), capi.as_u8p(fixed),
                                         degree.ctypes.data_as(u32p)), "mesh_smooth")
    return {"vertices": out, "fixed": fixed, "degree": degree}


def mesh_normals(vertices, polygons=None, device=0):
    """Area-weighted vertex normals of a triangle mesh on the GPU (tsdf_hip_mesh_normals; include/tsdf_hip.h states the rule):
    the fp64 sum of the face vectors (p_b - p_a) x (p_c - p_a) of the faces that name a vertex, in ascending face index,
    normalised -- pointing to the side from which a face's corners appear counter-clockwise.  vertices (n, 3) float32;
    polygons (k, 3) vertex indices, or None for a triangle soup (face f = vertices 3f, 3f+1, 3f+2).  Returns dict(normals
    (n, 3) float32, flags (n,) uint8: 1 = in no face, 2 = the normal is zero, 4 = a face of the vertex has a coordinate that
    is not finite and was skipped)."""
    verts = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = None if polygons is None else np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    if faces is None and len(verts) % 3:
        raise ValueError("mesh_normals: a triangle soup needs 3 vertices per face")
    n_faces = len(verts) // 3 if faces is None else len(faces)
    normals = np.zeros((len(verts), 3), dtype=np.float32)
    flags = np.zeros(len(verts), dtype=np.uint8)
    # (an array without elements may have no address: an indexed mesh without faces is not a soup)
    fp = None if faces is None else (faces if len(faces) else np.zeros((1, 3), np.uint32)).ctypes.data_as(C.POINTER(C.c_uint32))
    capi.check(capi.load().tsdf_hip_mesh_normals(int(device), capi.as_f32p(verts), len(verts), fp, n_faces, capi.as_f32p(normals), capi.as_u8p(flags)),
               "mesh_normals")
    return {"normals": normals, "flags": flags}


def reference_cull_planes(p, trans):
    """The six planes (l, r, t, b, far, near; 4 float32 each) pcl::FrustumCulling::applyFilter builds for the reference's
    getFrustumCulledVoxels (tsdf_volume_octree.cpp:633-646) from the forward pose `trans`: host-side Eigen / PCL
    arithmetic restated, like eigen_affine_inverse -- here by the library's own helper
    (tsdf_hip_reference_cull_planes), since Python has no Eigen to do it with."""
    tr = np.ascontiguousarray(np.asarray(trans, dtype=np.float64).reshape(4, 4))
    planes = np.empty(24, np.float32)
    capi.check(capi.load().tsdf_hip_reference_cull_planes(C.byref(p), tr.ctypes.data_as(C.POINTER(C.c_double)), capi.as_f32p(planes)),
               "reference_cull_planes")
    return planes


def transform_points_f64(xyz, m):
    """pcl::transformPointCloud with an Affine3d on float points [PCL-recall]: evaluated in double,
    x*c0 + (y*c1 + (z*c2 + c3)), rounded to float."""
    p = xyz.astype(np.float64)
    out = np.empty_like(p)
    for r in range(3):
        out[..., r] = p[..., 0] * m[r, 0] + (p[..., 1] * m[r, 1] + (p[..., 2] * m[r, 2] + m[r, 3]))
    return out.astype(np.float32)


def transform_cloud_with_normals(cloud, m):
    """pcl::transformPointCloudWithNormals (tsdf_volume_octree.cpp:422) on an (..., 8) array; with
    is_dense=false non-finite points are left untouched [PCL-recall]."""
    out = cloud.copy()
    xyz, nrm = cloud[..., 0:3], cloud[..., 3:6]
    fin = np.isfinite(xyz).all(-1)
    out[..., 0:3] = np.where(fin[..., None], transform_points_f64(xyz, m), xyz)
    p = nrm.astype(np.float64)
    rn = np.empty_like(p)
    for r in range(3):
        rn[..., r] = p[..., 0] * m[r, 0] + (p[..., 1] * m[r, 1] + p[..., 2] * m[r, 2])
    out[..., 3:6] = np.where(fin[..., None], rn.astype(np.float32), nrm)
    return out
