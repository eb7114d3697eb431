"""Harness over libbrmi.so: owns the HBM resources a render graph would own and drives the pass.

PyTorch is plumbing here (device memory, streams, torch.distributed); every kernel is in
libbrmi.so behind the C ABI of include/brmi.h.  There is no CPU fallback: if the HIP library is
missing or no GPU is present this module raises.
"""
import ctypes as C

import numpy as np

from . import capi


class BrmiError(RuntimeError):
    pass


def detile(flat, width, height, tile=8):
    """Tiled 8x8 storage, column-major inside a tile (numpy, leading dim = padded pixels) -> linear [H, W, ...]."""
    tx, ty = (width + tile - 1) // tile, (height + tile - 1) // tile
    rest = flat.shape[1:]
    a = flat.reshape((ty, tx, tile, tile) + rest)            # [tileY, tileX, xInTile, yInTile]
    a = np.transpose(a, (0, 3, 1, 2) + tuple(range(4, 4 + len(rest)))).reshape((ty * tile, tx * tile) + rest)
    return np.ascontiguousarray(a[:height, :width])


def tile(img, tile=8):
    """Linear [H, W, ...] -> tiled 8x8 storage (column-major inside a tile), padded to whole tiles; inverse of detile."""
    height, width = img.shape[:2]
    tx, ty = (width + tile - 1) // tile, (height + tile - 1) // tile
    rest = img.shape[2:]
    pad = np.zeros((ty * tile, tx * tile) + rest, dtype=img.dtype)
    pad[:height, :width] = img
    a = pad.reshape((ty, tile, tx, tile) + rest)                      # [tileY, yInTile, tileX, xInTile]
    a = np.transpose(a, (0, 2, 3, 1) + tuple(range(4, 4 + len(rest))))
    return np.ascontiguousarray(a).reshape((ty * tx * tile * tile,) + rest)


class VisibilityRenderer:
    """One brmi_pass (= CLodExtension + VisUtil + light clustering + deferred shading of one view)."""

    def __init__(self, scene, device="cuda:0", max_clusters=None, occlusion=False, stats=False, band=(0, 0), stripes=None, **cfg_over):
        """stripes = (rows, count, index): the interleaved screen partition (brmi_config::stripe*): this pass owns the chunks of `rows` rows
        with index = `index` (mod `count`) of the scene's frame and renders them into compact surfaces of height / count rows; read-backs
        return those compact images, `frame_rows()` says which rows of the frame they are."""
        import torch
        if not torch.cuda.is_available():
            raise BrmiError("no GPU: libbrmi.so needs an MI355X (there is no CPU fallback)")
        self.torch = torch
        self.lib = capi.brmi_lib()
        self.scene, self.device = scene, torch.device(device)
        torch.cuda.set_device(self.device)
        self.W, self.H = scene.width, scene.height
        self.stripes = stripes
        if stripes is not None:
            rows, count, index = stripes
            if scene.height % (rows * count):
                raise ValueError(f"{scene.height} rows do not split into chunks of {rows} rows for {count} GPUs")
            self.H = scene.height // count          # the compact surfaces
        cfg = capi.Config()
        self.lib.brmi_default_config(C.byref(cfg), self.W, self.H)
        if stripes is not None:
            cfg.stripeRows, cfg.stripeCount, cfg.stripeIndex, cfg.fullHeight = stripes[0], stripes[1], stripes[2], scene.height
        est = max(4096, scene.stats.get("instancedMeshlets") or 2 * scene.stats["meshletsTotal"] * max(1, scene.stats["instances"]) // max(1, scene.stats["meshes"]))      # every (instance, meshlet) pair: nothing more can be visible
        cfg.maxVisibleClusters = int(max_clusters or min(1 << 24, max(1 << 16, est)))
        cfg.maxTraversalRecords = cfg.maxVisibleClusters
        cfg.enableOcclusionCulling = 1 if occlusion else 0
        cfg.collectPassStatistics = 1 if stats else 0
        cfg.bandY0, cfg.bandY1 = band
        for k, v in cfg_over.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self._h = capi.vp()
        self._check(self.lib.brmi_create(C.byref(cfg), C.byref(self._h)), "brmi_create", use_pass=False)
        self.sb, self._scene_keep = scene.device_buffers(self.device)
        self.device_arrays = dict(scene.device_arrays)      # this pass's own copies (two passes in flight each have their camera buffers)
        if getattr(scene, "pending_chains", None):
            self.build_texture_chains()
        self._check(self.lib.brmi_set_scene(self._h, C.byref(self.sb)), "brmi_set_scene")
        self._anisotropy = None      # set_anisotropy's table
        self._environment, self._environment_index = None, 0      # set_environment's device tables, perFrame.activeEnvironmentIndex of this pass's frames
        self._debug_mode, self._debug_view, self._pf_own = 0, None, None      # set_debug_view: outputType, the targets, this pass's per-frame record
        self._frame_index = 0        # of the last brmi_update
        self._temporal = None        # set_temporal's history images and jitter state
        self.descs = {}

        def cb(_user, d):
            d = d.contents
            self.descs[d.id] = dict(name=d.name.decode(), bytes=d.bytes, width=d.width, height=d.height, bpp=d.bytesPerPixel)

        self._cb = capi.DECLARE_CB(cb)
        self._check(self.lib.brmi_declare(self._h, self._cb, None), "brmi_declare")
        self.res = {}
        binds = (capi.ResourceBinding * len(self.descs))()
        for i, (rid, d) in enumerate(sorted(self.descs.items())):
            t = torch.zeros(max(16, int(d["bytes"])), dtype=torch.uint8, device=self.device)
            self.res[rid] = t
            binds[i].id, binds[i].ptr, binds[i].bytes = rid, t.data_ptr(), t.numel()
        self.stream = torch.cuda.current_stream(self.device)
        self._binds = binds
        self._shadows = None         # set_shadows' maps, index tables and light-view passes
        self._check(self.lib.brmi_setup(self._h, binds, len(self.descs), self._s()), "brmi_setup")
        self.update()

    # ------------------------------------------------------------------------------------------
    def _s(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def texels(self):
        """The device tensor of the scene's texel array (every texture's packed chain), or None for a scene without textures."""
        return self.device_arrays.get("texels")

    def build_texture_chains(self):
        """Levels 1.. of every texture in scene.pending_chains, built in this pass's texel buffer by brmi_texmips_build / brmi_texmips_build_alpha
        (DESIGN.md 4.13), and copied back into scene.arrays["texels"]: the host arrays (what the CPU oracle reads, what a later pass uploads) then hold
        the chains the device built, and the list is emptied."""
        torch, scene = self.torch, self.scene
        texels = self.texels()
        descs = scene.arrays["textureDescs"].view(np.uint8).reshape(-1, 96)
        table = self.device_arrays["srgbToLinear"]
        scratch = torch.zeros(4, dtype=torch.uint8, device=self.device)
        keep = []
        for index, alpha in scene.pending_chains:
            d = capi.TextureDesc.from_buffer_copy(descs[index].tobytes())
            d.texels = texels.data_ptr() + int(descs[index, :8].view(np.uint64)[0])
            if alpha:
                stats = torch.zeros(d.mipCount * 260, dtype=torch.int32, device=self.device)
                scales = torch.zeros(d.mipCount, dtype=torch.float32, device=self.device)
                keep += [stats, scales]
                rc = self.lib.brmi_texmips_build_alpha(C.byref(d), table.data_ptr(), stats.data_ptr(), scales.data_ptr(), self._s())
            else:
                rc = self.lib.brmi_texmips_build(C.byref(d), table.data_ptr(), scratch.data_ptr(), 4, self._s())
            if rc != 0:
                raise BrmiError(f"texture {index}: mip chain build failed ({rc}): {self.lib.brmi_last_error(None).decode()}")
        torch.cuda.synchronize(self.device)
        scene.arrays["texels"] = texels.cpu().numpy().view(scene.arrays["texels"].dtype).reshape(scene.arrays["texels"].shape)
        scene.pending_chains = []

    def _check(self, rc, what, use_pass=True):
        if rc != 0:
            msg = self.lib.brmi_last_error(self._h).decode() if use_pass and self._h else ""
            raise BrmiError(f"{what} failed ({rc}): {msg}")

    def frame_rows(self):
        """Row of the scene's frame behind every row of this pass's surfaces (the identity without `stripes`)."""
        if self.stripes is None:
            return np.arange(self.H)
        from . import compose
        rows, count, index = self.stripes
        return compose.stripe_frame_rows(index, count, self.scene.height, rows)

    def set_camera_from(self, other, frame_index=0):
        """Next frame's camera: copy `other`'s camera / culling-camera buffers (same geometry, another camera step) into
        the device buffers the pass reads -- what the reference's CameraManager does between frames -- then brmi_update."""
        for name in ("cameras", "cullingCameras"):
            self.device_arrays[name].copy_(self.torch.from_numpy(other.arrays[name]).to(self.device))
        self._cam_scene = other
        self._cam_bytes = None
        self.update(frame_index)

    def set_camera_device(self, cameras_dev, culling_cameras_dev, cameras_host, frame_index=0):
        """Next frame's camera from buffers already in HBM (uint8 tensors with the bytes of Scene.camera_at): two device-to-device copies on the
        current stream into this pass's camera buffers, then brmi_update with the host copy of the same camera."""
        if self._temporal is not None:
            raise BrmiError("set_camera_device: not with a temporal binding (the jitter is applied to host camera bytes: set_camera_from)")
        self.device_arrays["cameras"].copy_(cameras_dev, non_blocking=True)
        self.device_arrays["cullingCameras"].copy_(culling_cameras_dev, non_blocking=True)
        upd = capi.FrameUpdate(cameras_host.ctypes.data, self._per_frame_host(self.scene).ctypes.data, frame_index)
        self._check(self.lib.brmi_update(self._h, C.byref(upd), self._s()), "brmi_update")
        self._frame_index = frame_index
        self._cam_bytes = cameras_host      # update() of a later frame repeats this camera

    def set_band(self, y0, y1):
        """Rows [y0, y1) this pass renders from its next frame on (brmi_set_band; passes created with dynamicBand=1).  update() before the frame, as always."""
        self._check(self.lib.brmi_set_band(self._h, capi.u32(int(y0)), capi.u32(int(y1))), "brmi_set_band")
        self.band = (int(y0), int(y1))

    def _per_frame_host(self, src):
        """The scene's per-frame record; with a debug view set, this pass's own copy of it with perFrame.outputType filled in (scenes are shared)."""
        pf = src.per_frame_host()
        mode = self._debug_mode
        if not mode and not self._environment_index:
            return pf
        self._pf_own = np.array(pf, copy=True)
        self._pf_own.view(np.uint32)[capi.PER_FRAME_OUTPUT_TYPE_WORD] = mode
        self._pf_own.view(np.uint32)[capi.PER_FRAME_ACTIVE_ENVIRONMENT_WORD] = self._environment_index
        return self._pf_own

    def _upload_cameras(self, cam, cull):
        for name, a in (("cameras", cam), ("cullingCameras", cull)):
            self.device_arrays[name][: len(a)].copy_(self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device))

    def _jittered_camera(self, src, frame_index):
        """set_temporal: the camera of `src` jittered by frame_index, uploaded to this pass's camera buffers; the host copy of it."""
        from . import temporal as tmod
        t = self._temporal
        if t["current"] is not None and t["current_index"] != frame_index:      # (an update() repeated for one frame keeps that frame's predecessor)
            t["previous"] = t["current"]
        cam, cull = tmod.jitter_camera(src.arrays["cameras"], src.arrays["cullingCameras"], self.W, self.H, tmod.jitter_offset(frame_index, t["phases"]), previous=t["previous"])
        t["current"], t["current_index"] = cam, frame_index
        self._upload_cameras(cam, cull)
        return cam

    def update(self, frame_index=0):
        self._frame_index = frame_index
        if getattr(self, "_cam_bytes", None) is not None:
            upd = capi.FrameUpdate(self._cam_bytes.ctypes.data, self._per_frame_host(self.scene).ctypes.data, frame_index)
            self._check(self.lib.brmi_update(self._h, C.byref(upd), self._s()), "brmi_update")
            return
        src = getattr(self, "_cam_scene", self.scene)
        cam, pf = src.camera_host(), self._per_frame_host(src)
        if self._temporal is not None:
            cam = self._jittered_camera(src, frame_index)
        upd = capi.FrameUpdate(cam.ctypes.data, pf.ctypes.data, frame_index)
        self._check(self.lib.brmi_update(self._h, C.byref(upd), self._s()), "brmi_update")

    def execute(self, shading_stream=None):
        """The whole frame on the current stream; with `shading_stream` (a torch stream) the resolve + shading half goes there."""
        if shading_stream is None:
            self._check(self.lib.brmi_execute(self._h, self._s()), "brmi_execute")
        else:
            self._check(self.lib.brmi_execute_split(self._h, self._s(), C.c_void_p(shading_stream.cuda_stream)), "brmi_execute_split")
        err, self._slab_error = getattr(self, "_slab_error", None), None
        if err is not None:
            raise BrmiError(f"the shade-slab hook raised during execute: {err!r}") from err

    def stage(self, name, *args):
        fn = getattr(self.lib, "brmi_" + name)
        self._check(fn(self._h, *[capi.u32(a) for a in args], self._s()), "brmi_" + name)
        err, self._slab_error = getattr(self, "_slab_error", None), None
        if err is not None:
            raise BrmiError(f"the shade-slab hook raised during brmi_{name}: {err!r}") from err

    def counters(self):
        c = capi.Counters()
        self._check(self.lib.brmi_read_counters(self._h, C.byref(c), self._s()), "brmi_read_counters")
        return c

    def stage_times(self):
        ms = (capi.f32 * len(capi.STAGE_NAMES))()
        self._check(self.lib.brmi_stage_times(self._h, ms), "brmi_stage_times")
        return dict(zip(capi.STAGE_NAMES, [float(x) for x in ms]))

    def set_timed_stages(self, names=None):
        """Record HIP events only around the named stages (None = all)."""
        mask = 0xFFFFFFFF if names is None else sum(1 << capi.STAGE_NAMES.index(n) for n in names)
        self._check(self.lib.brmi_set_timed_stages(self._h, mask), "brmi_set_timed_stages")

    def algorithmic_bytes(self):
        per = (capi.u64 * len(capi.STAGE_NAMES))()
        total = capi.u64()
        self._check(self.lib.brmi_algorithmic_bytes(self._h, per, C.byref(total)), "brmi_algorithmic_bytes")
        return dict(zip(capi.STAGE_NAMES, [int(x) for x in per])), int(total.value)

    def held_clusters(self):
        """(held, late): indices into visible_clusters() of the last frame's phase-1 clusters the culling held back, and of those the late pass drew (brmi_debug_read_held)."""
        nh, nl = capi.u32(), capi.u32()
        self._check(self.lib.brmi_debug_read_held(self._h, None, 0, C.byref(nh), None, 0, C.byref(nl)), "brmi_debug_read_held")
        held, late = np.zeros(max(1, nh.value), dtype=np.uint32), np.zeros(max(1, nl.value), dtype=np.uint32)
        self._check(self.lib.brmi_debug_read_held(self._h, held.ctypes.data_as(C.POINTER(capi.u32)), len(held), C.byref(nh), late.ctypes.data_as(C.POINTER(capi.u32)), len(late), C.byref(nl)), "brmi_debug_read_held")
        return held[: nh.value], late[: nl.value]

    def draw_list(self):
        """(draw, held_boxes, box_count): the last frame's draw list (indices into visible_clusters(); the list's counter is checked against its capacity), the box-table
        index of every held record in held_clusters()'s order, and the size of that table (brmi_debug_read_draw_list)."""
        nd, nh, nb = capi.u32(), capi.u32(), capi.u32()
        self._check(self.lib.brmi_debug_read_draw_list(self._h, None, 0, C.byref(nd), None, 0, C.byref(nh), C.byref(nb)), "brmi_debug_read_draw_list")
        if nd.value > self.cfg.maxVisibleClusters or nh.value > self.cfg.maxVisibleClusters:
            raise BrmiError(f"draw list of {nd.value} / held list of {nh.value} entries in buffers of {self.cfg.maxVisibleClusters}")
        draw, boxes = np.zeros(max(1, nd.value), dtype=np.uint32), np.zeros(max(1, nh.value), dtype=np.uint32)
        self._check(self.lib.brmi_debug_read_draw_list(self._h, draw.ctypes.data_as(C.POINTER(capi.u32)), len(draw), C.byref(nd), boxes.ctypes.data_as(C.POINTER(capi.u32)), len(boxes), C.byref(nh), C.byref(nb)), "brmi_debug_read_draw_list")
        return draw[: nd.value], boxes[: nh.value], int(nb.value)

    def lean_clusters(self):
        """(1 if the last frame's phase-1 main launch was the lean rasteriser, clusters it left to the general launch, triangles queued for k_raster_emit, runs of
        them) -- brmi_debug_lean_clusters."""
        out = (capi.u32 * 4)()
        self._check(self.lib.brmi_debug_lean_clusters(self._h, out), "brmi_debug_lean_clusters")
        return tuple(int(v) for v in out)

    def raster_shape(self):
        """1 if the last frame's phase 1 launched the slim register shape of the opaque direct rasteriser, 0 for the general one (brmi_debug_raster_shape)."""
        out = capi.u32(0)
        self._check(self.lib.brmi_debug_raster_shape(self._h, C.byref(out)), "brmi_debug_raster_shape")
        return int(out.value)

    def wide_triangles(self):
        """(phase-1 draw pass, late pass, phase 2) counts of the last frame's triangles queued for the workgroup-wide record emission (brmi_debug_wide_triangles)."""
        out = (capi.u32 * 3)()
        self._check(self.lib.brmi_debug_wide_triangles(self._h, out), "brmi_debug_wide_triangles")
        return tuple(int(x) for x in out)

    def algorithmic_bytes_launched(self):
        """The same for the kernel variants the frame launched (brmi_algorithmic_bytes_launched)."""
        per = (capi.u64 * len(capi.STAGE_NAMES))()
        total = capi.u64()
        self._check(self.lib.brmi_algorithmic_bytes_launched(self._h, per, C.byref(total)), "brmi_algorithmic_bytes_launched")
        return dict(zip(capi.STAGE_NAMES, [int(x) for x in per])), int(total.value)

    # -- read-back (linear layout) ---------------------------------------------------------------
    def _img(self, rid, dtype, comps=1):
        self.torch.cuda.synchronize(self.device)
        raw = self.res[capi.RES[rid]].cpu().numpy()
        a = raw.view(dtype)
        n = a.size // comps
        a = a.reshape((n, comps)) if comps > 1 else a.reshape((n,))
        return detile(a, self.W, self.H)

    def visibility(self):
        return self._img("VISIBILITY", np.uint64)

    def depth(self):
        return self._img("LINEAR_DEPTH", np.float32)

    def hdr(self):
        return self._img("HDR_COLOR", np.uint64)

    def gbuffer(self):
        return dict(normals=self._img("GBUF_NORMALS", np.float32, 4), albedo=self._img("GBUF_ALBEDO", np.uint32),
                    coat=self._img("GBUF_COAT", np.uint64), emissive=self._img("GBUF_EMISSIVE", np.uint64),
                    fuzz=self._img("GBUF_FUZZ", np.uint64), mr=self._img("GBUF_METALLIC_ROUGHNESS", np.uint32),
                    motion=self._img("GBUF_MOTION_VECTORS", np.uint32))

    def visible_clusters(self):
        c = self.counters()
        n = c.visibleClusters + c.visibleClustersPhase2
        self.torch.cuda.synchronize(self.device)
        raw = self.res[capi.RES["VISIBLE_CLUSTERS"]][: n * 16].cpu().numpy()
        return raw.view(np.uint32).reshape(n, 4)

    def invalidate_hzb(self):
        self._check(self.lib.brmi_invalidate_hzb(self._h), "brmi_invalidate_hzb")

    def set_shade_slabs(self, slabs, callback=None):
        """brmi_set_shade_slabs: the deferred shading in `slabs` row slabs; `callback(row0, row1, stream_ptr)` is called on the host after each slab's
        launches (the hook for PeerBandComposer.submit_rows).  slabs <= 1 or no callback: one launch over the band."""
        if callback is None or slabs <= 1:
            self._slab_cb = None
            self._check(self.lib.brmi_set_shade_slabs(self._h, capi.u32(0), None, None), "brmi_set_shade_slabs")
            return
        proto = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)

        def trampoline(user, r0, r1, stream):
            # ctypes swallows an exception raised inside a callback (it only prints it): keep the first one and re-raise it when the call into the
            # library that ran the hook has returned (execute), so that a failed hand-over of a slab does not leave a half-composed frame unnoticed
            try:
                callback(int(r0), int(r1), stream)
            except BaseException as e:      # noqa: BLE001
                if self._slab_error is None:
                    self._slab_error = e
        self._slab_error = None
        self._slab_cb = proto(trampoline)      # kept alive with the pass
        self._check(self.lib.brmi_set_shade_slabs(self._h, capi.u32(slabs), C.cast(self._slab_cb, C.c_void_p), None), "brmi_set_shade_slabs")

    # -- residency-aware cut and streaming feedback (brmi_set_streaming) ---------------------------
    def group_count(self):
        return int(self.sb.lodGroupCount)

    def set_streaming(self, non_resident_groups, active_group_scan_count=None, request_capacity=1 << 16, touched_capacity=1 << 17):
        """The cut follows residency from the next frame on: `non_resident_groups` (indices into lodGroups, or a bool mask over them) are not resident, groups
        at or above `active_group_scan_count` (default: the group count) neither, and those are never requested.  None switches streaming off.  The buffers
        (residency bits, request and touched lists, counts, scratch) are this pass's own tensors; calling it again with the same capacities rewrites the
        residency bits in place on the current stream, so frames in flight keep the bits they were issued with."""
        torch = self.torch
        if non_resident_groups is None:
            self._check(self.lib.brmi_set_streaming(self._h, None), "brmi_set_streaming")
            self._streaming = None
            return
        groups = self.group_count()
        mask = np.zeros(((groups + 31) // 32) * 32, dtype=bool)
        nr = np.asarray(non_resident_groups)
        if nr.dtype == bool:
            mask[:groups] = nr
        elif nr.size:
            mask[nr.astype(np.int64)] = True
        words = np.packbits(mask.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
        words = np.ascontiguousarray(words if words.size else np.zeros(1, dtype=np.uint32))
        active = groups if active_group_scan_count is None else int(active_group_scan_count)
        st = getattr(self, "_streaming", None)
        if st is not None and st["caps"] == (int(request_capacity), int(touched_capacity)):
            st["bits"].copy_(torch.from_numpy(words.view(np.int32)), non_blocking=False)
        else:
            scratch_bytes = int(self.lib.brmi_streaming_scratch_bytes(groups))
            st = dict(caps=(int(request_capacity), int(touched_capacity)),
                      bits=torch.from_numpy(words.view(np.int32)).to(self.device),
                      requests=torch.zeros((max(1, int(request_capacity)), 4), dtype=torch.int32, device=self.device),
                      touched=torch.zeros(max(1, int(touched_capacity)), dtype=torch.int32, device=self.device),
                      counts=torch.zeros(2, dtype=torch.int32, device=self.device),
                      scratch=torch.zeros(scratch_bytes + 16, dtype=torch.uint8, device=self.device))
        b = capi.StreamingBuffers()
        b.structSize = C.sizeof(capi.StreamingBuffers)
        b.activeGroupScanCount = active
        b.nonResidentBits = st["bits"].data_ptr()
        b.loadRequests, b.requestCapacity = st["requests"].data_ptr(), int(request_capacity)
        b.touchedGroups, b.touchedCapacity = st["touched"].data_ptr(), int(touched_capacity)
        b.counts = st["counts"].data_ptr()
        b.scratch, b.scratchBytes = st["scratch"].data_ptr(), st["scratch"].numel()
        self._check(self.lib.brmi_set_streaming(self._h, C.byref(b)), "brmi_set_streaming")
        self._streaming = st

    def streaming_tensors(self):
        """The device tensors behind the feedback (requests [capacity, 4], touched [capacity], counts [2], int32): clone them on the frame's geometry stream
        to keep a frame's feedback while later frames are in flight."""
        st = self._streaming
        return st["requests"], st["touched"], st["counts"]

    @staticmethod
    def unpack_feedback(requests, touched, counts):
        counts = np.asarray(counts).view(np.uint32).reshape(2).copy()
        requests, touched = np.asarray(requests).view(np.uint32), np.asarray(touched).view(np.uint32)
        return requests[: min(int(counts[0]), len(requests))].copy(), touched[: min(int(counts[1]), len(touched))].copy(), counts

    def streaming_feedback(self):
        """(requests ndarray[n, 4] of {group, instance, mesh buffer, priority16 << 16 | view}, touched ndarray, counts) of the last frame; n and len(touched)
        are clamped to the capacities, counts = (requested groups, touched groups) are not.  Waits for the device."""
        if getattr(self, "_streaming", None) is None:
            raise BrmiError("streaming_feedback: set_streaming first")
        self.torch.cuda.synchronize(self.device)
        r, t, c = self.streaming_tensors()
        return self.unpack_feedback(r.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy())

    # -- anisotropic filtering (brmi_set_sampler_anisotropy) ---------------------------------------
    def set_anisotropy(self, values):
        """maxAnisotropy of the scene's samplers from the next frame on: an int for every sampler, a sequence with one entry per sampler, or None for
        off (the isotropic sampler, exactly the frames of a pass that never called this).  Values are clamped to [1, 16] by the sampler; 0 reads as 1.
        The table is this pass's own tensor; replacing or dropping one waits for the device first, since a frame still in flight (on whichever stream its
        G-buffer half runs) may be reading it."""
        if self._anisotropy is not None:
            self.torch.cuda.synchronize(self.device)
        if values is None:
            self._check(self.lib.brmi_set_sampler_anisotropy(self._h, None, capi.u32(0)), "brmi_set_sampler_anisotropy")
            self._anisotropy = None
            return
        count = int(self.sb.samplerCount)
        words = np.full(count, int(values), dtype=np.uint32) if np.isscalar(values) else np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
        if len(words) != count:
            raise BrmiError(f"set_anisotropy: {len(words)} values for the scene's {count} samplers")
        table = self.torch.from_numpy(np.concatenate([words, np.zeros(1, dtype=np.uint32)]).view(np.int32)).to(self.device)      # (never empty)
        self._check(self.lib.brmi_set_sampler_anisotropy(self._h, table.data_ptr(), capi.u32(count)), "brmi_set_sampler_anisotropy")
        self._anisotropy = table

    # -- image-based lighting (brmi_set_environment) ------------------------------------------------
    def environment_buffers(self, environments, specular=True, skybox=False):
        """(capi.EnvironmentBuffers, tensors to keep alive) for a list of environment.Environment: the tables uploaded to this pass's device.  An environment
        with a sky cube (Environment.cube16) brings it as a cubemap of its own behind the prefiltered ones."""
        from . import environment as envmod
        torch, keep = self.torch, []

        def up(a):
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(self.device)
            keep.append(t)
            return t.data_ptr()
        info, descs, _ = envmod.environment_tables(environments, up)
        b = capi.EnvironmentBuffers()
        # without the skybox switch the struct goes over as its first layout (the fields up to cubemapCount are where they were): a build of the library from
        # before the switch (BRMI_LIB_PATH, A/B runs) takes it too
        b.structSize, b.specularIBL = C.sizeof(capi.EnvironmentBuffers) if skybox else capi.ENVIRONMENT_BUFFERS_SIZE_V1, 1 if specular else 0
        b.environments, b.environmentCount = up(info), len(environments)
        b.cubemaps, b.cubemapCount = up(descs), len(descs) // 6
        b.skybox = 1 if skybox else 0
        return b, keep

    def set_environment(self, env, index=0, specular=True, skybox=False):
        """Image-based lighting from the next frame on: an environment.Environment or a list of them (perFrame.activeEnvironmentIndex = `index` picks the
        frame's), or None for off -- exactly the frames of a pass that never called this.  skybox=True: the frame's pixels without geometry show the
        environment's sky cube (brmi_skybox behind the shading stage); without it a frame launches what it always launched.  The tables are this pass's own tensors; replacing or dropping
        them waits for the device first (a frame in flight may be reading them).  Repeats the last update() with the index in this pass's per-frame record."""
        if self._environment is not None:
            self.torch.cuda.synchronize(self.device)
        if env is None:
            self._check(self.lib.brmi_set_environment(self._h, None), "brmi_set_environment")
            self._environment, self._environment_index = None, 0
        else:
            envs = list(env) if isinstance(env, (list, tuple)) else [env]
            b, keep = self.environment_buffers(envs, specular, skybox)
            self._check(self.lib.brmi_set_environment(self._h, None), "brmi_set_environment")
            self._environment_index = int(index)
            self.update(self._frame_index)      # the index first: the binding is refused while the last update names an entry the table lacks
            self._check(self.lib.brmi_set_environment(self._h, C.byref(b)), "brmi_set_environment")
            self._environment = dict(buffers=b, keep=keep)
        # the device record too (brmi_frame_update::perFrameHost is by contract the host copy of that buffer)
        pf = self.device_arrays["perFrame"]
        words = self.torch.from_numpy(np.array([self._environment_index], dtype=np.int32)).to(self.device)
        pf.view(self.torch.int32)[capi.PER_FRAME_ACTIVE_ENVIRONMENT_WORD: capi.PER_FRAME_ACTIVE_ENVIRONMENT_WORD + 1].copy_(words)
        self.update(self._frame_index)

    def set_environment_index(self, index):
        """perFrame.activeEnvironmentIndex of the frames from the next update() on (which this repeats); an index the bound table lacks makes it raise."""
        previous, self._environment_index = self._environment_index, int(index)
        try:
            self.update(self._frame_index)
        except BrmiError:
            self._environment_index = previous
            raise
        pf = self.device_arrays["perFrame"]
        words = self.torch.from_numpy(np.array([self._environment_index], dtype=np.int32)).to(self.device)
        pf.view(self.torch.int32)[capi.PER_FRAME_ACTIVE_ENVIRONMENT_WORD: capi.PER_FRAME_ACTIVE_ENVIRONMENT_WORD + 1].copy_(words)

    # -- XeGTAO ambient occlusion (brmi_set_gtao) ---------------------------------------------------
    def gtao_layout(self):
        """capi.GtaoLayout of this pass's frame: where the depth levels, the edges and the working terms lie in the scratch."""
        lay = capi.GtaoLayout()
        self._check(self.lib.brmi_gtao_get_layout(capi.u32(self.W), capi.u32(self.H), C.byref(lay)), "brmi_gtao_get_layout", use_pass=False)
        return lay

    def set_gtao(self, quality="high", radius=0.5, denoise=1, max_depth_lod=0, fill=0, guard=0):
        """Screen-space ambient occlusion from the next frame on: execute() runs the depth prefilter, the main pass and the denoiser between the G-buffer and
        the shading stage, and the environment term takes min(albedo.a, term / 255).  quality: "low" | "medium" | "high" | "ultra" (or 0..3), None for off --
        exactly the frames of a pass that never called this.  The scratch and the final term are this pass's own tensors (every byte `fill` to start with,
        `guard` more bytes behind each that the library is not told about: gtao_guards_intact()); replacing or dropping them waits for the device first."""
        torch = self.torch
        if getattr(self, "_gtao", None) is not None:
            torch.cuda.synchronize(self.device)
        if quality is None:
            self._check(self.lib.brmi_set_gtao(self._h, None), "brmi_set_gtao")
            self._gtao = None
            return
        lay = self.gtao_layout()
        b = capi.GtaoBuffers()
        b.structSize = C.sizeof(capi.GtaoBuffers)
        self.lib.brmi_gtao_default_settings(C.byref(b.settings))
        b.settings.qualityLevel = capi.GTAO_QUALITY[quality.lower()] if isinstance(quality, str) else int(quality)
        b.settings.radius, b.settings.denoisePasses, b.settings.maxDepthLod = float(radius), int(denoise), int(max_depth_lod)
        scratch = torch.full((int(lay.scratchBytes) + int(guard),), int(fill), dtype=torch.uint8, device=self.device)
        term = torch.full((int(lay.outputBytes) + int(guard),), int(fill), dtype=torch.uint8, device=self.device)
        b.scratch, b.scratchBytes, b.aoTerm, b.aoTermBytes = scratch.data_ptr(), int(lay.scratchBytes), term.data_ptr(), int(lay.outputBytes)
        self._check(self.lib.brmi_set_gtao(self._h, C.byref(b)), "brmi_set_gtao")
        self._gtao = dict(buffers=b, scratch=scratch, term=term, layout=lay, fill=int(fill))

    def gtao_guards_intact(self):
        """True while the guard bytes behind set_gtao's scratch and final term still hold their fill."""
        g = self._gtao
        self.torch.cuda.synchronize(self.device)
        return bool((g["scratch"][int(g["layout"].scratchBytes):] == g["fill"]).all()) and bool((g["term"][int(g["layout"].outputBytes):] == g["fill"]).all())

    def ao_term(self):
        """(H, W) uint8: XeGTAO's final visibility codes of the last frame (255 = unoccluded)."""
        if getattr(self, "_gtao", None) is None:
            raise BrmiError("ao_term: set_gtao first")
        self.torch.cuda.synchronize(self.device)
        return detile(self._gtao["term"][: int(self._gtao["layout"].outputBytes)].cpu().numpy(), self.W, self.H)

    # -- the display chain (brmi_set_display) -------------------------------------------------------
    def display_layout(self):
        """capi.DisplayLayout of this pass's frame: where the histogram, the adapted luminance, the LPM control block and the bloom levels lie in the scratch."""
        lay = capi.DisplayLayout()
        self._check(self.lib.brmi_display_get_layout(capi.u32(self.W), capi.u32(self.H), C.byref(lay)), "brmi_display_get_layout", use_pass=False)
        return lay

    def set_display(self, tonemap="lpm", bloom=True, auto_exposure=True, time_coefficient=1.0 / 60.0, fixed_luminance=0.18, fill=0, guard=0):
        """The displayed picture from the next frame on: execute() runs auto-exposure, the bloom pyramid and the tone mapper behind the lit frame, and ldr()
        returns RGBA8.  tonemap: "reinhard" | "neutral" | "aces" | "lpm" | "none" (or 0..4), None for off -- exactly the frames of a pass that never called
        this.  Calling it again with a binding in place only changes the settings (the frame's delta time as time_coefficient, say): the buffers, and the
        adapted luminance in them, stay.  The buffers are this pass's own tensors (every byte `fill` to start with except the histogram and the adapted
        luminance, which are zero; `guard` more bytes behind each that the library is not told about: display_guards_intact())."""
        torch = self.torch
        d = getattr(self, "_display", None)
        if tonemap is None:
            if d is not None:
                torch.cuda.synchronize(self.device)
            self._check(self.lib.brmi_set_display(self._h, None), "brmi_set_display")
            self._display = None
            return
        if d is None:
            lay = self.display_layout()
            d = dict(layout=lay, fill=int(fill),
                     scratch=torch.full((int(lay.scratchBytes) + int(guard),), int(fill), dtype=torch.uint8, device=self.device),
                     ldr=torch.full((int(lay.ldrBytes) + int(guard),), int(fill), dtype=torch.uint8, device=self.device),
                     blended=torch.full((int(lay.blendedHdrBytes) + int(guard),), int(fill), dtype=torch.uint8, device=self.device))
            d["scratch"][int(lay.histogramOffset): int(lay.histogramOffset) + 1024].zero_()
            d["scratch"][int(lay.adaptedLuminanceOffset): int(lay.adaptedLuminanceOffset) + 4].zero_()
        lay = d["layout"]
        b = capi.DisplayBuffers()
        b.structSize = C.sizeof(capi.DisplayBuffers)
        self.lib.brmi_display_default_settings(C.byref(b.settings))
        b.settings.tonemapType = capi.TONEMAP_TYPES[tonemap.lower()] if isinstance(tonemap, str) else int(tonemap)
        b.settings.bloom, b.settings.autoExposure = int(bool(bloom)), int(bool(auto_exposure))
        b.settings.timeCoefficient, b.settings.fixedAdaptedLuminance = float(time_coefficient), float(fixed_luminance)
        b.scratch, b.scratchBytes, b.ldr, b.ldrBytes = d["scratch"].data_ptr(), int(lay.scratchBytes), d["ldr"].data_ptr(), int(lay.ldrBytes)
        b.blendedHdr, b.blendedHdrBytes = d["blended"].data_ptr(), int(lay.blendedHdrBytes)
        self._check(self.lib.brmi_set_display(self._h, C.byref(b)), "brmi_set_display")
        d["buffers"], d["bloom"] = b, bool(bloom)
        self._display = d

    def _displayed(self, what):
        if getattr(self, "_display", None) is None:
            raise BrmiError(f"{what}: set_display first")
        self.torch.cuda.synchronize(self.device)
        return self._display

    def display_guards_intact(self):
        """True while the guard bytes behind set_display's three buffers still hold their fill."""
        d = self._displayed("display_guards_intact")
        lay = d["layout"]
        return all(bool((d[k][int(n):] == d["fill"]).all()) for k, n in (("scratch", lay.scratchBytes), ("ldr", lay.ldrBytes), ("blended", lay.blendedHdrBytes)))

    def ldr(self):
        """(H, W, 4) uint8: the last frame as the tone mapper stored it (R8G8B8A8_UNORM, alpha 255)."""
        d = self._displayed("ldr")
        return d["ldr"][: self.W * self.H * 4].cpu().numpy().reshape(self.H, self.W, 4)

    def blended_hdr(self):
        """(H, W) uint64: the lit frame with the bloom blended in (four halves a pixel), what the reference leaves in its upscaled HDR target.  Bloom only."""
        d = self._displayed("blended_hdr")
        if not d["bloom"]:
            raise BrmiError("blended_hdr: the display chain runs without bloom")
        return detile(d["blended"][: int(d["layout"].blendedHdrBytes)].cpu().numpy().view(np.uint64), self.W, self.H)

    def adapted_luminance(self):
        """The adapted luminance the last frame's average stage left: the only state the chain carries from frame to frame."""
        d = self._displayed("adapted_luminance")
        o = int(d["layout"].adaptedLuminanceOffset)
        return float(d["scratch"][o: o + 4].cpu().numpy().view(np.float32)[0])

    def reset_exposure(self):
        """Adaptation starts again from zero (and from an empty histogram), as on the first frame."""
        d = self._displayed("reset_exposure")
        lay = d["layout"]
        d["scratch"][int(lay.histogramOffset): int(lay.histogramOffset) + 1024].zero_()
        d["scratch"][int(lay.adaptedLuminanceOffset): int(lay.adaptedLuminanceOffset) + 4].zero_()

    # -- temporal anti-aliasing (brmi_set_temporal) -------------------------------------------------
    def temporal_layout(self):
        lay = capi.TemporalLayout()
        self._check(self.lib.brmi_temporal_get_layout(capi.u32(self.W), capi.u32(self.H), C.byref(lay)), "brmi_temporal_get_layout", use_pass=False)
        return lay

    def set_temporal(self, blend=0.1, phases=16, fill=0, guard=0):
        """Temporal anti-aliasing from the next frame on: update(frame_index) jitters this pass's camera by temporal.jitter_offset(frame_index, phases), execute()
        resolves the lit frame against last frame's resolved image behind the skybox, and the display chain reads resolved_hdr().  blend: the current frame's
        weight; None for off -- the camera bytes and the frames of a pass that never called this.  The two history images are this pass's own tensors (every
        byte `fill` to start with, `guard` more bytes behind each that the library is not told about: temporal_guard_intact()).  Binding again restarts the
        accumulation.  Repeats the last update()."""
        torch = self.torch
        if self._temporal is not None:
            torch.cuda.synchronize(self.device)
        if blend is None:
            self._check(self.lib.brmi_set_temporal(self._h, None), "brmi_set_temporal")
            had, self._temporal = self._temporal is not None, None
            if had and getattr(self, "_cam_bytes", None) is None:      # the camera as it was before the jitter
                src = getattr(self, "_cam_scene", self.scene)
                self._upload_cameras(src.arrays["cameras"], src.arrays["cullingCameras"])
                self.update(self._frame_index)
            return
        if getattr(self, "_cam_bytes", None) is not None:
            raise BrmiError("set_temporal: the pass's camera came from set_camera_device (the jitter is applied to host camera bytes: set_camera_from)")
        lay = self.temporal_layout()
        images = [torch.full((int(lay.historyBytes) + int(guard),), int(fill), dtype=torch.uint8, device=self.device) for _ in range(2)]
        b = capi.TemporalBuffers()
        b.structSize = C.sizeof(capi.TemporalBuffers)
        self.lib.brmi_temporal_default_settings(C.byref(b.settings))
        b.settings.blend, b.settings.phases = float(blend), int(phases)
        b.history[0], b.history[1], b.historyBytes = images[0].data_ptr(), images[1].data_ptr(), int(lay.historyBytes)
        self._check(self.lib.brmi_set_temporal(self._h, C.byref(b)), "brmi_set_temporal")
        self._temporal = dict(buffers=b, images=images, layout=lay, fill=int(fill), phases=int(phases), previous=None, current=None, current_index=None)
        self.update(self._frame_index)

    def _temporal_bound(self, what):
        if self._temporal is None:
            raise BrmiError(f"{what}: set_temporal first")
        self.torch.cuda.synchronize(self.device)
        return self._temporal

    def resolved_hdr(self):
        """(H, W) uint64: the last frame as the temporal resolve left it (four halves a pixel), detiled like hdr()."""
        t = self._temporal_bound("resolved_hdr")
        index = capi.u32(0)
        self._check(self.lib.brmi_temporal_state(self._h, C.byref(index), None), "brmi_temporal_state")
        return detile(t["images"][index.value][: int(t["layout"].historyBytes)].cpu().numpy().view(np.uint64), self.W, self.H)

    def temporal_reset(self):
        """The next frame's resolve has no history: it writes the current frame, as the first one did."""
        self._temporal_bound("temporal_reset")
        self._check(self.lib.brmi_temporal_reset(self._h), "brmi_temporal_reset")

    def temporal_guard_intact(self):
        """True while the guard bytes behind set_temporal's two history images still hold their fill."""
        t = self._temporal_bound("temporal_guard_intact")
        return all(bool((img[int(t["layout"].historyBytes):] == t["fill"]).all()) for img in t["images"])

    # -- shadow maps of spot and point lights (brmi_set_shadows) ------------------------------------
    def set_shadows(self, lights, resolution=1024, point_resolution=512):
        """Shadows from the next frame on for `lights` (indices into the scene's light buffer; spot and point lights only), or None for off -- exactly the
        frames of a pass that never called this.  Builds one light camera per spot light and six 90 degree cameras per point light the way the reference's
        light manager does (shadows.light_views), appends them to this pass's camera buffer, fills the lights' shadowViewInfoIndex / shadowMapIndex /
        shadowSamplerIndex, allocates the R32F maps and owns one light-view pass per resolution.  The maps are rendered by render_shadow_maps(), not by execute()."""
        from . import shadows as sh
        torch = self.torch
        if lights is not None and getattr(self, "_streaming", None) is not None:
            raise BrmiError("set_shadows: call it before set_streaming (the grown camera buffer is a new scene binding, which forgets the streaming buffers)")
        if self._shadows is not None:
            torch.cuda.synchronize(self.device)
            self._check(self.lib.brmi_set_shadows(self._h, None), "brmi_set_shadows")
            for r in self._shadows["passes"].values():
                r.close()
            self._shadows = None
        rec = self.device_arrays["lights"].cpu().numpy().view(sh.LIGHT_DTYPE).copy()
        for k in ("shadowViewInfoIndex", "shadowMapIndex", "shadowSamplerIndex"):
            rec[k] = -1
        if lights is None:
            self.device_arrays["lights"].copy_(torch.from_numpy(rec.view(np.uint8)).to(self.device))
            self.update(self._frame_index)
            return
        main_count = getattr(self, "_main_camera_count", None) or int(self.sb.cameraCount)
        self._main_camera_count = main_count
        cams = [self.device_arrays["cameras"].cpu().numpy()[: main_count * sh.CAMERA_BYTES]]
        views, descs, spot_idx, point_idx, keep = [], [], [], [], []
        for li in lights:
            l = rec[int(li)]
            if int(l["type"]) not in (sh.LIGHT_POINT, sh.LIGHT_SPOT):
                raise BrmiError(f"set_shadows: light {li} is neither a spot nor a point light (directional shadows are not built)")
            spot = int(l["type"]) == sh.LIGHT_SPOT
            res = int(resolution if spot else point_resolution)
            l["shadowMapIndex"], l["shadowSamplerIndex"] = len(descs), 0
            l["shadowViewInfoIndex"] = len(spot_idx) if spot else len(point_idx) // 6
            for cam, cull in sh.light_views(l, res):
                index = main_count + len(views)
                (spot_idx if spot else point_idx).append(index)
                t = torch.zeros((res, res), dtype=torch.float32, device=self.device)
                d = capi.TextureDesc()
                d.texels, d.width, d.height, d.mipCount, d.format = t.data_ptr(), res, res, 1, capi.TEXTURE_FORMAT_R32_FLOAT
                views.append(dict(light=int(li), camera=cam, culling=cull, res=res, map=t, desc=d, near=float(l["nearPlane"]), far=float(l["farPlane"])))
                descs.append(d)
                cams.append(cam)

        def up(a):
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.device)
            keep.append(t)
            return t
        # the grown camera buffer is a new scene binding: brmi_set_scene and brmi_setup again with the resources this pass already owns
        camera_t = up(np.concatenate(cams))
        self.device_arrays["cameras"] = camera_t
        self.device_arrays["lights"].copy_(torch.from_numpy(rec.view(np.uint8)).to(self.device))
        self.sb.cameras, self.sb.cameraCount = camera_t.data_ptr(), main_count + len(views)
        torch.cuda.synchronize(self.device)
        self._check(self.lib.brmi_set_scene(self._h, C.byref(self.sb)), "brmi_set_scene")
        self._check(self.lib.brmi_setup(self._h, self._binds, len(self.descs), self._s()), "brmi_setup")
        if self._anisotropy is not None:      # brmi_set_scene forgets the per-sampler table; the samplers are the ones they were
            self._check(self.lib.brmi_set_sampler_anisotropy(self._h, self._anisotropy.data_ptr(), capi.u32(int(self.sb.samplerCount))), "brmi_set_sampler_anisotropy")
        b = capi.ShadowBuffers()
        b.structSize = C.sizeof(capi.ShadowBuffers)
        desc_bytes = b"".join(bytes(d) for d in descs) or bytes(96)
        b.maps, b.mapCount = up(np.frombuffer(desc_bytes, dtype=np.uint8)).data_ptr(), len(descs)
        b.spotCameraIndices, b.spotCount = up(np.array(spot_idx + [0], dtype=np.uint32)).data_ptr(), len(spot_idx)
        b.pointCameraIndices, b.pointCount = up(np.array(point_idx + [0], dtype=np.uint32)).data_ptr(), len(point_idx) // 6
        self.update(self._frame_index)
        self._check(self.lib.brmi_set_shadows(self._h, C.byref(b)), "brmi_set_shadows")
        self._shadows = dict(buffers=b, keep=keep, views=views, passes={}, lights=rec)

    def _light_pass(self, res):
        """This pass's light-view pass of `res` x `res` pixels: the scene's geometry (the device buffers are shared) behind one camera of its own."""
        sd = self._shadows
        if res not in sd["passes"]:
            v = next(v for v in sd["views"] if v["res"] == res)
            view_scene = self.scene.light_view(v["camera"], v["culling"], res, share=(self.sb, self.device_arrays))
            sd["passes"][res] = VisibilityRenderer(view_scene, device=self.device, max_clusters=int(self.cfg.maxVisibleClusters))
        return sd["passes"][res]

    def render_shadow_maps(self):
        """Renders every map of set_shadows: per view the camera, the geometry stages through their entry points (clear, cull, raster, depth copy), then
        brmi_shadow_capture.  execute() never does this: a static scene renders its maps once."""
        if self._shadows is None:
            raise BrmiError("render_shadow_maps: set_shadows first")
        for k in range(len(self._shadows["views"])):
            self.render_shadow_view(k)
        self.torch.cuda.synchronize(self.device)

    def render_shadow_view(self, index):
        """One map of set_shadows (descriptor order), issued on the current stream and not waited for."""
        torch, v = self.torch, self._shadows["views"][index]
        r = self._light_pass(v["res"])
        r.device_arrays["cameras"].copy_(torch.from_numpy(v["camera"]).to(self.device))
        r.device_arrays["cullingCameras"].copy_(torch.from_numpy(v["culling"]).to(self.device))
        r._cam_bytes = v["camera"]
        r.update(self._frame_index)
        r.stage("clear_visibility"); r.stage("cull", 1); r.stage("raster", 1); r.stage("depth_copy")
        r._check(self.lib.brmi_shadow_capture(r._h, capi.f32(v["near"]), capi.f32(v["far"]), C.byref(v["desc"]), r._s()), "brmi_shadow_capture")

    def shadow_maps(self):
        """The maps as (res, res) float32 arrays, in descriptor order (a point light's six faces +X -X +Y -Y +Z -Z in a row)."""
        if self._shadows is None:
            raise BrmiError("shadow_maps: set_shadows first")
        self.torch.cuda.synchronize(self.device)
        return [v["map"].cpu().numpy() for v in self._shadows["views"]]

    def debug_shadow(self, light, positions, normals):
        """brmi_debug_shadow: the shadow function of light `light` for made-up receivers ((n, 3) world positions and normals) -> (n,) float32 of 0 / 1."""
        torch = self.torch
        pos = torch.from_numpy(np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)).to(self.device)
        nrm = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)).to(self.device)
        out = torch.full((max(1, pos.shape[0]),), -1.0, dtype=torch.float32, device=self.device)
        self._check(self.lib.brmi_debug_shadow(self._h, capi.u32(int(light)), pos.data_ptr(), nrm.data_ptr(), out.data_ptr(), capi.u32(pos.shape[0]), self._s()), "brmi_debug_shadow")
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy()[: pos.shape[0]]

    # -- debug views (brmi_set_debug_view, perFrame.outputType) ------------------------------------
    def set_debug_view(self, mode, fill=0, check=True):
        """The debug view of the frames from the next update() on: a perFrame.outputType number or the reference's name without the OUTPUT_ prefix
        ("meshlets", "LIGHT_CLUSTER_LIGHT_COUNT", ...); None, 0 or "color" unbinds and gives the ordinary frames again.  Allocates the payload and the
        image target (this pass's own tensors), fills the payload with the sentinel and every byte of the image with `fill` (pixels without geometry
        keep it), and repeats the last update() -- same camera, same frame index -- with outputType in this pass's per-frame record.  A number the library
        has no view for is refused here; check=False lets it through to the library, whose next execute() refuses it before it launches anything."""
        torch = self.torch
        if isinstance(mode, str):
            key = mode.upper()
            key = key[len("OUTPUT_"):] if key.startswith("OUTPUT_") else key
            if key not in capi.OUTPUT_TYPES:
                raise BrmiError(f"set_debug_view: no debug view named {mode!r} (known: {', '.join(sorted(capi.OUTPUT_TYPES))})")
            mode = capi.OUTPUT_TYPES[key]
        mode = int(mode or 0)
        if check and mode not in capi.OUTPUT_TYPES.values():
            raise BrmiError(f"set_debug_view: outputType {mode} is not a debug view of this path (known: {', '.join(sorted(capi.OUTPUT_TYPES))})")
        if self._debug_view is not None:
            torch.cuda.synchronize(self.device)      # a frame in flight may still be writing the targets that are about to be dropped
        if mode == 0:
            self._check(self.lib.brmi_set_debug_view(self._h, None), "brmi_set_debug_view")
            self._debug_view = None
        else:
            payload = torch.full((int(self.lib.brmi_debug_view_bytes(self.W, self.H)) // 4,), -1, dtype=torch.int32, device=self.device)
            image = torch.full((self.H, self.W, 4), int(fill), dtype=torch.uint8, device=self.device)
            b = capi.DebugViewBuffers()
            b.structSize = C.sizeof(capi.DebugViewBuffers)
            b.payload, b.payloadBytes = payload.data_ptr(), payload.numel() * 4
            b.image, b.imageBytes = image.data_ptr(), image.numel()
            self._check(self.lib.brmi_set_debug_view(self._h, C.byref(b)), "brmi_set_debug_view")
            self._debug_view = dict(payload=payload, image=image)
        self._debug_mode = mode
        # the device record too: brmi_frame_update::perFrameHost is by contract the host copy of that buffer (the library picks the kernel from the host
        # copy, and its frame snapshot carries the device one along; no kernel reads the field today)
        pf = self.device_arrays["perFrame"]
        words = torch.from_numpy(np.array([mode], dtype=np.int32)).to(self.device)
        pf.view(torch.int32)[capi.PER_FRAME_OUTPUT_TYPE_WORD: capi.PER_FRAME_OUTPUT_TYPE_WORD + 1].copy_(words)
        self.update(self._frame_index)

    def debug_payload(self):
        """(H, W, 2) uint32: the last frame's debug payload, untiled; (0xFFFFFFFF, 0xFFFFFFFF) where there is no geometry."""
        if self._debug_view is None:
            raise BrmiError("debug_payload: set_debug_view first")
        self.torch.cuda.synchronize(self.device)
        return detile(self._debug_view["payload"].cpu().numpy().view(np.uint32).reshape(-1, 2), self.W, self.H)

    def debug_image(self):
        """(H, W, 4) uint8: the last frame's debug view as sRGB colour; pixels without geometry keep set_debug_view's fill."""
        if self._debug_view is None:
            raise BrmiError("debug_image: set_debug_view first")
        self.torch.cuda.synchronize(self.device)
        return self._debug_view["image"].cpu().numpy()

    def set_history_source(self, other):
        """Frames in flight: phase 1 tests against the depth chain `other` built for the frame before (None unlinks)."""
        self._check(self.lib.brmi_set_history_source(self._h, other._h if other is not None else None), "brmi_set_history_source")

    def hzb_mips(self):
        """Mips >= 1 of the linear-depth chain as row-major arrays (mip 0 is depth() padded to a power of two)."""
        self.torch.cuda.synchronize(self.device)
        raw = self.res[capi.RES["HZB"]].cpu().numpy().view(np.float32)
        pw, ph = 1 << (self.W - 1).bit_length(), 1 << (self.H - 1).bit_length()
        out, off, mip = [], 0, 1
        while pw > 1 or ph > 1:
            pw, ph = max(1, pw >> 1), max(1, ph >> 1)
            out.append(raw[off: off + pw * ph].reshape(ph, pw))
            off += pw * ph
            mip += 1
        return out

    def light_clusters(self):
        self.torch.cuda.synchronize(self.device)
        c = self.res[capi.RES["LIGHT_CLUSTERS"]].cpu().numpy().view(np.uint32)
        p = self.res[capi.RES["LIGHT_PAGES"]].cpu().numpy().view(np.uint32)
        return c[: (c.size // 12) * 12].reshape(-1, 12), p[: (p.size // 14) * 14].reshape(-1, 14)

    def hdr_tensor(self):
        """The tiled HDR target as a torch uint8 view (for RCCL composition)."""
        return self.res[capi.RES["HDR_COLOR"]]

    def close(self):
        if self._h:
            self.torch.cuda.synchronize(self.device)
            self.lib.brmi_destroy(self._h)
            self._h = None
            # every byte the pass used is caller-owned: drop the resource tensors and the uploaded scene with the pass
            self.res = {}
            self._debug_view = None
            self._environment = None
            self._gtao = None
            self._display = None
            self._temporal = None
            if getattr(self, "_shadows", None) is not None:
                for r in self._shadows["passes"].values():
                    r.close()
            self._shadows = None
            self._scene_keep = []
            self.device_arrays = {}
            if hasattr(self.scene, "device_arrays"):
                self.scene.device_arrays = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
