"""Renderer: the per-frame loop of the reference (display(), OpenglRayTracing/main.cpp:558-603)
driving the MI355X kernels through the C ABI (include/pt_abi.h).

    r = Renderer(1920, 1080, integrator="lambert")
    r.upload_scene(tris, nodes); r.upload_env(hdr)
    eye, rot = orbit_camera(0, 0, 4)
    for frame in range(n): r.render_frame(eye, rot, frame)
    img = r.accum()          # (h, w, 4) running mean, row 0 = bottom row (GL)

Nothing here has a CPU path: every call goes to libpt.so and raises if the
native library or the GPU is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native

INTEGRATORS = {
    "lambert": 0, "lambert_o": 0,           # OpenglRayTracing/shaders/pass1.fsh
    "disney": 1, "disney_uniform_d": 1,     # DisneyBRDF/shaders/pass1.fsh
    "mis": 2, "disney_mis_sobol_is": 2,     # ImportanceSampling_LowDiscrepancySequence/shaders/pass1.fsh
    "basic": 3, "basic_cpu_compat": 3,      # BasicRayTracingWithC++/main.cpp
}
FLAG_NO_CULL = 0x1
FLAG_CLOSEST_SHADOW = 0x2
FLAG_COUNT_FETCHES = 0x4
FLAG_WAVEFRONT = 0x8  # retired in round 5: pt_create rejects it (include/pt_abi.h)
FLAG_REGEN = 0x10
FLAG_NO_TILE_ORDER = 0x20
FLAG_REFERENCE_TREE = 0x40
FLAG_SERIAL_FRAMES = 0x80
FLAG_NO_BINS = 0x100
FLAG_HOST_ACCEL = 0x200
FLAG_MEGAKERNEL = 0x400
FLAG_PRIMARY_PASS = 0x800
FLAG_MOMENTS = 0x1000
FLAG_ADAPTIVE = 0x2000
FLAG_SHARE_MOMENTS = 0x4000
ENV_RGBE = 0x1  # pt_update_env's PT_ENV_RGBE (update_env(rgbe=True))
RADIANCE_RAYS_PER_SAMPLE = 0x1  # pt_radiance_mean's PT_RADIANCE_RAYS_PER_SAMPLE (radiance_mean(per_sample_rays=True))
PACK_STATS_F = 5 # f32 per packed slot of pack_owned_stats: r, g, b, m1, m2
GATHER = {"auto": 0, "copy": 1, "rccl": 2}


@dataclass
class FrameStats:
    rays: int
    node_fetch: int
    tri_fetch: int
    mat_fetch: int
    tex_fetch: int
    kernel_ms: float
    kernel_ms_total: float
    launches: int
    max_stack: int
    split_items: int
    runtime_tree: int
    waves_per_simd: int
    devices: int = 1
    gather: int = 0
    frames_in_flight: int = 1
    upload_ms: float = 0.0
    accel_build_ms: float = 0.0
    accel_device: int = -1
    accel_nodes: int = 0
    accel_depth: int = 0
    regen: int = 0
    frames: int = 0       # frames rendered (a batch launch renders several)
    frame_batch: int = 1  # most frames per launch
    env_compact: int = 0  # the env read from its compact (RGBE) texels (2: and the sample table by rows)
    tree4_nodes: int = 0  # 4-wide runtime-tree nodes


@dataclass
class AdaptiveStatus:
    tiles: int       # 8x8 tiles of the image (of a share_moments share: those it owns)
    retired: int     # of them retired
    frames: int      # moments_frames() at the last adaptive_update (0: none since the restart)
    max_err2: float  # the largest squared error over the tiles still active


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_native.c_float_p)


def device_count() -> int:
    n = C.c_int()
    _native.load().pt_device_count(C.byref(n))
    return n.value


class Renderer:
    def __init__(self, width: int, height: int, integrator="lambert", max_bounce: int = -1, device: int = 0,
                 tile_rank: int = 0, tile_world: int = 1, tile_size: int = 32, flags: int = 0,
                 basic_samples: int = 128, basic_seed: int = 0, sample_rank: int = 0, sample_world: int = 1,
                 devices=None, gather="auto", frame_batch: int = 0, moments: bool = False, adaptive: bool = False,
                 share_moments: bool = False):
        """share_moments: moments / adaptive on a screen-tile share (PT_FLAG_SHARE_MOMENTS, with tile_world > 1):
        the moments of the rank's own pixels, gathered with pack_owned_stats() / unpack_ranks_stats(), and
        adaptive_update() / adaptive_status() over the rank's own tiles (distributed.FrameGather(moments=True)
        gathers and combines them). adaptive: converged 8x8 tiles stop taking samples (PT_FLAG_ADAPTIVE: adaptive_update(),
        adaptive_status(), tile_error()); implies moments. moments: keep the per-pixel sample moments beside the running mean (PT_FLAG_MOMENTS:
        moments(), moments_frames(), and denoise_var()'s variance from them). devices: a list of HIP device ids (2..8, repeats allowed) makes this one context render
        screen tiles on all of them and gather them into the first device's accumulation every
        frame (pt_config.n_devices; gather "auto" / "copy" / "rccl"). frame_batch: most frames per
        launch of render_frames (0 = automatic: 2 x tile_world frames; tile_world on large Disney/MIS
        scenes)."""
        self._lib = _native.load()
        cfg = _native.PtConfig()
        cfg.width, cfg.height = int(width), int(height)
        cfg.integrator = INTEGRATORS[integrator] if isinstance(integrator, str) else int(integrator)
        cfg.max_bounce = int(max_bounce)
        cfg.device_id = int(device)
        cfg.tile_rank, cfg.tile_world, cfg.tile_size = int(tile_rank), int(tile_world), int(tile_size)
        cfg.flags = int(flags) | (FLAG_MOMENTS if moments or adaptive else 0) | (FLAG_ADAPTIVE if adaptive else 0) | \
            (FLAG_SHARE_MOMENTS if share_moments else 0)
        cfg.basic_samples = int(basic_samples)
        cfg.basic_seed = int(basic_seed) & 0xFFFFFFFF
        cfg.sample_rank, cfg.sample_world = int(sample_rank), int(sample_world)
        if devices is not None and len(devices) == 1:
            cfg.device_id = int(devices[0])
        if devices is not None and len(devices) > 1:
            cfg.n_devices = len(devices)
            for k, d in enumerate(devices):
                cfg.device_ids[k] = int(d)
            cfg.device_id = int(devices[0])
        cfg.gather = GATHER[gather] if isinstance(gather, str) else int(gather)
        cfg.frame_batch = int(frame_batch)
        from . import HW_QUEUES  # the queues GPU_MAX_HW_QUEUES granted this process (package import)
        cfg.hw_queues = int(HW_QUEUES)
        h = C.c_void_p()
        _native.check(self._lib.pt_create(C.byref(h), C.byref(cfg)), None, "pt_create")
        self._h = h
        self.width, self.height = cfg.width, cfg.height
        self.integrator = cfg.integrator
        self.device = cfg.device_id  # the GPU the context's buffers live on (a device group's first)
        self.tile_rank, self.tile_world = cfg.tile_rank, cfg.tile_world
        self.sample_rank, self.sample_world = cfg.sample_rank, cfg.sample_world

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pt_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc, what):
        _native.check(rc, self._h, what)

    def upload_scene(self, tris: np.ndarray, nodes: np.ndarray):
        t = np.ascontiguousarray(tris, np.float32).reshape(-1, 36)
        n = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
        self._ck(self._lib.pt_upload_scene(self._h, _fp(t), t.shape[0], _fp(n), n.shape[0]), "pt_upload_scene")
        self._n_nodes = n.shape[0]
        self._n_tris = t.shape[0]

    def update_geometry(self, verts):
        """New positions and shading normals for the uploaded triangles, in place (pt_update_geometry):
        verts is (n, 18) -- p1 p2 p3 n1 n2 n3 per triangle -- or (n, 36), a whole Triangle_encoded array
        whose materials are ignored; n the uploaded count, the uploaded order. The uploaded tree keeps its
        topology and gets exact boxes, the runtime's tree is rebuilt on the GPU: the context is then what
        upload_scene of the updated arrays would have made it. A numpy array is copied from the host; a
        torch tensor -- float32, contiguous, on the context's device, else ValueError -- is read in place
        in stream order on the context's stream (pt_update_geometry_device): hand the stream that
        produced it to set_stream, or synchronise. Returns when the scene is ready; restart the
        accumulation at frame_counter 0."""
        what = "update_geometry"
        host, v, (n, stride) = Renderer._update_source(what, "verts", verts, "(n, 18) or (n, 36)", 2, (18, 36))
        if host:
            self._ck(self._lib.pt_update_geometry(self._h, _fp(v), n, stride), "pt_update_geometry")
            return
        _, p, _ = self._query_args(what, n, [("verts", v, "float32", stride, True)])
        self._ck(self._lib.pt_update_geometry_device(self._h, p[0], n, stride), "pt_update_geometry_device")

    def update_materials(self, mats):
        """New materials for the uploaded triangles, in place (pt_update_materials): mats is (n, 18) --
        Triangle_encoded floats 18..35 per triangle -- or (n, 36), a whole Triangle_encoded array whose
        floats 0..17 are ignored; n the uploaded count, the uploaded order. The material table is rebuilt
        on the GPU and no tree is: the context is then what upload_scene of the records with the new
        materials would have made it. A numpy array is copied from the host; a torch tensor -- float32,
        contiguous, on the context's device, else ValueError -- is read in place in stream order on the
        context's stream (pt_update_materials_device): hand the stream that produced it to set_stream,
        or synchronise. Returns when the scene is ready; the guides are stale until the next
        render_guides; restart the accumulation at frame_counter 0."""
        what = "update_materials"
        host, m, (n, stride) = Renderer._update_source(what, "mats", mats, "(n, 18) or (n, 36)", 2, (18, 36))
        skip = 72 if stride == 36 else 0  # floats 18..35 of a whole record
        if host:
            self._ck(self._lib.pt_update_materials(self._h, C.cast(m.ctypes.data + skip, _native.c_float_p), n, stride),
                     "pt_update_materials")
            return
        self._query_args(what, n, [("mats", m, "float32", stride, True)])
        self._ck(self._lib.pt_update_materials_device(self._h, C.c_void_p(m.data_ptr() + skip), n, stride),
                 "pt_update_materials_device")

    def material_count(self) -> int:
        """The number of distinct materials of the scene (pt_material_count)."""
        n = C.c_int(0)
        self._ck(self._lib.pt_material_count(self._h, C.byref(n)), "pt_material_count")
        return n.value

    def materials(self):
        """Diagnostics (pt_download_materials) -> (table (material_count, 18) f32, ids (triangles,) i32):
        the distinct materials in the order of their first appearance, and every triangle's id."""
        table = np.empty((self.material_count(), 18), np.float32)
        ids = np.empty(getattr(self, "_n_tris", 0), np.int32)
        self._ck(self._lib.pt_download_materials(self._h, _fp(table), table.shape[0],
                                                 ids.ctypes.data_as(_native.c_int_p)), "pt_download_materials")
        return table, ids

    def node_boxes(self) -> np.ndarray:
        """Diagnostics (pt_download_node_boxes): the uploaded tree's current boxes, (nodes, 6) f32 -- lo,
        hi by node id of the last upload_scene; entries of unreachable nodes are unspecified."""
        out = np.empty((getattr(self, "_n_nodes", 0), 6), np.float32)
        self._ck(self._lib.pt_download_node_boxes(self._h, _fp(out)), "pt_download_node_boxes")
        return out

    def hdr_cache_device(self, hdr: np.ndarray) -> np.ndarray:
        """calculateHdrCache on this context's GPU, (h, w, 3) like scene.calculate_hdr_cache."""
        h = np.ascontiguousarray(hdr, np.float32)
        hh, ww = h.shape[:2]
        out = np.empty((hh, ww, 3), np.float32)
        self._ck(self._lib.pt_hdr_cache_device(self._h, _fp(h), ww, hh, _fp(out)), "pt_hdr_cache_device")
        return out

    def upload_env(self, hdr, cache=None):
        if hdr is None:
            self._ck(self._lib.pt_upload_env(self._h, None, 0, 0, None), "pt_upload_env")
            return
        h = np.ascontiguousarray(hdr, np.float32)
        hh, ww = h.shape[:2]
        c = None if cache is None else np.ascontiguousarray(cache, np.float32)
        self._ck(self._lib.pt_upload_env(self._h, _fp(h), ww, hh, None if c is None else _fp(c)), "pt_upload_env")

    def update_env(self, hdr, cache=None, rgbe: bool = False):
        """A new environment in place (pt_update_env): hdr is (h, w, 3) float32, cache the (h, w, 3) table of
        calculate_hdr_cache or None for the library's own, computed on the GPU; rgbe rounds every texel to
        the RGBE texel a Radiance file would hold first (PT_ENV_RGBE), so that a map computed in floats is
        kept in the compact forms. The context is then what upload_env of the same map would have made
        it, and an update of the same size as the last allocates nothing. A numpy array is copied from the
        host; a torch tensor -- float32, contiguous, on the context's device, shape (h, w, 3), else
        ValueError -- is read in place in stream order on the context's stream (pt_update_env_device):
        hand the stream that produced it to set_stream, or synchronise. None clears the environment.
        Returns when the environment is ready; restart the accumulation at frame_counter 0."""
        what = "update_env"
        flags = ENV_RGBE if rgbe else 0
        if hdr is None:
            self._ck(self._lib.pt_update_env(self._h, None, 0, 0, None, flags), "pt_update_env")
            return
        host, h, (hh, ww, _) = Renderer._update_source(what, "hdr", hdr, "(h, w, 3)", 3, (3,))
        if host:
            if cache is not None and hasattr(cache, "data_ptr"):
                raise ValueError(f"{what}: hdr is a host array, cache a tensor: pass both as one kind")
            c = None if cache is None else np.ascontiguousarray(cache, np.float32)
            if c is not None and c.shape != h.shape:
                raise ValueError(f"{what}: cache must be {h.shape} like hdr, not {c.shape}")
            self._ck(self._lib.pt_update_env(self._h, _fp(h), ww, hh, None if c is None else _fp(c), flags), "pt_update_env")
            return
        if cache is not None and (not hasattr(cache, "data_ptr") or tuple(cache.shape) != tuple(h.shape)):
            raise ValueError(f"{what}: cache must be a tensor of shape {tuple(h.shape)} like hdr")
        _, p, _ = self._query_args(what, hh * ww, [("hdr", h, "float32", 3, True), ("cache", cache, "float32", 3, False)])
        self._ck(self._lib.pt_update_env_device(self._h, p[0], ww, hh, p[1], flags), "pt_update_env_device")

    def env_size(self):
        """(w, h) of the environment, (0, 0) without one (pt_env_size)."""
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self._lib.pt_env_size(self._h, C.byref(w), C.byref(h)), "pt_env_size")
        return w.value, h.value

    def download_env(self, form: int = 0):
        """Diagnostics (pt_download_env) -> (texels (h, w, 4) f32: r g b pdf, table (h, w, 2) f32: x y) as the
        kernels read them: form 0 the float texels and table, form 1 the same decoded from the compact forms
        (env_compact >= 1), form 2 the table read through the row form (env_compact == 2; texels is None)."""
        w, h = self.env_size()
        texels = None if form == 2 else np.empty((h, w, 4), np.float32)
        table = np.empty((h, w, 2), np.float32)
        self._ck(self._lib.pt_download_env(self._h, int(form), None if texels is None else _fp(texels), _fp(table)),
                 "pt_download_env")
        return texels, table

    def upload_shapes(self, shapes: np.ndarray):
        """BASIC: n x 24 f64 shape records (scenes.cornell_shapes, include/pt_scene.h)."""
        s = np.ascontiguousarray(shapes, np.float64).reshape(-1, 24)
        self._ck(self._lib.pt_upload_shapes(self._h, s.ctypes.data_as(_native.c_double_p), s.shape[0]),
                 "pt_upload_shapes")

    def basic_image(self) -> np.ndarray:
        """BASIC: the reference's double image (h, w, 3), row 0 = top (BasicRayTracingWithC++/main.cpp:356)."""
        out = np.empty((self.height, self.width, 3), np.float64)
        self._ck(self._lib.pt_download_basic_image(self._h, out.ctypes.data_as(_native.c_double_p)),
                 "pt_download_basic_image")
        return out

    def set_basic_stream(self, stream, offsets):
        """BASIC: replay a recorded randf() stream; offsets (samples, h, w) = where each pixel sample's
        draws start. stream None returns to the per-pixel counter RNG. Returns nothing."""
        if stream is None:
            self._ck(self._lib.pt_set_basic_stream(self._h, None, 0, None, 0), "pt_set_basic_stream")
            return
        st = np.ascontiguousarray(stream, np.float64).reshape(-1)
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        self._keep_stream = (st, off)
        self._ck(self._lib.pt_set_basic_stream(self._h, st.ctypes.data_as(_native.c_double_p), st.size,
                                               off.ctypes.data_as(C.POINTER(C.c_int64)), off.size),
                 "pt_set_basic_stream")

    def set_basic_image(self, img: np.ndarray):
        """BASIC checkpoint restore: the double image (h, w, 3) as basic_image() returned it."""
        a = np.ascontiguousarray(img, np.float64).reshape(self.height, self.width, 3)
        self._ck(self._lib.pt_upload_basic_image(self._h, a.ctypes.data_as(_native.c_double_p)),
                 "pt_upload_basic_image")

    def basic_replay_overruns(self) -> int:
        c = C.c_int64()
        self._ck(self._lib.pt_basic_replay_overruns(self._h, C.byref(c)), "pt_basic_replay_overruns")
        return c.value

    def render_frame(self, eye, camera_rotate, frame_counter: int, download: bool = False, sync: bool = True):
        e = np.ascontiguousarray(eye, np.float32)
        r = np.ascontiguousarray(camera_rotate, np.float32).reshape(16)
        if not sync:
            self._ck(self._lib.pt_render_frame_async(self._h, _fp(e), _fp(r), int(frame_counter) & 0xFFFFFFFF),
                     "pt_render_frame_async")
            return None
        out = np.empty((self.height, self.width, 4), np.float32) if download else None
        self._ck(self._lib.pt_render_frame(self._h, _fp(e), _fp(r), int(frame_counter) & 0xFFFFFFFF,
                                           None if out is None else _fp(out)), "pt_render_frame")
        return out

    def render_frames(self, eye, camera_rotate, frame_counter: int, n: int):
        """n display() calls of one camera (frames frame_counter .. frame_counter + n - 1), rendered
        in batches (pt_render_frames_async; bit for bit n render_frame calls). Asynchronous."""
        e = np.ascontiguousarray(eye, np.float32)
        r = np.ascontiguousarray(camera_rotate, np.float32).reshape(16)
        self._ck(self._lib.pt_render_frames_async(self._h, _fp(e), _fp(r), int(frame_counter) & 0xFFFFFFFF, int(n)),
                 "pt_render_frames_async")

    def trace_closest(self, rays: np.ndarray):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = r.shape[0]
        t = np.empty(n, np.float32)
        tri = np.empty(n, np.int32)
        self._ck(self._lib.pt_trace_closest(self._h, _fp(r), n, _fp(t), tri.ctypes.data_as(_native.c_int_p)),
                 "pt_trace_closest")
        return t, tri

    @staticmethod
    def _rays_tmax(rays, tmax):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        b = None if tmax is None else np.ascontiguousarray(tmax, np.float32).reshape(-1)
        if b is not None and b.size != r.shape[0]:
            raise ValueError(f"tmax has {b.size} entries for {r.shape[0]} rays")
        return r, b

    def trace_closest_range(self, rays: np.ndarray, tmax=None):
        """trace_closest with a bound per ray (pt_trace_closest_range): (t, tri) of the closest hit with
        t < tmax[k], else the miss values (2147483648.0, -1); tmax None: no bound. Synchronous, and it
        does not wait for frames in flight."""
        r, b = self._rays_tmax(rays, tmax)
        n = r.shape[0]
        t = np.empty(n, np.float32)
        tri = np.empty(n, np.int32)
        self._ck(self._lib.pt_trace_closest_range(self._h, _fp(r), None if b is None else _fp(b), n, _fp(t),
                                                  tri.ctypes.data_as(_native.c_int_p)), "pt_trace_closest_range")
        return t, tri

    def trace_occluded(self, rays: np.ndarray, tmax=None) -> np.ndarray:
        """The occlusion test (pt_trace_occluded): uint8 per ray, 1 when it hits anything at t < tmax[k]
        (tmax None: anywhere), else 0. Synchronous."""
        r, b = self._rays_tmax(rays, tmax)
        n = r.shape[0]
        occ = np.empty(n, np.uint8)
        self._ck(self._lib.pt_trace_occluded(self._h, _fp(r), None if b is None else _fp(b), n,
                                             occ.ctypes.data_as(C.POINTER(C.c_uint8))), "pt_trace_occluded")
        return occ

    @staticmethod
    def _update_source(what, name, value, wanted, ndim, last):
        """The in-place updates' argument in either form -> (host, value, shape): a host array (anything
        without data_ptr, made a contiguous float32 numpy array; host True) or a device tensor (as given,
        for _query_args to check; host False), of ndim dimensions, the last one of `last` -- else
        ValueError naming the wanted shape."""
        host = isinstance(value, np.ndarray) or not hasattr(value, "data_ptr")
        if host:
            value = np.ascontiguousarray(value, np.float32)
        shape = tuple(int(k) for k in value.shape)
        if len(shape) != ndim or shape[-1] not in last:
            raise ValueError(f"{what}: {name} must be {wanted}, not {shape}")
        return host, value, shape

    def _query_args(self, what, n, specs):
        """The device queries' arguments: specs = [(name, value, dtype name, elements per ray, required)].
        Every value is a raw device pointer (an int; then n is required) or a torch tensor -- contiguous,
        on the context's device, of that dtype and size -- else ValueError. Returns (n, [pointers],
        torch module or None when only raw pointers came)."""
        torch = None
        tensors = [v for _, v, _, _, _ in specs if v is not None and not isinstance(v, (int, np.integer))]
        if tensors:
            import torch
        for name, v, dt, per, _ in specs:
            if v is None or isinstance(v, (int, np.integer)):
                continue
            if not torch.is_tensor(v):
                raise ValueError(f"{what}: {name} must be a device pointer (int) or a torch tensor, not {type(v).__name__}")
            if not v.is_cuda or v.device.index != self.device:
                raise ValueError(f"{what}: {name} is on {v.device}, the context renders on GPU {self.device}")
            if v.dtype != getattr(torch, dt):
                raise ValueError(f"{what}: {name} must be {dt}, not {v.dtype}")
            if not v.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous")
            if v.numel() % per:
                raise ValueError(f"{what}: {name} has {v.numel()} elements, not a multiple of {per}")
            if n is None and name == "rays":
                n = v.numel() // per
        if n is None:
            raise ValueError(f"{what}: n is required with raw device pointers")
        n = int(n)
        if n < 0:
            raise ValueError(f"{what}: n must be >= 0")
        ptrs = []
        for name, v, dt, per, required in specs:
            if v is None:
                if required and n > 0:
                    raise ValueError(f"{what}: {name} is required")
                ptrs.append(None)
            elif isinstance(v, (int, np.integer)):
                ptrs.append(C.c_void_p(int(v)))
            else:
                if v.numel() != n * per:
                    raise ValueError(f"{what}: {name} has {v.numel()} elements for {n} rays ({per} each)")
                ptrs.append(C.c_void_p(v.data_ptr()))
        return n, ptrs, torch

    def trace_closest_device(self, rays, tmax=None, out_t=None, out_tri=None, n=None):
        """trace_closest_range on device memory (pt_trace_closest_device): asynchronous, in stream order on
        the context's stream (set_stream), without a copy. rays (n x 6 float32), tmax (n float32 or None),
        out_t (n float32) and out_tri (n int32) are raw device pointers (ints, with n) or torch tensors --
        contiguous, on the context's device, of those dtypes: anything else raises ValueError. With tensor
        rays, outputs not given are allocated on the current torch stream's device. Returns (out_t, out_tri)
        as given or allocated. What produces the rays and what reads the results must be ordered with the
        context's stream: hand it the producing stream with set_stream, or synchronise."""
        what = "trace_closest_device"
        specs = [("rays", rays, "float32", 6, True), ("tmax", tmax, "float32", 1, False)]
        n, _, torch = self._query_args(what, n, specs)
        if torch is not None and torch.is_tensor(rays):
            if out_t is None:
                out_t = torch.empty(n, dtype=torch.float32, device=rays.device)
            if out_tri is None:
                out_tri = torch.empty(n, dtype=torch.int32, device=rays.device)
        specs += [("out_t", out_t, "float32", 1, True), ("out_tri", out_tri, "int32", 1, True)]
        n, p, _ = self._query_args(what, n, specs)
        self._ck(self._lib.pt_trace_closest_device(self._h, p[0], p[1], n, p[2], p[3]), "pt_trace_closest_device")
        return out_t, out_tri

    def trace_occluded_device(self, rays, tmax=None, out=None, n=None):
        """trace_occluded on device memory (pt_trace_occluded_device): as trace_closest_device, with one
        output of n uint8 (0 / 1). Returns out as given or allocated."""
        what = "trace_occluded_device"
        specs = [("rays", rays, "float32", 6, True), ("tmax", tmax, "float32", 1, False)]
        n, _, torch = self._query_args(what, n, specs)
        if out is None and torch is not None and torch.is_tensor(rays):
            out = torch.empty(n, dtype=torch.uint8, device=rays.device)
        specs += [("out", out, "uint8", 1, True)]
        n, p, _ = self._query_args(what, n, specs)
        self._ck(self._lib.pt_trace_occluded_device(self._h, p[0], p[1], n, p[2]), "pt_trace_occluded_device")
        return out

    def camera_rays_device(self, eye, camera_rotate, sample_index: int = 0, out_rays=None, out_ids=None):
        """The frame kernels' camera rays of sample sample_index, jitter included, for every pixel of this
        context's width x height (pt_camera_rays_device): ray py * width + px = (eye, direction), id =
        (px, py). out_rays (w*h x 6 float32) and out_ids (w*h x 2 int32) are torch tensors or raw device
        pointers as in trace_closest_device; not given, they are allocated as torch tensors on the context's
        device. Asynchronous on the context's stream. Returns (out_rays, out_ids)."""
        what = "camera_rays_device"
        n = self.width * self.height
        if out_rays is None or out_ids is None:
            import torch
            dev = f"cuda:{self.device}"
            if out_rays is None:
                out_rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
            if out_ids is None:
                out_ids = torch.empty((n, 2), dtype=torch.int32, device=dev)
        _, p, _ = self._query_args(what, n, [("out_rays", out_rays, "float32", 6, True),
                                             ("out_ids", out_ids, "int32", 2, True)])
        e = np.ascontiguousarray(eye, np.float32)
        r = np.ascontiguousarray(camera_rotate, np.float32).reshape(16)
        self._ck(self._lib.pt_camera_rays_device(self._h, _fp(e), _fp(r), int(sample_index) & 0xFFFFFFFF, p[0], p[1]),
                 "pt_camera_rays_device")
        return out_rays, out_ids

    def radiance_device(self, rays, ids=None, sample_index: int = 0, out=None, n=None):
        """One sample of this context's integrator along each ray, on device memory (pt_radiance_device):
        out[k] = (r, g, b, t) of ray k taken as the camera ray of pixel ids[k] = (px, py) of sample
        sample_index (ids None: (k & 4095, k >> 12)); a ray equal to a frame's camera ray yields that frame's
        sample bit for bit (include/pt_abi.h). rays (n x 6 float32), ids (n x 2 int32 or None) and out (n x 4
        float32) are torch tensors or raw device pointers (ints, with n) as in trace_closest_device; out not
        given is allocated with tensor rays. Asynchronous, in stream order on the context's stream. Returns out."""
        what = "radiance_device"
        specs = [("rays", rays, "float32", 6, True), ("ids", ids, "int32", 2, False)]
        n, _, torch = self._query_args(what, n, specs)
        if out is None and torch is not None and torch.is_tensor(rays):
            out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        specs += [("out", out, "float32", 4, True)]
        n, p, _ = self._query_args(what, n, specs)
        self._ck(self._lib.pt_radiance_device(self._h, p[0], p[1], n, int(sample_index) & 0xFFFFFFFF, p[2]),
                 "pt_radiance_device")
        return out

    def radiance(self, rays: np.ndarray, ids=None, sample_index: int = 0) -> np.ndarray:
        """radiance_device on host arrays (pt_radiance): (n, 4) f32 -- r, g, b, t. Synchronous."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = r.shape[0]
        i = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1, 2)
        if i is not None and i.shape[0] != n:
            raise ValueError(f"ids has {i.shape[0]} entries for {n} rays")
        out = np.empty((n, 4), np.float32)
        self._ck(self._lib.pt_radiance(self._h, _fp(r), None if i is None else i.ctypes.data_as(_native.c_int_p), n,
                                       int(sample_index) & 0xFFFFFFFF, _fp(out)), "pt_radiance")
        return out

    @staticmethod
    def _mean_samples(what, first_sample, n_samples):
        first_sample, n_samples = int(first_sample), int(n_samples)
        if n_samples < 1:
            raise ValueError(f"{what}: n_samples must be >= 1")
        if first_sample < 0 or first_sample + n_samples > 0xFFFFFFFF:
            raise ValueError(f"{what}: samples {first_sample} .. {first_sample + n_samples - 1} leave the 32-bit sample index")
        return first_sample, n_samples

    def radiance_mean_device(self, rays, ids=None, first_sample: int = 0, n_samples: int = 1, per_sample_rays: bool = False,
                             mean=None, moments=None, n=None):
        """n_samples samples of this context's integrator along each ray, folded on the GPU into a running
        mean (pt_radiance_mean_device): sample j is radiance_device's rgb for sample index first_sample + j,
        folded in sample order with the frames' weights 1 / (s + 1) and the frames' floats, so a picture goes
        on across calls as frames do across launches. first_sample 0 starts from zero (mean and moments are
        not read); otherwise they are read and must be given. mean[k] = (r, g, b, t of the last sample's ray).
        moments: None -- none kept; True -- allocated (first_sample 0 only); or given -- (n x 2 float32) the
        running means of the sample luminance and its square, a FLAG_MOMENTS context's plane.
        per_sample_rays: rays is (n_samples x n x 6), sample j's ray k at [j, k] (a caller's own jitter);
        otherwise (n x 6), and the ray's closest hit is searched once for all its samples.
        rays, ids (n x 2 int32 or None), mean (n x 4 float32) and moments are torch tensors or raw device
        pointers (ints, with n) as in radiance_device; mean not given is allocated with tensor rays.
        Asynchronous, in stream order on the context's stream. Returns (mean, moments)."""
        what = "radiance_mean_device"
        first_sample, n_samples = self._mean_samples(what, first_sample, n_samples)
        per = 6 * n_samples if per_sample_rays else 6
        specs = [("rays", rays, "float32", per, True), ("ids", ids, "int32", 2, False)]
        n, _, torch = self._query_args(what, n, specs)
        if (mean is None or moments is True) and first_sample:
            raise ValueError(f"{what}: first_sample {first_sample} continues a mean (and moments): give them")
        if torch is not None and torch.is_tensor(rays):
            if mean is None:
                mean = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            if moments is True:
                moments = torch.empty((n, 2), dtype=torch.float32, device=rays.device)
        if moments is True:
            raise ValueError(f"{what}: moments=True needs tensor rays; give a pointer")
        specs += [("mean", mean, "float32", 4, True), ("moments", moments, "float32", 2, False)]
        n, p, _ = self._query_args(what, n, specs)
        flags = RADIANCE_RAYS_PER_SAMPLE if per_sample_rays else 0
        self._ck(self._lib.pt_radiance_mean_device(self._h, p[0], p[1], n, first_sample, n_samples, flags, p[2], p[3]),
                 "pt_radiance_mean_device")
        return mean, moments

    def radiance_mean(self, rays: np.ndarray, ids=None, first_sample: int = 0, n_samples: int = 1,
                      per_sample_rays: bool = False, mean=None, moments=None):
        """radiance_mean_device on host arrays (pt_radiance_mean). rays (n, 6) or, per_sample_rays,
        (n_samples, n, 6). mean (n, 4) and moments (n, 2) are float32 arrays to go on from (required when
        first_sample is not 0; updated copies are returned), moments None for none or True for new ones.
        Synchronous. Returns (mean, moments)."""
        what = "radiance_mean"
        first_sample, n_samples = self._mean_samples(what, first_sample, n_samples)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        if per_sample_rays and r.shape[0] % n_samples:
            raise ValueError(f"{what}: {r.shape[0]} rays are no multiple of {n_samples} samples")
        n = r.shape[0] // n_samples if per_sample_rays else r.shape[0]
        i = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1, 2)
        if i is not None and i.shape[0] != n:
            raise ValueError(f"ids has {i.shape[0]} entries for {n} rays")
        if first_sample and (mean is None or moments is True):
            raise ValueError(f"{what}: first_sample {first_sample} continues a mean (and moments): give them")
        mean = np.zeros((n, 4), np.float32) if mean is None else np.array(mean, np.float32).reshape(-1, 4)
        if moments is not None:
            moments = np.zeros((n, 2), np.float32) if moments is True else np.array(moments, np.float32).reshape(-1, 2)
        if mean.shape[0] != n or (moments is not None and moments.shape[0] != n):
            raise ValueError(f"{what}: mean and moments must have {n} rows")
        flags = RADIANCE_RAYS_PER_SAMPLE if per_sample_rays else 0
        self._ck(self._lib.pt_radiance_mean(self._h, _fp(r), None if i is None else i.ctypes.data_as(_native.c_int_p), n,
                                            first_sample, n_samples, flags, _fp(mean),
                                            None if moments is None else _fp(moments)), "pt_radiance_mean")
        return mean, moments

    def build_bvh_device(self, tris: np.ndarray, leaf_size: int = 4):
        """pt_build_bvh_device: the GPU binned-SAH tree over tris (n x 36 f32) in the reference's
        node encoding. Returns (nodes (m x 12 f32, dummy node 0, root 1), order (n int32: input
        index of the triangle at each built position))."""
        t = np.ascontiguousarray(tris, np.float32).reshape(-1, 36)
        n = t.shape[0]
        cap = 2 * n + 2
        nodes = np.zeros((cap, 12), np.float32)
        order = np.empty(n, np.int32)
        m = C.c_int()
        self._ck(self._lib.pt_build_bvh_device(self._h, _fp(t), n, int(leaf_size), _fp(nodes), cap, C.byref(m),
                                               order.ctypes.data_as(_native.c_int_p)), "pt_build_bvh_device")
        return nodes[:m.value].copy(), order

    def accum(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(self._lib.pt_download_accum(self._h, _fp(out)), "pt_download_accum")
        return out

    def accum_into(self, dptr: int):
        """Copy the accumulation (H x W x 4 f32) into device memory at dptr (stream-ordered, synchronous)."""
        self._ck(self._lib.pt_download_accum(self._h, C.cast(C.c_void_p(dptr), C.POINTER(C.c_float))),
                 "pt_download_accum")

    def set_accum(self, a: np.ndarray):
        a = np.ascontiguousarray(a, np.float32).reshape(self.height, self.width, 4)
        self._ck(self._lib.pt_upload_accum(self._h, _fp(a)), "pt_upload_accum")

    def clear(self):
        self._ck(self._lib.pt_clear_accum(self._h), "pt_clear_accum")

    def accum_device_ptr(self) -> int:
        p = C.c_void_p()
        self._ck(self._lib.pt_accum_device_ptr(self._h, C.byref(p)), "pt_accum_device_ptr")
        return p.value

    def tonemap(self, limit: float = 1.5, gamma: float = 0.0) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), np.float32)
        self._ck(self._lib.pt_tonemap(self._h, float(limit), float(gamma), _fp(out)), "pt_tonemap")
        return out

    def owned_pixel_count(self, rank=None, world=None) -> int:
        c = C.c_int64()
        rank = self.tile_rank if rank is None else rank
        world = self.tile_world if world is None else world
        self._ck(self._lib.pt_owned_pixel_count(self._h, int(rank), int(world), C.byref(c)), "pt_owned_pixel_count")
        return c.value

    def pack_owned(self, dptr: int):
        self._ck(self._lib.pt_pack_owned(self._h, C.c_void_p(dptr)), "pt_pack_owned")

    def unpack_rank(self, rank: int, world: int, dptr: int):
        self._ck(self._lib.pt_unpack_rank(self._h, int(rank), int(world), C.c_void_p(dptr)), "pt_unpack_rank")

    def unpack_ranks(self, world: int, dpacked):
        """Ranks 1..world-1's packed running means (device pointers, entry 0 ignored) into the
        accumulation, one launch."""
        arr = (C.c_void_p * world)(*[C.c_void_p(int(x)) if x else C.c_void_p() for x in dpacked])
        self._ck(self._lib.pt_unpack_ranks(self._h, int(world), arr), "pt_unpack_ranks")

    def pack_owned_stats(self, dptr: int):
        """pack_owned with the moments (pt_pack_owned_stats; a Renderer(..., share_moments=True)):
        owned_pixel_count() slots of 5 f32 (r, g, b, m1, m2) into device memory."""
        self._ck(self._lib.pt_pack_owned_stats(self._h, C.c_void_p(dptr)), "pt_pack_owned_stats")

    def unpack_ranks_stats(self, world: int, dpacked):
        """unpack_ranks of pack_owned_stats buffers (pt_unpack_ranks_stats): ranks 1..world-1's running
        means and moments into the accumulation and the moments plane, one launch. Every rank must have
        rendered the same frames."""
        arr = (C.c_void_p * max(world, 1))(*[C.c_void_p(int(x)) if x else C.c_void_p() for x in dpacked]) \
            if dpacked is not None else None
        self._ck(self._lib.pt_unpack_ranks_stats(self._h, int(world), arr), "pt_unpack_ranks_stats")

    def display_pack(self, dptr: int, limit: float = 1.5, gamma: float = 0.0):
        """This rank's owned pixels of the displayed frame (pass3 into an 8-bit window), 3 u8 each."""
        self._ck(self._lib.pt_display_pack(self._h, float(limit), float(gamma), C.c_void_p(dptr)), "pt_display_pack")

    def display_own(self, dimage: int, limit: float = 1.5, gamma: float = 0.0):
        """This rank's tiles (every pixel when tile_world is 1) of the displayed frame into an H x W x 4 u8 image."""
        self._ck(self._lib.pt_display_own(self._h, float(limit), float(gamma), C.c_void_p(dimage)), "pt_display_own")

    def display_unpack(self, world: int, dpacked, dimage: int):
        """Ranks 1..world-1's packed display pixels (device pointers, entry 0 ignored) into the image."""
        arr = (C.c_void_p * world)(*[C.c_void_p(int(x)) if x else C.c_void_p() for x in dpacked])
        self._ck(self._lib.pt_display_unpack(self._h, int(world), arr, C.c_void_p(dimage)), "pt_display_unpack")

    def render_guides(self, eye, camera_rotate):
        """Guide buffers of this camera (pt_render_guides): every pixel centre's first hit. Asynchronous."""
        e = np.ascontiguousarray(eye, np.float32)
        r = np.ascontiguousarray(camera_rotate, np.float32).reshape(16)
        self._ck(self._lib.pt_render_guides(self._h, _fp(e), _fp(r)), "pt_render_guides")

    def guides(self) -> dict:
        """The guide planes, (h, w, 4) f32 each, row 0 = bottom: "pos_t" (P, t), "nrm_tri" (N, the
        triangle index's int bits) and "albedo" (baseColor, 1); "tri" is nrm_tri's last channel
        viewed as int32 (-1 = miss)."""
        out = {k: np.empty((self.height, self.width, 4), np.float32) for k in ("pos_t", "nrm_tri", "albedo")}
        self._ck(self._lib.pt_download_guides(self._h, _fp(out["pos_t"]), _fp(out["nrm_tri"]), _fp(out["albedo"])),
                 "pt_download_guides")
        out["tri"] = out["nrm_tri"][..., 3].view(np.int32)
        return out

    def guides_into(self, pos_t: int | None = None, nrm_tri: int | None = None, albedo: int | None = None):
        """Copy guide planes (H x W x 4 f32 each) into device memory at the given pointers (pt_download_guides
        with device destinations: stream-ordered, synchronous), for a consumer that stays on the GPU."""
        p = [C.cast(C.c_void_p(x), _native.c_float_p) if x else None for x in (pos_t, nrm_tri, albedo)]
        self._ck(self._lib.pt_download_guides(self._h, *p), "pt_download_guides")

    def guides_device_ptrs(self):
        p = [C.c_void_p() for _ in range(3)]
        self._ck(self._lib.pt_guides_device_ptr(self._h, *[C.byref(x) for x in p]), "pt_guides_device_ptr")
        return tuple(x.value for x in p)

    def _params(self, what, prm, defaults, params, names, ints=()):
        """prm set by its *_defaults function, then from a method's **params: `names` are the
        parameters it has, `ints` those of them that are integers."""
        defaults(C.byref(prm))
        for k, v in params.items():
            if k not in names:
                raise TypeError(f"{what}() has no parameter {k!r}")
            setattr(prm, k, int(v) if k in ints else float(v))
        return prm

    def _image(self, download: str) -> np.ndarray:
        """An (h, w, 4) f32 image through the ABI's download function of that name."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(getattr(self._lib, download)(self._h, _fp(out)), download)
        return out

    def denoise(self, out_dptr: int | None = None, download: bool = True, src_dptr: int | None = None, **params):
        """The edge-avoiding a-trous filter of the accumulation (pt_denoise) -- or, with src_dptr, of
        an H x W x 4 f32 device image such as resolved_device_ptr() (pt_denoise_from) -- steered by
        the last render_guides. params: passes, sigma_c, sigma_z, sigma_a, normal_log2, limit (defaults:
        pt_denoise_defaults). With out_dptr (H x W x 4 f32 device memory) asynchronous, returns
        None; without, returns the denoised image (h, w, 4) -- or, with download False, leaves it
        in the context's buffer (denoised_device_ptr, display_denoised) without synchronising."""
        prm = self._params("denoise", _native.PtDenoiseParams(), self._lib.pt_denoise_defaults, params,
                           ("passes", "sigma_c", "sigma_z", "sigma_a", "normal_log2", "limit"),
                           ("passes", "normal_log2"))
        out_p = C.c_void_p(out_dptr) if out_dptr else None
        if src_dptr:
            self._ck(self._lib.pt_denoise_from(self._h, C.byref(prm), C.c_void_p(src_dptr), out_p), "pt_denoise_from")
        else:
            self._ck(self._lib.pt_denoise(self._h, C.byref(prm), out_p), "pt_denoise")
        if out_dptr or not download:
            return None
        return self._image("pt_download_denoised")

    def denoised_device_ptr(self) -> int:
        p = C.c_void_p()
        self._ck(self._lib.pt_denoised_device_ptr(self._h, C.byref(p)), "pt_denoised_device_ptr")
        return p.value

    def display_denoised(self, dimage: int, limit: float = 1.5, gamma: float = 0.0):
        """The last denoise()'s image through the 8-bit display path into an H x W x 4 u8 device image."""
        self._ck(self._lib.pt_display_denoised(self._h, float(limit), float(gamma), C.c_void_p(dimage)),
                 "pt_display_denoised")

    def moments(self) -> np.ndarray:
        """The running means (m1, m2) of the sample luminance and of its square, (h, w, 2), row 0 =
        bottom (pt_download_moments; a Renderer(..., moments=True))."""
        out = np.empty((self.height, self.width, 2), np.float32)
        self._ck(self._lib.pt_download_moments(self._h, _fp(out)), "pt_download_moments")
        return out

    def moments_frames(self) -> int:
        """The frames the moments hold; 0 when they are not valid or the context keeps none."""
        n = C.c_uint32()
        self._ck(self._lib.pt_moments_frames(self._h, C.byref(n)), "pt_moments_frames")
        return n.value

    def moments_device_ptr(self) -> int:
        p = C.c_void_p()
        self._ck(self._lib.pt_moments_device_ptr(self._h, C.byref(p)), "pt_moments_device_ptr")
        return p.value

    def denoise_var(self, out_dptr: int | None = None, download: bool = True, src_dptr: int | None = None, **params):
        """The variance-guided a-trous filter (pt_denoise_var) of the accumulation -- or, with
        src_dptr, of an H x W x 4 f32 device image such as resolved_device_ptr() -- steered by the
        last render_guides and by the sample moments (a Renderer(..., moments=True) that holds
        min_temporal frames; else by a spatial variance estimate). params: passes, sigma_l, sigma_z,
        sigma_a, normal_log2, limit, min_temporal (defaults: pt_denoise_var_defaults). Returns as
        denoise() does; the image is the context's denoised image (denoised_device_ptr,
        display_denoised)."""
        prm = self._params("denoise_var", _native.PtDenoiseVarParams(), self._lib.pt_denoise_var_defaults, params,
                           ("passes", "sigma_l", "sigma_z", "sigma_a", "normal_log2", "limit", "min_temporal"),
                           ("passes", "normal_log2", "min_temporal"))
        out_p = C.c_void_p(out_dptr) if out_dptr else None
        self._ck(self._lib.pt_denoise_var(self._h, C.byref(prm), C.c_void_p(src_dptr) if src_dptr else None, out_p),
                 "pt_denoise_var")
        if out_dptr or not download:
            return None
        return self._image("pt_download_denoised")

    def variance(self) -> np.ndarray:
        """The initial variance plane (h, w) of the last denoise_var (pt_download_variance)."""
        out = np.empty((self.height, self.width), np.float32)
        self._ck(self._lib.pt_download_variance(self._h, _fp(out)), "pt_download_variance")
        return out

    def adaptive_update(self, **params):
        """One adaptive-sampling decision (pt_adaptive_update; a Renderer(..., adaptive=True)): every
        8x8 tile whose pixels' standard error of the tone-mapped luminance is <= threshold, once the
        moments hold min_frames frames, retires and takes no more samples until the running mean
        restarts. params: threshold, limit, min_frames (defaults: pt_adaptive_defaults). Asynchronous."""
        prm = self._params("adaptive_update", _native.PtAdaptiveParams(), self._lib.pt_adaptive_defaults, params,
                           ("threshold", "limit", "min_frames"), ("min_frames",))
        self._ck(self._lib.pt_adaptive_update(self._h, C.byref(prm)), "pt_adaptive_update")

    def adaptive_status(self) -> AdaptiveStatus:
        """Tiles, how many have retired, the frames at the last update and the largest error still active."""
        s = _native.PtAdaptiveState()
        self._ck(self._lib.pt_adaptive_status(self._h, C.byref(s)), "pt_adaptive_status")
        return AdaptiveStatus(s.tiles, s.retired, s.frames, s.max_err2)

    def tile_error(self):
        """(err2, retired_at): per 8x8 tile, (tilesY, tilesX) f32 / uint32, row 0 = bottom
        (pt_download_tile_error): the squared error the last update found and the frame count at
        which the tile retired (0: active)."""
        shape = ((self.height + 7) // 8, (self.width + 7) // 8)
        err2 = np.empty(shape, np.float32)
        at = np.empty(shape, np.uint32)
        self._ck(self._lib.pt_download_tile_error(self._h, _fp(err2), at.ctypes.data_as(C.POINTER(C.c_uint32))),
                 "pt_download_tile_error")
        return err2, at

    def temporal_resolve(self, frames: int, out_dptr: int | None = None, download: bool = True, **params):
        """The running mean of `frames` frames (frameCounter + 1) blended with the committed history
        of the previous camera, reprojected through the last render_guides (pt_temporal_resolve).
        params: sigma_z, normal_cos, max_history (defaults: pt_temporal_defaults). With out_dptr
        (H x W x 4 f32 device memory) asynchronous, returns None -- such a resolve cannot be
        committed; without, returns the resolved image (h, w, 4), .w = the sample count -- or, with
        download False, leaves it in the context's buffer (resolved_device_ptr, display_resolved,
        denoise(src_dptr=...)) without synchronising."""
        prm = self._params("temporal_resolve", _native.PtTemporalParams(), self._lib.pt_temporal_defaults, params,
                           ("sigma_z", "normal_cos", "max_history"))
        self._ck(self._lib.pt_temporal_resolve(self._h, C.byref(prm), int(frames) & 0xFFFFFFFF,
                                               C.c_void_p(out_dptr) if out_dptr else None), "pt_temporal_resolve")
        if out_dptr or not download:
            return None
        return self._image("pt_download_resolved")

    def temporal_commit(self):
        """The last temporal_resolve's image and the current guides become the history (before the
        camera moves: commit, then render_guides of the new camera)."""
        self._ck(self._lib.pt_temporal_commit(self._h), "pt_temporal_commit")

    def temporal_reset(self):
        """Drops the history: the next temporal_resolve returns the running mean itself."""
        self._ck(self._lib.pt_temporal_reset(self._h), "pt_temporal_reset")

    def resolved_device_ptr(self) -> int:
        p = C.c_void_p()
        self._ck(self._lib.pt_resolved_device_ptr(self._h, C.byref(p)), "pt_resolved_device_ptr")
        return p.value

    def display_resolved(self, dimage: int, limit: float = 1.5, gamma: float = 0.0):
        """The last temporal_resolve()'s image through the 8-bit display path into an H x W x 4 u8 device image."""
        self._ck(self._lib.pt_display_resolved(self._h, float(limit), float(gamma), C.c_void_p(dimage)),
                 "pt_display_resolved")

    def set_stream(self, stream_ptr: int | None):
        self._ck(self._lib.pt_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None), "pt_set_stream")

    def synchronize(self):
        self._ck(self._lib.pt_synchronize(self._h), "pt_synchronize")

    def stats(self) -> FrameStats:
        s = _native.PtFrameStats()
        self._ck(self._lib.pt_get_stats(self._h, C.byref(s)), "pt_get_stats")
        return FrameStats(s.rays, s.node_fetch, s.tri_fetch, s.mat_fetch, s.tex_fetch, s.kernel_ms,
                          s.kernel_ms_total, s.launches, s.max_stack, s.split_items, s.runtime_tree,
                          s.waves_per_simd, s.devices, s.gather, s.frames_in_flight, s.upload_ms,
                          s.accel_build_ms, s.accel_device, s.accel_nodes, s.accel_depth, s.regen, s.frames,
                          s.frame_batch, s.env_compact, s.tree4_nodes)

    def fmath_device(self, fn: int, x, y=None) -> np.ndarray:
        """Diagnostics: include/pt_fmath.h function `fn` (pt_fmath_device's ids 0..10) of x (and y)
        on this context's GPU; pt_fmath_host gives the same bits on the CPU."""
        x = np.ascontiguousarray(x, np.float32)
        y = None if y is None else np.ascontiguousarray(y, np.float32)
        out = np.empty_like(x)
        self._ck(self._lib.pt_fmath_device(self._h, int(fn), _fp(x), None if y is None else _fp(y), x.size, _fp(out)),
                 "pt_fmath_device")
        return out

    def sph_texel(self, w: int, h: int, dirs):
        """Diagnostics (pt_sph_texel_device): the sky texel y * w + x of each direction (n x 3, used
        as given, not normalised) in a w x h map, by the kernels' fast decision and by its correctly
        rounded fallback: (texel, texel_exact), int32 each."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = d.shape[0]
        t = np.empty(n, np.int32)
        te = np.empty(n, np.int32)
        self._ck(self._lib.pt_sph_texel_device(self._h, int(w), int(h), _fp(d), n, t.ctypes.data_as(_native.c_int_p),
                                               te.ctypes.data_as(_native.c_int_p)), "pt_sph_texel_device")
        return t, te

    def reset_stats(self):
        self._ck(self._lib.pt_reset_stats(self._h), "pt_reset_stats")
