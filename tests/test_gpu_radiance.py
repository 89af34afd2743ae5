"""Radiance along caller-supplied rays on the GPU (pt_radiance_device, pt_radiance, pt_camera_rays_device)
against its contract: a ray that is bit for bit the camera ray of pixel (px, py) of sample s yields the
sample a frame with that sample index gives the pixel, bit for bit, for any camera, in any order, in any
batch. The reference is the oracle's frame, one sample at a time (tests/radiance_ref.py oracle_sample), and
the oracle's closest hit for t. Images are 33 x 31 (1023 rays: hits and sky on c2); the radiance calls run
on a 64 x 64 context, so nothing can leak from the context's size. Every comparison is on bits.

References are computed once per case (frame_case) and shared: do not write to them."""
import ctypes as C
import functools

import numpy as np
import pytest

import material_scene as ms
import oracle
import radiance_ref as rf
import refit_ref as rr
from opengl_ray_tracing_amd import FLAG_NO_CULL, FLAG_REFERENCE_TREE, Renderer, _native, orbit_camera
from post_common import INVALID, NOSCENE, bits, config

pytestmark = pytest.mark.gpu

F = np.float32
CW, CH = 33, 31
N = CW * CH
SAMPLES = (0, 7)
PREFIXES = [1, 63, 64, 65, 1023]
# name -> (scene, integrator, max_bounce)
CASES = {
    "c2-lambert": ("c2", "lambert", 2),
    "c3-mis2": ("c3", "mis", 2),
    "c3-disney5": ("c3", "disney", 5),
    "c4-mis8": ("c4", "mis", 8),
    "material-lambert": ("material", "lambert", 2),
    "material-disney": ("material", "disney", 5),
    "material-mis": ("material", "mis", 2),
    "c2-noenv": ("c2-noenv", "lambert", 2),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (tris, nodes, hdr, cache, eye, rot) of a scene name above"""
    if name == "material":
        tris, nodes, hdr, cache, eye, rot, *_ = ms.build()
        return tris, nodes, hdr, cache, eye, rot
    cfg, tris, nodes, hdr, eye, rot = config(name.split("-")[0])
    return tris, nodes, (None if name.endswith("-noenv") else hdr), None, eye, rot


@functools.lru_cache(maxsize=None)
def the_oracle(name):
    tris, nodes, hdr, cache, _, _ = scene(name)
    return oracle.Oracle(tris, nodes, hdr, cache)


@functools.lru_cache(maxsize=None)
def cameras():
    """c2's own camera and two whose eye lies inside the scene's bounding box -> ((eye, rot), ...)"""
    tris = scene("c2")[0]
    p = np.asarray(tris, F).reshape(-1, 36)[:, 0:9].reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    cams = [scene("c2")[4:6]]
    for frac, angles in (((0.5, 0.55, 0.5), (40.0, 10.0, 1.0)), ((0.3, 0.7, 0.6), (120.0, 30.0, 1.0))):
        eye = (lo + (hi - lo) * np.array(frac, F)).astype(F)
        assert np.all(eye > lo) and np.all(eye < hi)
        cams.append((eye, orbit_camera(*angles)[1]))
    return tuple(cams)


@functools.lru_cache(maxsize=None)
def frame_case(case, s, cam=0):
    """The camera rays of sample s of a case at CW x CH, and what the oracle's frame gives them:
    -> (rays (N, 6), want (N, 4): the frame's sample rgb and the closest hit's t). cam: cameras()' index (c2)."""
    name, integ, mb = CASES[case]
    tris, nodes, hdr, cache, eye, rot = scene(name)
    if cam:
        eye, rot = cameras()[cam]
    rays = rf.camera_rays(CW, CH, eye, rot, s)
    orc = the_oracle(name)
    want = rf.oracle_sample(orc, CW, CH, integ, mb, eye, rot, s).reshape(-1, 4).copy()
    t, tri, _ = orc.trace_closest(rays)
    want[:, 3] = np.where(tri >= 0, t, rf.MISS_T)
    if name.startswith("c2") and not cam:
        assert 0.1 < (tri >= 0).mean() < 0.95  # hits and sky
    assert cam == 0 or 0.1 < (tri >= 0).mean() < 0.95  # the other cameras see geometry and sky too
    for a in (rays, want):
        a.setflags(write=False)
    return rays, want


def context(case, w=64, h=64, flags=0):
    name, integ, mb = CASES[case]
    tris, nodes, hdr, cache, _, _ = scene(name)
    r = Renderer(w, h, integ, max_bounce=mb, flags=flags)
    r.upload_scene(tris, nodes)
    if hdr is not None:
        r.upload_env(hdr, cache)
    return r


def dev(a):
    """a numpy array as a tensor on the GPU, there before anything of the renderer's stream reads it"""
    import torch
    t = torch.from_numpy(np.array(a)).to("cuda:0")  # a copy: the shared references are read-only
    torch.cuda.synchronize()
    return t


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want, what):
    got = np.asarray(got, F).reshape(-1, 4)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rays differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


IDS = rf.pixel_ids(CW, CH)


# ------------------------------------------------------------------ 1. camera rays
@pytest.mark.parametrize("s", [0, 7, 2**32 - 1])
def test_camera_rays(s):
    import torch
    _, _, _, _, eye, rot = scene("c2")
    want = rf.camera_rays(CW, CH, eye, rot, s)
    with Renderer(CW, CH, "lambert") as r:
        rays, ids = r.camera_rays_device(eye, rot, s)
        assert rays.shape == (N, 6) and rays.dtype == torch.float32 and ids.shape == (N, 2) and ids.dtype == torch.int32
        r.synchronize()
        assert np.array_equal(bits(host(rays)), bits(want))
        assert np.array_equal(host(ids), IDS)
        # d_ids NULL
        alone = torch.zeros((N, 6), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        e, m = np.ascontiguousarray(eye, F), np.ascontiguousarray(rot, F).reshape(16)
        fp = _native.c_float_p
        assert r._lib.pt_camera_rays_device(r._h, e.ctypes.data_as(fp), m.ctypes.data_as(fp), s,
                                            C.c_void_p(alone.data_ptr()), None) == 0
        r.synchronize()
        assert np.array_equal(bits(host(alone)), bits(want))


# ------------------------------------------------------------------ 2. the frame's samples
@pytest.mark.parametrize("case", [c for c in CASES])
def test_equals_the_frames_samples(case):
    with context(case) as r:
        for s in SAMPLES:
            rays, want = frame_case(case, s)
            same(r.radiance(rays, IDS, s), want, f"{case} sample {s}")
    if case == "c2-noenv":
        rays, want = frame_case(case, 0)
        sky = want[:, 3] == rf.MISS_T
        assert sky.any() and not want[sky, 0:3].any()  # a black sky


@pytest.mark.parametrize("flags", [FLAG_REFERENCE_TREE, FLAG_NO_CULL], ids=["reference_tree", "no_cull"])
def test_c2_on_the_other_trees(flags):
    with context("c2-lambert", flags=flags) as r:
        assert r.stats().max_stack > 32  # the reference tree is deeper than the LDS stack: the overflow area is in use
        for s in SAMPLES:
            rays, want = frame_case("c2-lambert", s)
            same(r.radiance(rays, IDS, s), want, f"flags {flags:#x} sample {s}")


# ------------------------------------------------------------------ 3. order and batch
@functools.lru_cache(maxsize=None)
def shuffled_case(s=7):
    """Three cameras' rays of sample s concatenated and shuffled -> (rays, ids, want)"""
    parts = [frame_case("c2-lambert", s, cam) for cam in range(len(cameras()))]
    rays = np.concatenate([p[0] for p in parts])
    want = np.concatenate([p[1] for p in parts])
    ids = np.concatenate([IDS] * len(parts))
    perm = np.random.RandomState(1234).permutation(len(rays))
    return tuple(np.ascontiguousarray(a[perm]) for a in (rays, ids, want))


def test_order_and_batch():
    s = 7
    rays, ids, want = shuffled_case(s)
    assert len(rays) == 3 * N
    with context("c2-lambert") as r:
        same(r.radiance(rays, ids, s), want, "three cameras shuffled")
        d_rays, d_ids = dev(rays), dev(ids)
        for n in PREFIXES:
            out = r.radiance_device(d_rays[:n], d_ids[:n], s)
            r.synchronize()
            same(host(out), want[:n], f"prefix {n}")


def test_default_ids():
    """ids None is (k & 4095, k >> 12): more than one row of ids, and the explicit form agrees. The first image
    row's pixels have their default ids ((k, 0), k < CW), so its rays give the frame's samples either way."""
    s = 7
    rays0, want0 = frame_case("c2-lambert", s)
    rays3 = shuffled_case(s)[0]
    rays = np.ascontiguousarray(np.concatenate([rays0, rays3, rays3])[:4096 + 65])
    ids = rf.default_ids(len(rays))
    assert ids[:, 1].max() == 1 and np.array_equal(ids[:CW], IDS[:CW])
    with context("c2-lambert") as r:
        a = r.radiance(rays, None, s)
        b = r.radiance(rays, ids, s)
        d = r.radiance_device(dev(rays), None, s)
        r.synchronize()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(host(d)))
    same(a[:CW], want0[:CW], "the first image row under the default ids")


# ------------------------------------------------------------------ 4. forms
def test_host_device_and_torch_stream():
    import torch
    s = 7
    rays, ids, want = shuffled_case(s)
    with context("c2-lambert") as r:
        h = r.radiance(rays, ids, s)
        d = r.radiance_device(dev(rays), dev(ids), s)
        r.synchronize()
        assert np.array_equal(bits(h), bits(host(d)))
        same(h, want, "host form")
        # tensors produced and consumed on a torch stream the context was given
        base, base_ids = dev(rays), dev(ids)
        st = torch.cuda.Stream()
        r.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            d_rays = torch.cat([base[:, 0:3] * 1.0, base[:, 3:6] + 0.0], dim=1).contiguous()
            d_ids = base_ids.clone()
            out = r.radiance_device(d_rays, d_ids, s)
            hits = (out[:, 3] < float(rf.MISS_T)).sum()
        st.synchronize()
        assert out.dtype == torch.float32 and out.shape == (len(rays), 4)
        same(out.cpu().numpy(), want, "torch stream")
        assert int(hits) == int((want[:, 3] < rf.MISS_T).sum())
        # raw pointers with n into a tensor of the caller's
        mine = torch.full((len(rays), 4), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.radiance_device(d_rays.data_ptr(), d_ids.data_ptr(), s, mine.data_ptr(), n=len(rays))
        r.synchronize()
        same(mine.cpu().numpy(), want, "raw pointers")
        for kw in (dict(rays=d_rays.double()), dict(rays=d_rays, ids=d_ids.long()), dict(rays=d_rays, ids=d_ids[:-1]),
                   dict(rays=d_rays, out=mine[:-1]), dict(rays=d_rays.cpu()), dict(rays=d_rays.data_ptr())):
            with pytest.raises(ValueError):
                r.radiance_device(**kw)
        r.set_stream(None)


# ------------------------------------------------------------------ 5. between frames in flight
def test_between_frames_in_flight():
    """Frames, a radiance call, more frames, no synchronisation in between: neither disturbs the other."""
    s = 7
    rays, want = frame_case("c2-lambert", s)
    _, _, _, _, eye, rot = scene("c2")

    def run(query):
        with context("c2-lambert", 100, 76) as r:
            d_rays, d_ids = dev(rays), dev(IDS)
            out = None
            r.render_frames(eye, rot, 0, 8)
            if query:
                out = r.radiance_device(d_rays, d_ids, s)
            r.render_frames(eye, rot, 8, 8)
            acc = r.accum()
            st = r.stats()
            return acc, st, None if out is None else host(out)

    acc_q, st_q, out = run(True)
    acc, st, _ = run(False)
    same(out, want, "radiance between frames")
    assert np.array_equal(bits(acc_q), bits(acc))
    assert st_q.rays == st.rays and st_q.frames == st.frames == 16  # pt_frame_stats is not touched


# ------------------------------------------------------------------ 6. after update_geometry
@pytest.mark.parametrize("integ,mb", [("lambert", 2), ("mis", 2)])
def test_after_update_geometry(integ, mb):
    sc, k, s = "material", 1, 7
    tris0, nodes0, hdr, cache, eye, rot, _, _ = rr.scene_arrays(sc)
    tris_k, nodes_k, _ = rr.posed(sc, k)
    rays = rf.camera_rays(CW, CH, eye, rot, s)

    def ctx(tris, nodes):
        r = Renderer(64, 64, integ, max_bounce=mb)
        r.upload_scene(tris, nodes)
        r.upload_env(hdr, cache)
        return r

    with ctx(tris0, nodes0) as a, ctx(tris_k, nodes_k) as b:
        before = a.radiance(rays, IDS, s)
        a.update_geometry(rr.pose(tris0, k))
        got, fresh = a.radiance(rays, IDS, s), b.radiance(rays, IDS, s)
    assert np.array_equal(bits(got), bits(fresh))
    assert not np.array_equal(bits(got), bits(before))  # the pose moves what the rays see
    want = rf.oracle_sample(oracle.Oracle(tris_k, nodes_k, hdr, cache), CW, CH, integ, mb, eye, rot, s).reshape(-1, 4)
    assert np.array_equal(bits(got[:, 0:3]), bits(want[:, 0:3]))


# ------------------------------------------------------------------ 7. errors
def test_error_paths():
    import torch
    rays, want = frame_case("c2-lambert", 0)
    tris, nodes, *_ = scene("c2")
    lib = _native.load()
    n = 64
    fp, ip = _native.c_float_p, _native.c_int_p
    h_rays, h_ids = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(IDS[:n])
    h_out = np.full((n, 4), -5.0, F)
    d_rays, d_ids = dev(h_rays), dev(h_ids)
    d_out = torch.full((n, 4), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def calls(r, count, with_rays=True, with_out=True):
        return [
            lib.pt_radiance(r._h, h_rays.ctypes.data_as(fp) if with_rays else None, h_ids.ctypes.data_as(ip), count, 0,
                            h_out.ctypes.data_as(fp) if with_out else None),
            lib.pt_radiance_device(r._h, C.c_void_p(d_rays.data_ptr()) if with_rays else None,
                                   C.c_void_p(d_ids.data_ptr()), count, 0,
                                   C.c_void_p(d_out.data_ptr()) if with_out else None),
        ]

    def untouched():
        torch.cuda.synchronize()
        return bool(np.all(h_out == F(-5.0))) and bool((d_out == -5.0).all())

    with Renderer(16, 16, "lambert") as r:
        assert calls(r, n) == [NOSCENE] * 2  # before pt_upload_scene
        assert calls(r, -1) == [INVALID] * 2
        r.upload_scene(tris, nodes)
        assert calls(r, -1) == [INVALID] * 2
        assert calls(r, n, with_rays=False) == [INVALID] * 2
        assert calls(r, n, with_out=False) == [INVALID] * 2
        assert calls(r, 0) == [0] * 2  # n == 0: PT_OK, nothing read or written
        assert calls(r, 0, with_rays=False, with_out=False) == [0] * 2
        r.synchronize()
        assert untouched()
        assert lib.pt_last_error(r._h)
        # the same buffers take results once the call is valid (no env: the hits' paths see a black sky)
        assert calls(r, n) == [0] * 2
        r.synchronize()
        assert np.array_equal(bits(h_out), bits(host(d_out)))
        assert np.array_equal(bits(h_out[:, 3]), bits(want[:n, 3]))
        e, m = np.zeros(3, F), np.eye(4, dtype=F).reshape(16)
        assert lib.pt_camera_rays_device(r._h, e.ctypes.data_as(fp), m.ctypes.data_as(fp), 0, None, None) == INVALID
        with pytest.raises(ValueError):
            r.radiance(rays[:4], IDS[:3])
    with Renderer(16, 16, "basic") as r:  # the BASIC integrator has no scene of triangles
        assert calls(r, n) == [NOSCENE] * 2
        big = torch.zeros((16 * 16, 6), dtype=torch.float32, device="cuda:0")
        e, m = np.zeros(3, F), np.eye(4, dtype=F).reshape(16)
        assert lib.pt_camera_rays_device(r._h, e.ctypes.data_as(fp), m.ctypes.data_as(fp), 0,
                                         C.c_void_p(big.data_ptr()), None) == INVALID
