"""Adaptive sampling on the GPU (PT_FLAG_ADAPTIVE, pt_adaptive_update, pt_adaptive_status,
pt_download_tile_error) against the float32 restatement tests/adaptive_ref.py on the oracle's own
samples, bit for bit: the accumulation, the moments and the two tile planes after every update
through every frame kernel and both calling patterns, the rays a retired tile no longer costs, a
context that retires nothing (a PT_FLAG_MOMENTS context), one that retires everything, updates
between launches in flight, restarts and invalidation, the error paths, and the filters after it.

Unless stated a run is 32 frames as 4 x (render_frames of 8, then adaptive_update at a threshold
of 4/255, limit 1.5, min_frames 8).
"""
import numpy as np
import pytest

import adaptive_ref as ar
import variance_ref as vr
from adaptive_common import EVERY, FRAMES, PRM, case, samples, the_oracle
from post_common import INVALID, bits, device_plane, rc_of
from opengl_ray_tracing_amd import Renderer
from opengl_ray_tracing_amd.renderer import FLAG_ADAPTIVE, FLAG_MEGAKERNEL, FLAG_MOMENTS, FLAG_NO_BINS, FLAG_REGEN

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (5, 3), (33, 31), (100, 76)]
KERNELS = [("c2", 0), ("c2", FLAG_MEGAKERNEL), ("c3", 0), ("c4", 0), ("c3-disney", FLAG_REGEN)]
KERNEL_IDS = ["c2-regen", "c2-megakernel", "c3-mis-regen", "c4-mis-megakernel", "c3-disney-narrow-regen"]


def renderer(name, w, h, **kw):
    integ, mb, tris, nodes, hdr, _, _ = case(name)
    r = Renderer(w, h, integ, max_bounce=mb, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


def check_state(r, want, k, what=""):
    """The context after the restatement's update k: the four planes and the status."""
    acc, m, err2, at = want["history"][k]
    frames = (k + 1) * EVERY
    assert np.array_equal(bits(r.accum()), bits(acc)), (what, k)
    assert np.array_equal(bits(r.moments()), bits(m)), (what, k)
    e, a = r.tile_error()
    assert e.shape == err2.shape and a.dtype == np.uint32
    assert np.array_equal(bits(e), bits(err2)), (what, k)
    assert np.array_equal(a, at), (what, k)
    st = r.adaptive_status()
    assert (st.tiles, st.retired, st.frames) == (at.size, want["counts"][k], frames), (what, k, st)
    assert np.array_equal(bits(F(st.max_err2)), bits(want["max_err2"][k])), (what, k, st)
    assert r.moments_frames() == frames


def standard_run(r, eye, rot, want=None, what=""):
    for k in range(FRAMES // EVERY):
        r.render_frames(eye, rot, k * EVERY, EVERY)
        r.adaptive_update(**PRM)
        if want is not None:
            check_state(r, want, k, what)


# ------------------------------------------------------------------ 1. equals the restatement
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name,flags", KERNELS, ids=KERNEL_IDS)
def test_equals_the_restatement(name, flags, w, h):
    *_, eye, rot = case(name)
    want = ar.run(samples(name, w, h), EVERY, PRM)
    with renderer(name, w, h, flags=flags, adaptive=True) as r:
        st = r.adaptive_status()
        assert (st.tiles, st.retired, st.frames, st.max_err2) == (want["retired_at"].size, 0, 0, 0.0)
        standard_run(r, eye, rot, want, "batches")
        stats = r.stats()
    assert stats.regen == (0 if name == "c4" or flags & FLAG_MEGAKERNEL else 1), stats


@pytest.mark.parametrize("name,flags", KERNELS, ids=KERNEL_IDS)
def test_single_calls_equal_the_restatement(name, flags):
    """32 render_frame calls: the per-call megakernel path, which now runs behind the camera-ray pass."""
    w, h = 33, 31
    *_, eye, rot = case(name)
    want = ar.run(samples(name, w, h), EVERY, PRM)
    with renderer(name, w, h, flags=flags, adaptive=True) as r:
        for f in range(FRAMES):
            r.render_frame(eye, rot, f)
            if f % EVERY == EVERY - 1:
                r.adaptive_update(**PRM)
                check_state(r, want, f // EVERY, "calls")


# ------------------------------------------------------------------ 2. rays
@pytest.mark.parametrize("w,h", [(33, 31), (100, 76)])
def test_retired_tiles_cost_no_rays(w, h):
    name = "c2"
    integ, mb, *_, eye, rot = case(name)
    want = ar.run(samples(name, w, h), EVERY, PRM)
    orc = the_oracle(name)
    rays = 0
    for f, active in enumerate(want["active"]):
        ys, xs = np.nonzero(active)
        assert ys.size  # (an empty pixel list would mean every pixel)
        rays += orc.render(w, h, integ, f, eye, rot, pixels=np.stack([xs, ys], -1), max_bounce=mb)[1].rays
    with renderer(name, w, h, adaptive=True) as r, renderer(name, w, h, moments=True) as plain:
        standard_run(r, eye, rot)
        for k in range(FRAMES // EVERY):
            plain.render_frames(eye, rot, k * EVERY, EVERY)
        got, full = r.stats().rays, plain.stats().rays
    print(f"c2 {w}x{h}: rays {got} adaptive, {full} with every pixel ({1 - got / full:.3f} saved)")
    assert got == rays
    assert got < full


# ------------------------------------------------------------------ 3. nothing retired is a moments context
@pytest.mark.parametrize("name,flags", [("c2", 0), ("c4", 0)], ids=["c2-regen", "c4-mis-megakernel"])
def test_nothing_retired_is_a_moments_context(name, flags):
    w, h = 33, 31
    *_, eye, rot = case(name)
    s = samples(name, w, h)
    never = {**PRM, "min_frames": 1000}
    with renderer(name, w, h, flags=flags, adaptive=True) as r, renderer(name, w, h, flags=flags, moments=True) as plain:
        def same():
            assert np.array_equal(bits(r.accum()), bits(plain.accum()))
            assert np.array_equal(bits(r.moments()), bits(plain.moments()))
            assert r.stats().rays == plain.stats().rays
        for x in (r, plain):
            x.render_frames(eye, rot, 0, EVERY)
        same()  # before any update
        e, at = r.tile_error()
        assert not e.any() and not at.any()
        for k in range(1, FRAMES // EVERY):
            r.adaptive_update(**never)
            for x in (r, plain):
                x.render_frames(eye, rot, k * EVERY, EVERY)
            same()
        r.adaptive_update(**never)
        acc, m = r.accum(), r.moments()
        e, at = r.tile_error()
        st = r.adaptive_status()
        assert st.retired == 0 and not at.any() and st.frames == FRAMES
        assert np.array_equal(bits(e), bits(ar.tile_error(acc, m, FRAMES, PRM["limit"])))
        assert np.array_equal(bits(F(st.max_err2)), bits(e.max()))
        # ... and the oracle's
        fold = ar.run(s, EVERY, never)
        assert np.array_equal(bits(acc), bits(fold["acc"])) and np.array_equal(bits(m), bits(fold["m"]))
        assert np.array_equal(bits(e), bits(fold["err2"]))


# ------------------------------------------------------------------ 4. everything retired
@pytest.mark.parametrize("w,h", [(33, 31), (160, 32)])
@pytest.mark.parametrize("name,flags", [("c2", 0), ("c2", FLAG_MEGAKERNEL)], ids=["regen", "megakernel"])
def test_everything_retired_costs_nothing(name, flags, w, h):
    *_, eye, rot = case(name)
    with renderer(name, w, h, flags=flags, adaptive=True) as r:
        r.render_frames(eye, rot, 0, 2)
        r.adaptive_update(threshold=1e30, min_frames=2)
        st = r.adaptive_status()
        assert st.retired == st.tiles == ((w + 7) // 8) * ((h + 7) // 8) and st.max_err2 == 0.0
        assert np.all(r.tile_error()[1] == 2)
        acc, m, rays = r.accum(), r.moments(), r.stats().rays
        r.render_frames(eye, rot, 2, 13)
        r.render_frame(eye, rot, 15)
        assert np.array_equal(bits(r.accum()), bits(acc)) and np.array_equal(bits(r.moments()), bits(m))
        assert r.stats().rays == rays
        assert r.moments_frames() == 16


# ------------------------------------------------------------------ 5. in flight
@pytest.mark.parametrize("name,flags", [("c2", 0), ("c4", 0)], ids=["c2-regen", "c4-mis-megakernel"])
def test_update_between_launches_in_flight(name, flags):
    """Six launches of four frames enqueued at once, the update and two more launches behind them
    with no synchronisation in between: the restatement deciding once, at 24."""
    w, h = 100, 76
    *_, eye, rot = case(name)
    want = ar.run(samples(name, w, h), EVERY, PRM, updates_at=[24])
    assert 0 < want["counts"][0] < want["retired_at"].size
    with renderer(name, w, h, flags=flags, adaptive=True, frame_batch=4) as r:
        r.render_frames(eye, rot, 0, 24)
        r.adaptive_update(**PRM)
        r.render_frames(eye, rot, 24, 8)
        assert np.array_equal(bits(r.accum()), bits(want["acc"]))
        assert np.array_equal(bits(r.moments()), bits(want["m"]))
        e, at = r.tile_error()
        assert np.array_equal(bits(e), bits(want["err2"])) and np.array_equal(at, want["retired_at"])
        st = r.adaptive_status()
        assert (st.retired, st.frames) == (want["counts"][0], 24)


def test_update_and_frames_on_different_streams():
    """pt_set_stream between an update and the next frames, and between frames and the update: the
    planes' event orders them."""
    import torch
    name, w, h = "c2", 100, 76
    *_, eye, rot = case(name)
    want = ar.run(samples(name, w, h), EVERY, PRM)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with renderer(name, w, h, adaptive=True) as r:
        r.set_stream(s1.cuda_stream)
        r.render_frames(eye, rot, 0, EVERY)
        r.adaptive_update(**PRM)
        r.set_stream(s2.cuda_stream)
        r.render_frames(eye, rot, EVERY, EVERY)
        r.set_stream(s1.cuda_stream)
        r.adaptive_update(**PRM)
        r.set_stream(None)
        check_state(r, want, 1, "streams")
        r.set_stream(s2.cuda_stream)
        r.render_frames(eye, rot, 2 * EVERY, EVERY)
        r.adaptive_update(**PRM)
        check_state(r, want, 2, "streams")
        r.set_stream(None)


# ------------------------------------------------------------------ 6. restart and invalidation
def test_restart_and_invalidation():
    name, w, h = "c2", 33, 31
    integ, mb, tris, nodes, hdr, eye, rot = case(name)
    s = samples(name, w, h)
    plain8 = np.zeros((h, w, 4), F)
    for k in range(EVERY):
        plain8 = vr.mix_sample(plain8, s[k], k)
    want = ar.run(s, EVERY, PRM)
    with renderer(name, w, h, adaptive=True) as r:
        def retire():
            r.render_frames(eye, rot, 0, EVERY)
            r.adaptive_update(**PRM)
            st = r.adaptive_status()
            assert st.retired == want["counts"][0] > 0 and st.frames == EVERY
        def cleared():
            st = r.adaptive_status()
            e, at = r.tile_error()
            assert st.retired == 0 and st.frames == 0 and st.max_err2 == 0.0 and not at.any() and not e.any()
        retire()
        r.render_frames(eye, rot, 0, EVERY)  # a restart: every tile renders again
        cleared()
        assert np.array_equal(bits(r.accum()), bits(plain8))
        assert np.array_equal(bits(r.accum()), bits(want["history"][0][0]))
        for drop in (r.clear, lambda: r.set_accum(plain8), lambda: r.upload_scene(tris, nodes),
                     lambda: r.upload_env(hdr)):
            retire()
            drop()
            cleared()
            assert rc_of(r.adaptive_update, **PRM) == INVALID  # the moments are not valid
        # a gap in frameCounter: no update, and the retired stay retired until a restart
        retire()
        acc, m = r.accum(), r.moments()
        _, at = r.tile_error()
        gone = ar.pixel_mask(at, h, w)
        r.render_frame(eye, rot, EVERY + 3)
        assert r.moments_frames() == 0
        assert rc_of(r.adaptive_update, **PRM) == INVALID
        assert r.adaptive_status().retired == want["counts"][0]
        assert np.array_equal(r.tile_error()[1], at)
        acc2, m2 = r.accum(), r.moments()
        assert np.array_equal(bits(acc2[gone]), bits(acc[gone])) and np.array_equal(bits(m2[gone]), bits(m[gone]))
        assert not np.array_equal(bits(acc2[~gone]), bits(acc[~gone]))
        retire()  # from frame 0: as the first time
        assert np.array_equal(bits(r.accum()), bits(want["history"][0][0]))


# ------------------------------------------------------------------ 7. errors
def test_error_paths():
    name, w, h = "c2", 33, 31
    integ, mb, tris, nodes, hdr, eye, rot = case(name)
    with renderer(name, w, h, moments=True) as plain:
        plain.render_frames(eye, rot, 0, EVERY)
        assert rc_of(plain.adaptive_update) == INVALID
        assert rc_of(plain.adaptive_status) == INVALID
        assert rc_of(plain.tile_error) == INVALID
    assert rc_of(Renderer, w, h, integ, flags=FLAG_ADAPTIVE) == INVALID                                  # no moments
    assert rc_of(Renderer, w, h, integ, flags=FLAG_ADAPTIVE | FLAG_MOMENTS | FLAG_NO_BINS) == INVALID
    assert rc_of(Renderer, w, h, integ, flags=FLAG_NO_BINS, adaptive=True) == INVALID
    assert rc_of(Renderer, w, h, integ, adaptive=True, tile_world=2) == INVALID                          # as moments
    with renderer(name, w, h, adaptive=True) as r:
        assert rc_of(r.adaptive_update) == INVALID  # before any frame
        r.render_frames(eye, rot, 0, EVERY)
        for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")),
                    dict(threshold=float("inf")), dict(limit=0.0), dict(limit=-1.5), dict(min_frames=1),
                    dict(min_frames=0)):
            assert rc_of(r.adaptive_update, **bad) == INVALID, bad
        with pytest.raises(TypeError):
            r.adaptive_update(sigma=1.0)
        assert r._lib.pt_adaptive_status(r._h, None) == INVALID
        assert r._lib.pt_last_error(r._h)
        assert r.adaptive_status().frames == 0  # the failed calls decided nothing
        # the planes into device memory, each alone
        import torch
        e_d = torch.zeros(r.adaptive_status().tiles, dtype=torch.float32, device="cuda:0")
        a_d = torch.zeros(r.adaptive_status().tiles, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        r.adaptive_update(**PRM)
        import ctypes as C
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        r._ck(r._lib.pt_download_tile_error(r._h, C.cast(C.c_void_p(e_d.data_ptr()), fp), None), "tile_error")
        r._ck(r._lib.pt_download_tile_error(r._h, None, C.cast(C.c_void_p(a_d.data_ptr()), up)), "tile_error")
        r._ck(r._lib.pt_download_tile_error(r._h, None, None), "tile_error")
        e, at = r.tile_error()
        assert np.array_equal(bits(e_d.cpu().numpy()), bits(e.reshape(-1)))
        assert np.array_equal(a_d.cpu().numpy().view(np.uint32), at.reshape(-1))


# ------------------------------------------------------------------ 8. the filters still serve it
def test_the_filters_still_serve_it():
    name, w, h = "c4", 33, 31
    *_, eye, rot = case(name)
    want = ar.run(samples(name, w, h), EVERY, PRM)
    with renderer(name, w, h, adaptive=True) as r:
        standard_run(r, eye, rot)
        r.render_guides(eye, rot)
        g = r.guides()
        acc, m = r.accum(), r.moments()
        assert np.array_equal(bits(acc), bits(want["acc"]))
        got = r.denoise_var()
        assert np.array_equal(bits(got), bits(vr.denoise_var(acc, g, m, frames=FRAMES)))
        img = device_plane(h, w, "uint8")
        r.display_denoised(img.data_ptr(), 1.5, 0.0)
        r.synchronize()
        assert np.all(img.cpu().numpy()[..., 3] == 255)
