"""The per-pixel sample moments and the variance-guided a-trous filter on the GPU (PT_FLAG_MOMENTS,
pt_download_moments, pt_denoise_var, pt_download_variance) against the float32 restatement
tests/variance_ref.py, bit for bit: the moments of the oracle's samples through every frame kernel
and both calling patterns with the accumulation a plain context's, the validity count, the variance
estimate (spatial and from the moments) and the filter at sizes from one pixel to several
workgroups with LDS-staged and direct passes, everything else left untouched, the 8-bit display,
the quality gates and the error paths.

Reference: Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017); IS pass1.fsh:868-871
(the running mean whose weights the moments share); pass3.fsh:14-24 (tonemap and display).
"""
import functools

import numpy as np
import pytest

import denoise_ref as dr
import oracle
import variance_ref as vr
from post_common import INVALID, NOSCENE, _unorm8, bits, config, device_plane, rc_of
from opengl_ray_tracing_amd import Renderer, scenes
from opengl_ray_tracing_amd.renderer import FLAG_COUNT_FETCHES, FLAG_MEGAKERNEL, FLAG_SERIAL_FRAMES

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (5, 3), (33, 31), (100, 76)]
N = 7
TERMS_OFF = [dict(sigma_l=0.0), dict(sigma_z=0.0), dict(sigma_a=0.0), dict(normal_log2=-1)]


def renderer(name, w, h, **kw):
    cfg, tris, nodes, hdr, _, _ = config(name)
    r = Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


@functools.lru_cache(maxsize=None)
def oracle_moments(name, w, h):
    """The oracle's N samples of a config (sample k alone: frame 0 of sample rank k of N), folded:
    -> (running mean, moments), computed once per case and not modified."""
    cfg, tris, nodes, hdr, eye, rot = config(name)
    orc = oracle.Oracle(tris, nodes, hdr)
    acc = np.zeros((h, w, 4), F)
    m = np.zeros((h, w, 2), F)
    for k in range(N):
        s, _ = orc.render(w, h, cfg.integrator, 0, eye, rot, accum=np.zeros((h, w, 4), F),
                          max_bounce=cfg.max_bounce, sample_rank=k, sample_world=N)
        acc = vr.mix_sample(acc, s, k)
        m = vr.moments_update(m, s, k)
    acc.setflags(write=False)
    m.setflags(write=False)
    return acc, m


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name,flags", [("c2", 0), ("c2", FLAG_MEGAKERNEL), ("c4", 0)],
                         ids=["c2-regen", "c2-megakernel", "c4-mis"])
def test_moments_equal_the_restatement(name, flags, w, h):
    """7 single render_frame calls (each would otherwise mix inside the frame kernel) and
    render_frames(0, 7) (frame 0 alone, then a batch): the moments of the oracle's samples bit for
    bit, 7 frames counted, and the accumulation a plain context's (and the oracle's) bit for bit."""
    cfg, tris, nodes, hdr, eye, rot = config(name)
    want_acc, want_m = oracle_moments(name, w, h)
    with renderer(name, w, h, flags=flags, moments=True) as r, renderer(name, w, h, flags=flags) as plain:
        assert r.moments_frames() == 0 and not r.moments().any()
        assert plain.moments_frames() == 0
        for f in range(N):
            r.render_frame(eye, rot, f)
            plain.render_frame(eye, rot, f)
            assert r.moments_frames() == f + 1
        acc = r.accum()
        assert np.array_equal(bits(acc), bits(plain.accum()))
        assert np.array_equal(bits(acc), bits(want_acc))
        assert np.array_equal(bits(r.moments()), bits(want_m))
        r.render_frames(eye, rot, 0, N)
        plain.render_frames(eye, rot, 0, N)
        assert r.moments_frames() == N
        acc = r.accum()
        assert np.array_equal(bits(acc), bits(plain.accum()))
        assert np.array_equal(bits(acc), bits(want_acc))
        assert np.array_equal(bits(r.moments()), bits(want_m))
        assert plain.moments_frames() == 0


def test_validity_counting():
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h = 33, 31
    with renderer("c2", w, h, moments=True) as r:
        def restart(n=3):
            r.render_frames(eye, rot, 0, n)
            assert r.moments_frames() == n
        restart()
        r.render_frame(eye, rot, 3)
        assert r.moments_frames() == 4
        r.render_frame(eye, rot, 6)  # a gap
        assert r.moments_frames() == 0
        r.render_frame(eye, rot, 7)  # stays invalid until a restart
        assert r.moments_frames() == 0
        restart()
        r.render_frame(eye, rot, 1)  # a step back
        assert r.moments_frames() == 0
        restart()
        r.set_accum(r.accum())
        assert r.moments_frames() == 0
        restart()
        r.clear()
        assert r.moments_frames() == 0 and not r.moments().any() and not r.accum().any()
        restart()
        r.upload_scene(tris, nodes)
        assert r.moments_frames() == 0
        restart()
        r.upload_env(hdr)
        assert r.moments_frames() == 0
        restart(N)
        assert np.array_equal(bits(r.moments()), bits(oracle_moments("c2", w, h)[1]))


# ------------------------------------------------------------------ the variance and the filter
def check_filter(r, c, g, m, frames, passes_list, src=None):
    for passes in passes_list:
        got = r.denoise_var(passes=passes, src_dptr=src)
        want, v0 = vr.denoise_var(c, g, m, frames, **{**vr.DEFAULTS, "passes": passes}, with_variance=True)
        assert np.array_equal(bits(r.variance()), bits(v0)), (frames, passes)
        assert np.array_equal(bits(got), bits(want)), (frames, passes)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["c4", "c2"])
def test_variance_and_filter_equal_the_restatement(name, w, h):
    """At 2 frames (the spatial estimate) and at 9 (from the moments), 1, 3 and 5 passes (8 at
    33x31); at 9 frames each term off in turn and the defaults into a caller's buffer, a min_temporal
    above the frame count (spatial again), and a resolved image whose count exceeds the frames (n_p).
    100x76 is no multiple of the 16-pixel tile and has interior LDS tiles; passes of stride >= 4
    take the direct-load kernel. The accumulation, the moments and pt_denoise's image stay as they were."""
    cfg, tris, nodes, hdr, eye, rot = config(name)
    passes_list = [1, 3, 5] + ([8] if (w, h) == (33, 31) else [])
    with renderer(name, w, h, moments=True) as r:
        r.render_guides(eye, rot)
        g = r.guides()
        r.render_frames(eye, rot, 0, 2)
        acc, m = r.accum(), r.moments()
        check_filter(r, acc, g, m, 2, passes_list)
        r.render_frames(eye, rot, 2, 7)
        assert r.moments_frames() == 9
        acc, m = r.accum(), r.moments()
        plain_denoised = r.denoise()
        check_filter(r, acc, g, m, 9, passes_list)
        if dr.hit_mask(g).any():
            spatial = vr.initial_variance(acc, g, None, 0)
            assert not np.array_equal(r.variance(), spatial)  # the moments were used
        out = device_plane(h, w)
        for prm in TERMS_OFF + [dict(passes=3), dict(min_temporal=10), dict(min_temporal=9)]:
            assert r.denoise_var(out.data_ptr(), **prm) is None
            r.synchronize()
            assert r.denoised_device_ptr() == out.data_ptr()
            want, v0 = vr.denoise_var(acc, g, m, 9, **{**vr.DEFAULTS, **prm}, with_variance=True)
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), prm
            assert np.array_equal(bits(r.variance()), bits(v0)), prm
        # a resolved image (no history: the accumulation's rgb) that claims 20 samples
        resolved = r.temporal_resolve(20)
        assert np.all(resolved[..., 3] == 20)
        check_filter(r, resolved, g, m, 9, [3], src=r.resolved_device_ptr())
        assert np.array_equal(bits(r.accum()), bits(acc))
        assert np.array_equal(bits(r.moments()), bits(m)) and r.moments_frames() == 9
        assert np.array_equal(bits(r.denoise()), bits(plain_denoised))


@pytest.mark.parametrize("w,h", [(33, 31), (100, 76)])
def test_filter_without_moments_is_spatial(w, h):
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    with renderer("c2", w, h) as r:
        r.render_guides(eye, rot)
        g = r.guides()
        r.render_frames(eye, rot, 0, 9)
        acc = r.accum()
        check_filter(r, acc, g, None, 0, [1, 5])
        assert np.array_equal(bits(r.accum()), bits(acc))


def test_display_denoised_is_pass3_of_the_filtered_image():
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h = 100, 76
    with renderer("c2", w, h, moments=True) as r:
        r.render_frames(eye, rot, 0, 9)
        r.render_guides(eye, rot)
        den = r.denoise_var()
        img = device_plane(h, w, "uint8")
        r.display_denoised(img.data_ptr(), 1.5, 0.0)
        r.synchronize()
        r.set_accum(den)
        t = r.tonemap(1.5, 0.0)
    got = img.cpu().numpy()
    assert np.array_equal(got[..., :3], _unorm8(t)) and np.all(got[..., 3] == 255)


# ------------------------------------------------------------------ quality
@pytest.mark.parametrize("name", ["c4", "c2"])
def test_quality_gates_on_the_gpu(name):
    """tests/test_variance_ref.py's gates (a) and (b) with the GPU's own 4-, 256- and 2048-frame means."""
    cfg, tris, nodes, hdr, eye, rot = config(name)
    w, h = 160, 90
    rows = {}
    with renderer(name, w, h, moments=True) as r:
        r.render_guides(eye, rot)
        mask = r.guides()["tri"] >= 0
        done = 0
        for k in (4, 256):
            r.render_frames(eye, rot, done, k - done)
            done = k
            assert r.moments_frames() == k
            rows[k] = (r.accum(), r.denoise(), r.denoise_var())
        r.render_frames(eye, rot, done, 2048 - done)
        clean = r.accum()
    p = {k: [dr.psnr_tm(x, clean, mask) for x in v] for k, v in rows.items()}
    for k, (raw, atrous, var) in p.items():
        print(f"{name}, {k:3d} frames: raw {raw:.2f} dB | pt_denoise {atrous:.2f} | pt_denoise_var {var:.2f}")
    assert p[4][2] - p[4][0] >= 2.0, (name, p)
    assert p[256][2] >= p[256][0], (name, p)
    assert p[256][2] >= p[256][1] + 2.0, (name, p)


# ------------------------------------------------------------------ errors
def test_create_rejects_the_forbidden_combinations():
    for kw in (dict(integrator="basic"), dict(flags=FLAG_COUNT_FETCHES), dict(flags=FLAG_SERIAL_FRAMES),
               dict(tile_world=2), dict(tile_world=2, tile_rank=1), dict(devices=[0, 0])):
        kw = {"integrator": "lambert", **kw}
        assert rc_of(Renderer, 32, 32, moments=True, **kw) == INVALID, kw
    with Renderer(32, 32, "lambert", moments=True, sample_rank=1, sample_world=2) as r:  # allowed
        assert r.moments_frames() == 0


def test_error_paths():
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h = 33, 31
    with Renderer(w, h, "lambert") as r:
        assert rc_of(r.moments) == INVALID
        assert rc_of(r.moments_device_ptr) == INVALID
        assert rc_of(r.denoise_var) == NOSCENE
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        r.render_frame(eye, rot, 0)
        assert rc_of(r.denoise_var) == INVALID  # before any render_guides
        assert rc_of(r.variance) == INVALID     # before any denoise_var
        r.render_guides(eye, rot)
        for bad in (dict(passes=0), dict(passes=9), dict(normal_log2=-2), dict(normal_log2=11), dict(limit=0.0),
                    dict(limit=-1.0), dict(min_temporal=1), dict(min_temporal=0)):
            assert rc_of(r.denoise_var, **bad) == INVALID, bad
        assert rc_of(r.variance) == INVALID  # the failed calls estimated nothing
        assert rc_of(r.denoised_device_ptr) == INVALID
        r.denoise_var(passes=2)
        own = r.denoised_device_ptr()
        out = device_plane(h, w)
        assert rc_of(r.denoise_var, src_dptr=own) == INVALID                           # the context's buffer
        assert rc_of(r.denoise_var, out.data_ptr(), src_dptr=out.data_ptr()) == INVALID  # the output
        r.variance()
        r.upload_scene(tris, nodes)  # invalidates the guides
        assert rc_of(r.denoise_var) == INVALID
        r.render_guides(eye, rot)
        r.denoise_var(passes=1)
    with Renderer(32, 32, "basic", basic_samples=1) as b:
        b.upload_shapes(scenes.cornell_shapes())
        assert rc_of(b.denoise_var) == INVALID
        assert rc_of(b.moments) == INVALID
