"""The display post-processing on the GPU fed pixels that are not finite, or extreme: NaN, +-Inf, a
luminance that overflows, a negative, -0.0 and a denormal (tests/nonfinite_planes.py), through
pt_denoise, pt_denoise_var, the sample moments, pt_adaptive_update, pt_temporal_resolve, pt_tonemap,
the 8-bit display forms and the screen-tile gather -- each against its float32 restatement
(denoise_ref, variance_ref, adaptive_ref, temporal_ref, post_common._unorm8), equal bit for bit with
a NaN equal to any NaN (post_common.same: a NaN's sign and payload differ between the host and the
GPU; infinities, signed zeros and denormals still compare by bits). tests/test_nonfinite_ref.py pins
on the CPU what the restatements themselves do with such pixels.

The frame kernels do produce such pixels: MIS divides by the pdf of a black texel
(tests/test_gpu_env.py). Cases c, d and the second half of g render them (c2's mesh under
env_maps.black_rows_map(40, 20, 23), MIS at 2 bounces, 64 x 40, 2 frames: 8.8 % of the pixels are NaN);
the others upload a crafted plane, whose special pixels are placed by the camera's guide planes.
"""
import functools

import numpy as np
import pytest

import adaptive_ref as ar
import denoise_ref as dr
import env_maps
import fmath_sets as fs
import nonfinite_planes as nf
import oracle
import temporal_ref as tr
import variance_ref as vr
from post_common import _unorm8, bits, config, device_plane, same
from opengl_ray_tracing_amd import Renderer, orbit_camera
from opengl_ray_tracing_amd import distributed as D
from opengl_ray_tracing_amd.renderer import FLAG_MEGAKERNEL
from test_gpu_denoise import TERMS_OFF
from test_gpu_variance import TERMS_OFF as VAR_TERMS_OFF

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES = 2
KERNELS = pytest.mark.parametrize("flags", [0, FLAG_MEGAKERNEL], ids=["default", "megakernel"])
SIZES = pytest.mark.parametrize("w,h", nf.SIZES)


def renderer(w, h, **kw):
    cfg, tris, nodes, hdr, _, _ = config("c2")
    r = Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


def camera(delta=0.0):
    angle, up, rad = config("c2")[0].camera
    return orbit_camera(angle + delta, up, rad)


def readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def crafted(w, h):
    """c2's camera at w x h, once per size: (the finite 2-frame mean, the crafted plane, the guide
    planes, craft's record), not modified."""
    *_, eye, rot = config("c2")
    with renderer(w, h) as r:
        for f in range(FRAMES):
            r.render_frame(eye, rot, f)
        base = r.accum()
        r.render_guides(eye, rot)
        g = r.guides()
    c, rec = nf.craft(base, g)  # asserts hits and misses and every placement
    readonly(base, c, *g.values())
    return base, c, g, rec


def on_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).to("cuda:0")
    torch.cuda.synchronize()  # the copy (torch's stream) before the renderer's stream reads it
    return t


def assert_same(got, want, what):
    ok = same(got, want)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())


def assert_guides(r, g):
    got = r.guides()
    for k in ("pos_t", "nrm_tri", "albedo"):
        assert np.array_equal(bits(got[k]), bits(g[k])), k


# ------------------------------------------------------------------ a. pt_denoise
@SIZES
def test_denoise_equals_the_restatement(w, h):
    """The crafted plane as the accumulation and as a caller's device plane: 1, 3 and 5 passes (the
    staged passes of stride <= 2 and the direct ones) and each term off in turn. With the colour term
    on a non-finite pixel keeps its centre and stops its neighbours' sums; with it off the NaN spreads."""
    *_, eye, rot = config("c2")
    base, c, g, rec = crafted(w, h)
    cases = [dict(passes=p) for p in (1, 3, 5)] + TERMS_OFF
    want = [dr.atrous(c, g, **{**dr.DEFAULTS, **prm}) for prm in cases]
    hit, bad = dr.hit_mask(g), nf.nonfinite(c)
    assert same(want[2][bad], c[bad]).all() and not nf.nonfinite(want[2])[~bad].any()  # defaults: kept, contained
    assert nf.nonfinite(want[3])[hit].sum() > hit.sum() // 2                           # sigma_c = 0: spread
    src = on_device(c)
    with renderer(w, h) as r:
        r.render_guides(eye, rot)
        assert_guides(r, g)
        r.set_accum(c)
        for prm, x in zip(cases, want):
            assert_same(r.denoise(**prm), x, ("accumulation", prm))
        assert_same(r.accum(), c, "the accumulation is untouched")
        r.set_accum(base)
        for prm, x in zip(cases, want):
            assert_same(r.denoise(src_dptr=src.data_ptr(), **prm), x, ("device plane", prm))


# ------------------------------------------------------------------ b. pt_denoise_var, spatial
@SIZES
def test_denoise_var_spatial_equals_the_restatement(w, h):
    """A context without moments: the 7 x 7 variance estimate (0 where the window holds a NaN
    luminance) and the filter, with the defaults and each term off in turn."""
    *_, eye, rot = config("c2")
    base, c, g, rec = crafted(w, h)
    with renderer(w, h) as r:
        r.render_guides(eye, rot)
        r.set_accum(c)
        for prm in [dict()] + VAR_TERMS_OFF:
            want, v0 = vr.denoise_var(c, g, None, 0, **{**vr.DEFAULTS, **prm}, with_variance=True)
            got = r.denoise_var(**prm)
            assert_same(r.variance(), v0, ("variance", prm))
            assert_same(got, want, prm)
    hit = dr.hit_mask(g)
    with np.errstate(all="ignore"):
        window = nf._grow(hit & np.isnan(vr.lum_tm(c, 1.5)), 3) & hit
    assert window.sum() > 50 and not bits(v0[window]).any() and (v0[hit & ~window] > 0).any()


# ------------------------------------------------------------------ c, d: rendered NaN samples
W, H, NS = 64, 40, 4  # the frames of c: FRAMES; d renders NS


@functools.lru_cache(maxsize=None)
def black_rows():
    """c2's mesh under the map with black rows: (tris, nodes, hdr, eye, rot, the oracle's samples
    0 .. NS-1 of MIS at 2 bounces, 64 x 40), computed once."""
    cfg, tris, nodes, _, eye, rot = config("c2")
    hdr = env_maps.black_rows_map(40, 20, 23)
    orc = oracle.Oracle(tris, nodes, hdr)
    s = [orc.render(W, H, "mis", 0, eye, rot, accum=np.zeros((H, W, 4), F), max_bounce=2, sample_rank=k,
                    sample_world=NS)[0] for k in range(NS)]
    readonly(*s)
    return tris, nodes, hdr, eye, rot, tuple(s)


@functools.lru_cache(maxsize=None)
def black_rows_fold():
    """The oracle's first FRAMES samples folded -> (running mean, moments): at least 5 % of the pixels
    non-finite and at least 5 % finite, checked here on the oracle alone."""
    s = black_rows()[5]
    acc, m = np.zeros((H, W, 4), F), np.zeros((H, W, 2), F)
    for k in range(FRAMES):
        acc, m = vr.mix_sample(acc, s[k], k), vr.moments_update(m, s[k], k)
    share = float(nf.nonfinite(acc).mean())
    print(f"black rows 40x20, {FRAMES} frames: {share:.3f} of the pixels are non-finite")
    assert 0.05 <= share <= 0.95
    assert np.array_equal(nf.nonfinite(acc), ~np.isfinite(m).all(-1))
    return readonly(acc, m)


def mis_renderer(**kw):
    tris, nodes, hdr, *_ = black_rows()
    r = Renderer(W, H, "mis", max_bounce=2, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


@KERNELS
def test_moments_of_nan_samples_equal_the_restatement(flags):
    """Single render_frame calls, then one render_frames batch: the accumulation and the moments of
    the oracle's samples; then pt_denoise_var from those moments (min_temporal = the frame count)."""
    *_, eye, rot, s = black_rows()
    want_acc, want_m = black_rows_fold()
    with mis_renderer(flags=flags, moments=True) as r:
        for f in range(FRAMES):
            r.render_frame(eye, rot, f)
        assert r.moments_frames() == FRAMES
        assert_same(r.accum(), want_acc, "calls, accumulation")
        assert_same(r.moments(), want_m, "calls, moments")
        r.render_frames(eye, rot, 0, FRAMES)
        assert r.moments_frames() == FRAMES
        acc, m = r.accum(), r.moments()
        assert_same(acc, want_acc, "batch, accumulation")
        assert_same(m, want_m, "batch, moments")
        r.render_guides(eye, rot)
        g = r.guides()
        hit = dr.hit_mask(g)
        assert (nf.nonfinite(acc) & hit).sum() > 50 and (~nf.nonfinite(acc) & hit).sum() > 50
        for prm in (dict(min_temporal=FRAMES), dict(min_temporal=FRAMES, sigma_l=0.0)):
            want, v0 = vr.denoise_var(acc, g, m, FRAMES, **{**vr.DEFAULTS, **prm}, with_variance=True)
            got = r.denoise_var(**prm)
            assert_same(r.variance(), v0, ("variance", prm))
            assert_same(got, want, prm)
        assert not np.array_equal(bits(v0), bits(vr.initial_variance(acc, g, None, 0)))  # the moments were used


PRM = dict(threshold=0.2, limit=1.5, min_frames=FRAMES)


@KERNELS
def test_adaptive_on_nan_samples_equals_the_restatement(flags):
    """2 frames, an update (threshold 0.2, min_frames 2), 2 more frames in one batch. A tile whose
    every pixel is a NaN has err2 = 0 and retires; a tile with some NaN pixels is decided by the others."""
    *_, eye, rot, s = black_rows()
    want = ar.run(s, FRAMES, PRM, updates_at=[FRAMES])
    acc, m, err2, at = want["history"][0]
    tile_bad = np.zeros((8 * at.shape[0], 8 * at.shape[1]), bool)
    tile_bad[:H, :W] = nf.nonfinite(acc)
    tile_bad = tile_bad.reshape(at.shape[0], 8, at.shape[1], 8).any(axis=(1, 3))
    print(f"{int((at != 0).sum())} of {at.size} tiles retire, {int(((at != 0) & tile_bad).sum())} of them and "
          f"{int(((at == 0) & tile_bad).sum())} of the active ones hold a non-finite pixel")
    assert ((at != 0) & tile_bad).any() and (at == 0).any() and ((at == 0) & tile_bad).any()
    with mis_renderer(flags=flags, adaptive=True) as r:
        r.render_frames(eye, rot, 0, FRAMES)
        r.adaptive_update(**PRM)
        e, a = r.tile_error()
        assert np.array_equal(bits(e), bits(err2))
        assert np.array_equal(a, at)
        st = r.adaptive_status()
        assert (st.tiles, st.retired, st.frames) == (at.size, want["counts"][0], FRAMES), st
        assert np.array_equal(bits(F(st.max_err2)), bits(want["max_err2"][0])), st
        assert_same(r.accum(), acc, "accumulation at the update")
        assert_same(r.moments(), m, "moments at the update")
        r.render_frames(eye, rot, FRAMES, NS - FRAMES)
        assert r.moments_frames() == NS
        assert_same(r.accum(), want["acc"], "accumulation after the batch")
        assert_same(r.moments(), want["m"], "moments after the batch")
    gone = ar.pixel_mask(at, H, W)
    assert not same(want["acc"], acc)[~gone].all()  # the active pixels went on


# ------------------------------------------------------------------ e. pt_temporal_resolve
@functools.lru_cache(maxsize=None)
def poked(w, h):
    """Camera B's finite mean (2 degrees on) with one NaN and one Inf pixel of its own, on hits, once
    per size -> (plane, guides), not modified."""
    eyeB, rotB = camera(2.0)
    with renderer(w, h) as r:
        for f in range(FRAMES):
            r.render_frame(eyeB, rotB, f)
        acc = r.accum()
        r.render_guides(eyeB, rotB)
        g = r.guides()
    ys, xs = np.nonzero(dr.hit_mask(g))
    k = len(ys) // 3
    acc[ys[k], xs[k], 0:3] = np.nan
    acc[ys[2 * k], xs[2 * k], 1] = np.inf
    readonly(acc, *g.values())
    return acc, g


def temporal_steps(r, w, h, c, g):
    """set_accum(crafted), guides, resolve, commit; then camera B's poked mean and its guides, ready
    for a resolve -> (the first resolve, its restatement, B's plane, B's guides, the history)."""
    eyeA, rotA = camera()
    eyeB, rotB = camera(2.0)
    accB, gB = poked(w, h)
    r.set_accum(c)
    r.render_guides(eyeA, rotA)
    got0 = r.temporal_resolve(FRAMES)
    want0 = tr.resolve(c, FRAMES, g, None)
    r.temporal_commit()
    hist = tr.commit(want0, g, eyeA, rotA)
    r.set_accum(accB)
    r.render_guides(eyeB, rotB)
    return got0, want0, accB, gB, hist


@SIZES
def test_temporal_resolve_equals_the_restatement(w, h):
    """The crafted plane as the history of camera A, camera B's mean with a NaN and an Inf pixel of its
    own: the defaults and max_history = 1. A history NaN reaches the pixels whose valid taps hold it,
    also with weight 0, and no pixel beside them."""
    base, c, g, rec = crafted(w, h)
    with renderer(w, h) as r:
        got0, want0, accB, gB, hist = temporal_steps(r, w, h, c, g)
        assert_same(got0, want0, "no history")
        assert_guides(r, gB)
        for prm in (dict(), dict(max_history=1.0)):
            want = tr.resolve(accB, FRAMES, gB, hist, **{**tr.DEFAULTS, **prm})
            took = dr.hit_mask(gB) & (want[..., 3] > FRAMES)
            from_hist = took & nf.nonfinite(want) & ~nf.nonfinite(accB)
            clean = took & ~nf.nonfinite(want)
            print(f"{w}x{h} {prm}: {int(took.sum())} pixels take history, {int(from_hist.sum())} a non-finite one")
            assert from_hist.sum() >= 10 and (nf._grow(from_hist, 1) & clean).sum() >= 10
            assert (nf.nonfinite(want) & nf.nonfinite(accB)).sum() == 2
            assert_same(r.temporal_resolve(FRAMES, **prm), want, prm)


# ------------------------------------------------------------------ f. pt_tonemap and the 8-bit forms
def tonemap_host(c, gamma):
    """pt_tonemap on the host: denoise_ref.tm, then ptm_powf(x, 1 / gamma) through pt_fmath_host."""
    t = dr.tm(c, 1.5)
    if gamma > 0:
        t = fs.host(6, t, np.full(t.shape, F(1) / F(gamma), F)).reshape(t.shape)
    return t


@pytest.mark.parametrize("gamma", [0.0, 2.2])
@SIZES
def test_tonemap_and_the_8bit_forms(w, h, gamma):
    """The crafted plane, its filtered image and a resolved image with a non-finite history:
    pt_tonemap against the host's, the four display forms against _unorm8 of it, alpha 255. A byte
    comes from a NaN (0), from +Inf (tm(Inf) is a NaN: 0), from a negative (0), from a value above 1
    (255) and from ordinary values."""
    import torch
    *_, eye, rot = config("c2")
    base, c, g, rec = crafted(w, h)
    img = device_plane(h, w, "uint8")
    px, py, valid = D.packed_coords(w, h, 0, 1)
    packed = torch.zeros(3 * px.size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()  # the fill (torch's stream) before the renderer's stream writes it

    def check_accum(r, a, what):
        """`a` is the context's accumulation: pt_tonemap, pt_display_own and pt_display_pack of it."""
        t = tonemap_host(a, gamma)
        assert_same(r.tonemap(1.5, gamma), t, (what, "tonemap"))
        r.display_own(img.data_ptr(), 1.5, gamma)
        r.display_pack(packed.data_ptr(), 1.5, gamma)
        r.synchronize()
        got = img.cpu().numpy()
        assert np.array_equal(got[..., :3], _unorm8(t)) and np.all(got[..., 3] == 255), (what, "display_own")
        slots = packed.cpu().numpy().reshape(-1, 3)
        assert np.array_equal(slots[valid], _unorm8(t)[py[valid], px[valid]]), (what, "display_pack")
        assert not slots[~valid].any()
        return t

    with renderer(w, h) as r:
        r.set_accum(c)
        t = check_accum(r, c, "crafted")
        with np.errstate(invalid="ignore"):
            tm = dr.tm(c, 1.5)
            assert np.isnan(tm[..., 0][np.isposinf(c[..., 0])]).all() and np.isposinf(c[..., 0]).any()
            assert np.isnan(c[..., 0:3]).any() and (tm < 0).any() and (tm > 1).any() and ((tm > 0) & (tm < 1)).any()
            b = _unorm8(t)
            assert (b[np.isnan(t)] == 0).all() and (b[t < 0] == 0).all() and (b[t > 1] == 255).all()
        assert len(np.unique(b)) > 100
        # the filtered image, through pt_display_denoised and as an accumulation
        r.render_guides(eye, rot)
        den = r.denoise(sigma_c=0.0, passes=2)  # the NaN spread a little, the rest is filtered
        assert nf.nonfinite(den).sum() > nf.nonfinite(c).sum() and not nf.nonfinite(den).all()
        r.display_denoised(img.data_ptr(), 1.5, gamma)
        r.synchronize()
        got = img.cpu().numpy()
        assert np.array_equal(got[..., :3], _unorm8(tonemap_host(den, gamma))) and np.all(got[..., 3] == 255)
        r.set_accum(den)
        check_accum(r, den, "filtered")
        # the resolved image, through pt_display_resolved and as an accumulation
        got0, want0, accB, gB, hist = temporal_steps(r, w, h, c, g)
        res = r.temporal_resolve(FRAMES)
        assert nf.nonfinite(res).sum() > 10 and not nf.nonfinite(res).all()
        r.display_resolved(img.data_ptr(), 1.5, gamma)
        r.synchronize()
        got = img.cpu().numpy()
        assert np.array_equal(got[..., :3], _unorm8(tonemap_host(res, gamma))) and np.all(got[..., 3] == 255)
        r.set_accum(res)
        check_accum(r, res, "resolved")


# ------------------------------------------------------------------ g. the gather keeps bits
PAYLOADS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001], np.uint32)


def payload_plane(w, h):
    """A finite plane, alpha 1, where every third pixel holds one of: three NaNs with payloads (a
    quiet one, a negative one, a signalling one) and the seven special values, in one channel."""
    c = np.ones((h, w, 4), F)
    c[..., 0:3] = np.random.default_rng(w * h).uniform(0.0, 4.0, (h, w, 3))
    words = np.concatenate([PAYLOADS, np.array([v for _, v in nf.SPECIALS], F).view(np.uint32)])
    u = c.view(np.uint32)
    y, x = np.nonzero(np.add.outer(np.arange(h), np.arange(w)) % 3 == 0)  # a diagonal pattern: every column has some
    k = np.arange(y.size)
    u[y, x, k % 3] = words[k % len(words)]
    return c


@SIZES
def test_the_gather_keeps_every_bit(w, h):
    """set_accum -> accum, and pack_owned -> unpack_ranks between two tile_world = 2 contexts of one
    device: NaN payloads, infinities, -0.0 and the denormal come back bit for bit, alpha 1."""
    import torch
    c = payload_plane(w, h)
    world = 2
    ranks = [renderer(w, h, tile_rank=k, tile_world=world) for k in range(world)]
    try:
        ranks[1].set_accum(c)
        assert np.array_equal(bits(ranks[1].accum()), bits(c))
        buf = torch.zeros((ranks[1].owned_pixel_count(), 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()  # the fill (torch's stream) before the renderer's stream writes it
        ranks[1].pack_owned(buf.data_ptr())
        ranks[1].synchronize()
        want = D.pack(c, 1, world)[:, :3]
        assert np.array_equal(bits(buf.cpu().numpy()), bits(want))
        zero = np.zeros((h, w, 4), F)
        ranks[0].set_accum(zero)
        ranks[0].unpack_ranks(world, [0, buf.data_ptr()])
        got = ranks[0].accum()
    finally:
        for r in ranks:
            r.close()
    own = D.owned_pixels(w, h, 1, world)
    mine = np.zeros((h, w), bool)
    mine[own[:, 1], own[:, 0]] = True
    assert mine.any() and not mine.all()
    assert np.array_equal(bits(got[mine][:, :3]), bits(c[mine][:, :3])) and np.all(got[mine][:, 3] == 1)
    assert not got[~mine].any()
    for word in PAYLOADS:
        assert (bits(got[mine]) == word).any(), hex(word)


@pytest.mark.parametrize("shard", [8, 32])
def test_the_stats_gather_keeps_nan_moments(shard):
    """Two share_moments ranks render the black-rows frames of c; pack_owned_stats -> unpack_ranks_stats
    gives rank 0 the whole mean and moments: the oracle's fold, and each rank's own words bit for bit."""
    import torch
    *_, eye, rot, s = black_rows()
    want_acc, want_m = black_rows_fold()
    world = 2
    ranks = [mis_renderer(moments=True, share_moments=True, tile_rank=k, tile_world=world, tile_size=shard)
             for k in range(world)]
    try:
        own, bufs = [], []
        for k, r in enumerate(ranks):
            r.render_frames(eye, rot, 0, FRAMES)
            own.append(np.concatenate([r.accum()[..., :3], r.moments()], -1))
            t = torch.zeros((r.owned_pixel_count(), 5), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()  # the fill (torch's stream) before the renderer's stream writes it
            r.pack_owned_stats(t.data_ptr())
            r.synchronize()
            assert np.array_equal(bits(t.cpu().numpy()), bits(D.pack(own[k], k, world, shard))), k
            bufs.append(t)
        ranks[0].unpack_ranks_stats(world, [0, bufs[1].data_ptr()])
        acc, m = ranks[0].accum(), ranks[0].moments()
    finally:
        for r in ranks:
            r.close()
    assert_same(acc, want_acc, "gathered accumulation")
    assert_same(m, want_m, "gathered moments")
    px = D.owned_pixels(W, H, 1, world, shard)
    mine = np.zeros((H, W), bool)
    mine[px[:, 1], px[:, 0]] = True
    got = np.concatenate([acc[..., :3], m], -1)
    assert np.isnan(got[mine]).any() and np.isnan(got[~mine]).any()
    for k, mask in enumerate((~mine, mine)):
        assert np.array_equal(bits(got[mask]), bits(own[k][mask])), k
