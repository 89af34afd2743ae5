"""The sample moments and adaptive sampling on a screen-tile split (PT_FLAG_SHARE_MOMENTS,
pt_pack_owned_stats, pt_unpack_ranks_stats, pt_adaptive_update / pt_adaptive_status per share).

Every rank is a context of this one process on the one device, the packed buffers are torch tensors
(as test_gpu_features.test_tile_shards_reassemble_bit_exact). The yardstick is always a one-context
render of the kind the earlier suites tie to the oracle and to variance_ref / adaptive_ref -- a
PT_FLAG_MOMENTS context for the moments, a PT_FLAG_ADAPTIVE context for adaptive sampling -- computed
once per (case, size) and compared bit for bit; never the split itself.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from adaptive_common import EVERY, FRAMES, PRM, case
from post_common import INVALID, bits, rc_of
from opengl_ray_tracing_amd import Renderer, _native
from opengl_ray_tracing_amd import distributed as D
from opengl_ray_tracing_amd.renderer import FLAG_MOMENTS, FLAG_REGEN, FLAG_SHARE_MOMENTS

pytestmark = pytest.mark.gpu

F = np.float32
LAUNCHES = (3, 3, 1, 1)  # the 8 frames of the moments cases
# (case, flags, w, h): c2 the Lambert wide regen kernel, c4 the MIS megakernel, c3 through the narrow Disney regen
CONFIGS = [("c2", 0, 33, 31), ("c2", 0, 100, 76), ("c4", 0, 33, 31), ("c4", 0, 100, 76),
           ("c3-disney", FLAG_REGEN, 33, 31)]
CONFIG_IDS = ["c2-33x31", "c2-100x76", "c4-33x31", "c4-100x76", "c3-disney-narrow-regen-33x31"]
WORLDS = [2, 3, 8]
SHARDS = [8, 32]  # 33x31 in shard tiles of 32 is two tiles: with world 3 (and 8) ranks own nothing


def renderer(name, w, h, **kw):
    integ, mb, tris, nodes, hdr, _, _ = case(name)
    r = Renderer(w, h, integ, max_bounce=mb, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


def split(name, w, h, world, shard, **kw):
    return [renderer(name, w, h, tile_rank=k, tile_world=world, tile_size=shard, share_moments=True, **kw)
            for k in range(world)]


def close(ranks):
    for r in ranks:
        r.close()


def render8(r, eye, rot):
    first = 0
    for n in LAUNCHES:
        r.render_frames(eye, rot, first, n)
        first += n


def pixel_mask(w, h, k, world, shard):
    own = D.owned_pixels(w, h, k, world, shard)
    m = np.zeros((h, w), bool)
    m[own[:, 1], own[:, 0]] = True
    return m


def packed_buffers(ranks, floats, pack):
    """Every rank's pack into a torch tensor of its own (one slot at least: a rank that owns nothing
    still hands the call a buffer)."""
    import torch
    bufs = [torch.zeros((max(r.owned_pixel_count(), 1), floats), dtype=torch.float32, device="cuda:0") for r in ranks]
    torch.cuda.synchronize()  # the fills run on torch's stream, the packs on the renderers'
    for r, t in zip(ranks, bufs):
        pack(r)(t.data_ptr())
        r.synchronize()
    return bufs


def gather_stats(ranks):
    """What FrameGather(moments=True) does around the collective: pack on every rank, unpack on rank 0."""
    bufs = packed_buffers(ranks, 5, lambda r: r.pack_owned_stats)
    ranks[0].unpack_ranks_stats(len(ranks), [0] + [b.data_ptr() for b in bufs[1:]])
    return bufs


# ------------------------------------------------------------------ the yardsticks, once each
@functools.lru_cache(maxsize=None)
def one_context_moments(name, flags, w, h):
    """(accum, moments) of a PT_FLAG_MOMENTS context after the 8 frames."""
    *_, eye, rot = case(name)
    with renderer(name, w, h, flags=flags, moments=True) as r:
        render8(r, eye, rot)
        assert r.moments_frames() == sum(LAUNCHES)
        out = r.accum(), r.moments()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def one_context_adaptive(name, flags, w, h):
    """A PT_FLAG_ADAPTIVE context's 32 frames with an update every 8: per update (err2, retired_at,
    status), and at the end (accum, moments, rays)."""
    *_, eye, rot = case(name)
    updates = []
    with renderer(name, w, h, flags=flags, adaptive=True) as r:
        for k in range(FRAMES // EVERY):
            r.render_frames(eye, rot, k * EVERY, EVERY)
            r.adaptive_update(**PRM)
            updates.append((*r.tile_error(), r.adaptive_status()))
        end = r.accum(), r.moments(), r.stats().rays
    return updates, end


@functools.lru_cache(maxsize=None)
def one_context_filter(name, flags, w, h):
    """(denoise_var's output, its variance plane) of the one-context moments render."""
    *_, eye, rot = case(name)
    with renderer(name, w, h, flags=flags, moments=True) as r:
        render8(r, eye, rot)
        r.render_guides(eye, rot)
        return r.denoise_var(), r.variance()


# ------------------------------------------------------------------ 1. moments
@pytest.mark.parametrize("shard", SHARDS)
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name,flags,w,h", CONFIGS, ids=CONFIG_IDS)
def test_moments_of_a_split_equal_one_context(name, flags, w, h, world, shard):
    *_, eye, rot = case(name)
    acc_ref, m_ref = one_context_moments(name, flags, w, h)
    ranks = split(name, w, h, world, shard, flags=flags, moments=True)
    try:
        for k, r in enumerate(ranks):
            render8(r, eye, rot)
            mine = pixel_mask(w, h, k, world, shard)
            acc, m = r.accum(), r.moments()
            assert np.array_equal(bits(acc[mine]), bits(acc_ref[mine])), k
            assert np.array_equal(bits(m[mine]), bits(m_ref[mine])), k
            assert not acc[~mine].any() and not m[~mine].any(), k
            assert r.moments_frames() == 8, k
        assert any(r.owned_pixel_count() == 0 for r in ranks) == ((w, h, shard) == (33, 31, 32) and world > 2)
        bufs = gather_stats(ranks)
        for k, (r, t) in enumerate(zip(ranks, bufs)):
            n = r.owned_pixel_count()
            assert n == D.packed_count(w, h, k, world, shard)
            got = t.cpu().numpy()[:n]
            assert np.array_equal(bits(got[:, :3]), bits(D.pack(acc_ref, k, world, shard)[:, :3])), k
            assert np.array_equal(bits(got[:, 3:]), bits(D.pack(m_ref, k, world, shard))), k
        assert np.array_equal(bits(ranks[0].accum()), bits(acc_ref))
        assert np.array_equal(bits(ranks[0].moments()), bits(m_ref))
        assert [r.moments_frames() for r in ranks] == [8] * world
        # a plain unpack on a flagged context writes the others' colours and invalidates nothing
        rgb = packed_buffers(ranks, 3, lambda r: r.pack_owned)
        ranks[0].unpack_ranks(world, [0] + [b.data_ptr() for b in rgb[1:]])
        ranks[0].unpack_rank(world - 1, world, rgb[world - 1].data_ptr())
        assert ranks[0].moments_frames() == 8
        assert np.array_equal(bits(ranks[0].moments()), bits(m_ref))
        assert np.array_equal(bits(ranks[0].accum()), bits(acc_ref))
    finally:
        close(ranks)


# ------------------------------------------------------------------ 2. the filter on rank 0
@pytest.mark.parametrize("name,flags,w,h,world,shard", [("c2", 0, 33, 31, 3, 8), ("c4", 0, 100, 76, 2, 32)],
                         ids=["c2-33x31-w3-s8", "c4-100x76-w2-s32"])
def test_rank0_filters_with_the_gathered_moments(name, flags, w, h, world, shard):
    *_, eye, rot = case(name)
    out_ref, var_ref = one_context_filter(name, flags, w, h)
    ranks = split(name, w, h, world, shard, flags=flags, moments=True)
    plain = [renderer(name, w, h, flags=flags, tile_rank=k, tile_world=world, tile_size=shard) for k in range(world)]
    try:
        for r in ranks + plain:
            render8(r, eye, rot)
        gather_stats(ranks)
        ranks[0].render_guides(eye, rot)
        assert np.array_equal(bits(ranks[0].denoise_var()), bits(out_ref))
        assert np.array_equal(bits(ranks[0].variance()), bits(var_ref))
        # the same rank without moments estimates the variance from the 7x7 window: another plane, so the
        # equality above is the moments branch
        rgb = packed_buffers(plain, 3, lambda r: r.pack_owned)
        plain[0].unpack_ranks(world, [0] + [b.data_ptr() for b in rgb[1:]])
        assert np.array_equal(bits(plain[0].accum()), bits(ranks[0].accum()))
        plain[0].render_guides(eye, rot)
        plain[0].denoise_var()
        assert not np.array_equal(bits(plain[0].variance()), bits(var_ref))
    finally:
        close(ranks + plain)


# ------------------------------------------------------------------ 3. adaptive sampling
@pytest.mark.parametrize("shard", SHARDS)
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name,flags,w,h", CONFIGS, ids=CONFIG_IDS)
def test_adaptive_split_equals_one_context(name, flags, w, h, world, shard):
    *_, eye, rot = case(name)
    updates, (acc_ref, m_ref, rays_ref) = one_context_adaptive(name, flags, w, h)
    if (name, w, h) == ("c2", 100, 76):  # part of the image retires and part does not
        assert [u[2].retired for u in updates] == [44, 54, 59, 63] and updates[0][2].tiles == 130
    tiles = [D.owned_image_tiles(w, h, k, world, shard) for k in range(world)]
    ranks = split(name, w, h, world, shard, flags=flags, adaptive=True)
    try:
        for u, (err2_ref, at_ref, st_ref) in enumerate(updates):
            sts, e_sum, a_sum = [], np.zeros_like(err2_ref), np.zeros_like(at_ref)
            for k, r in enumerate(ranks):
                r.render_frames(eye, rot, u * EVERY, EVERY)
                r.adaptive_update(**PRM)
                e, a = r.tile_error()
                assert not e[~tiles[k]].any() and not a[~tiles[k]].any(), (u, k)
                st = r.adaptive_status()
                assert (st.tiles, st.frames) == (int(tiles[k].sum()), (u + 1) * EVERY), (u, k, st)
                assert st.retired == int(np.count_nonzero(a)), (u, k, st)
                sts.append(st)
                e_sum, a_sum = e_sum + e, a_sum + a  # disjoint support: x + 0
            assert np.array_equal(bits(e_sum), bits(err2_ref)), u
            assert np.array_equal(a_sum, at_ref), u
            assert sum(s.tiles for s in sts) == st_ref.tiles and sum(s.retired for s in sts) == st_ref.retired, u
            assert np.array_equal(bits(F(max(s.max_err2 for s in sts))), bits(F(st_ref.max_err2))), u
            # rank 0 unpacks after every batch: its retired tiles stay retired
            before = ranks[0].tile_error()[1]
            gather_stats(ranks)
            assert np.array_equal(ranks[0].tile_error()[1], before), u
            assert ranks[0].adaptive_status().retired == sts[0].retired and ranks[0].moments_frames() == (u + 1) * EVERY
        assert np.array_equal(bits(ranks[0].accum()), bits(acc_ref))
        assert np.array_equal(bits(ranks[0].moments()), bits(m_ref))
        rays = [r.stats().rays for r in ranks]
        assert sum(rays) == rays_ref
        for k, r in enumerate(ranks):  # a rank that owns nothing: no tile, no ray
            if r.owned_pixel_count() == 0:
                assert rays[k] == 0 and r.adaptive_status().tiles == 0
    finally:
        close(ranks)


def test_restart_and_invalidation_on_a_share():
    name, w, h, world, shard = "c2", 33, 31, 2, 8
    integ, mb, tris, nodes, hdr, eye, rot = case(name)
    updates, _ = one_context_adaptive(name, 0, w, h)
    at_ref = updates[0][1]
    assert np.count_nonzero(at_ref) > 0
    ranks = split(name, w, h, world, shard, adaptive=True)
    try:
        for k, r in enumerate(ranks):
            mine = D.owned_image_tiles(w, h, k, world, shard)
            want = np.where(mine, at_ref, 0)

            def retire():
                r.render_frames(eye, rot, 0, EVERY)
                r.adaptive_update(**PRM)
                assert np.array_equal(r.tile_error()[1], want)
                assert r.adaptive_status().frames == EVERY

            def cleared():
                st = r.adaptive_status()
                e, at = r.tile_error()
                assert st.retired == 0 and st.frames == 0 and st.max_err2 == 0.0 and not at.any() and not e.any()
                assert st.tiles == int(mine.sum())

            retire()
            r.render_frames(eye, rot, 0, EVERY)  # a restart: every tile renders again
            cleared()
            assert r.moments_frames() == EVERY
            for drop in (r.clear, lambda: r.set_accum(np.zeros((h, w, 4), F)), lambda: r.upload_scene(tris, nodes),
                         lambda: r.upload_env(hdr)):
                retire()
                drop()
                cleared()
                assert r.moments_frames() == 0
                assert rc_of(r.adaptive_update, **PRM) == INVALID  # the moments are not valid
            # a gap in frameCounter: no update, and the retired stay retired until a restart
            retire()
            r.render_frame(eye, rot, EVERY + 3)
            assert r.moments_frames() == 0
            assert rc_of(r.adaptive_update, **PRM) == INVALID
            assert np.array_equal(r.tile_error()[1], want)
            assert r.adaptive_status().retired == np.count_nonzero(want)
    finally:
        close(ranks)


# ------------------------------------------------------------------ 4. errors
def test_abi_13_and_symbols():
    lib = _native.load()
    assert lib.pt_abi_version() == 13 and _native.ABI_VERSION == 13
    for name in ("pt_pack_owned_stats", "pt_unpack_ranks_stats"):
        assert hasattr(lib, name) and name in _native.SIGNATURES


def test_create_accepts_the_flag_and_keeps_the_refusals():
    assert rc_of(Renderer, 32, 32, "lambert", flags=FLAG_SHARE_MOMENTS) == INVALID                    # no moments
    assert rc_of(Renderer, 32, 32, "lambert", flags=FLAG_SHARE_MOMENTS, tile_world=2) == INVALID
    assert rc_of(Renderer, 32, 32, "lambert", moments=True, share_moments=True, devices=[0, 0]) == INVALID
    assert rc_of(Renderer, 32, 32, "lambert", moments=True, share_moments=True, tile_world=2, sample_world=2) == INVALID
    for kw in (dict(moments=True), dict(adaptive=True)):  # without the flag: as before
        assert rc_of(Renderer, 32, 32, "lambert", tile_world=2, **kw) == INVALID, kw
        assert rc_of(Renderer, 32, 32, "lambert", tile_world=2, tile_rank=1, **kw) == INVALID, kw
    for kw in (dict(moments=True), dict(adaptive=True), dict(flags=FLAG_MOMENTS)):
        with Renderer(32, 32, "lambert", tile_world=2, tile_rank=1, share_moments=True, **kw) as r:
            assert r.moments_frames() == 0
    with Renderer(32, 32, "lambert", moments=True, share_moments=True) as r:  # tile_world 1: a moments context
        assert r.moments_frames() == 0


def test_stats_gather_error_paths():
    import torch
    buf = torch.zeros((32 * 32, 5), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ptr = buf.data_ptr()
    for kw in (dict(), dict(moments=True)):  # not flagged
        with Renderer(32, 32, "lambert", **kw) as r:
            assert rc_of(r.pack_owned_stats, ptr) == INVALID
            assert rc_of(r.unpack_ranks_stats, 2, [0, ptr]) == INVALID
    with Renderer(64, 32, "lambert", moments=True, share_moments=True, tile_world=2) as r:
        assert rc_of(r.pack_owned_stats, 0) == INVALID
        assert rc_of(r.unpack_ranks_stats, 0, [0]) == INVALID
        assert rc_of(r.unpack_ranks_stats, 17, [0] + [ptr] * 16) == INVALID
        assert rc_of(r.unpack_ranks_stats, 2, None) == INVALID
        assert r._lib.pt_pack_owned_stats(None, C.c_void_p(ptr)) == INVALID
        assert r._lib.pt_unpack_ranks_stats(None, 2, None) == INVALID
        r.pack_owned_stats(ptr)               # no frame yet: the zero planes
        r.unpack_ranks_stats(2, [0, 0])       # a null entry is skipped
        r.unpack_ranks_stats(16, [0] + [ptr] * 15)  # 64x32 in 16 shares: two shard tiles, ranks 2.. own nothing
        r.synchronize()
        assert not buf.cpu().numpy().any() and not r.moments().any()
