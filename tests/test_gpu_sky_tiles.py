"""All-sky tiles shaded by the running-mean update (pt_display.hip mixFrames, pt_kernels.h SkyTiles): in a
pipelined launch a tile whose camera-ray bin is empty is not given to the camera-ray pass (pt_primary.hip
primaryKernel over PrimaryBins::passList); the update computes its samples and counts its rays. The shapes
are the smallest at which that can go wrong -- no pass tile at all (an empty list: no pass launch), images
smaller than a tile, partial edge tiles, one pass tile near the end of the list, a tile whose bin is
non-empty only through the bins' 2-pixel margin, masks left in a slot's buffer by an earlier camera or
scene, moments and adaptive contexts, the frame kernels other than the default behind a pass, and
screen-tile shares that own nothing -- and every image is compared with the oracle bit for bit
(tests/parity.py, exact == 1.0).

Ray counts: Lambert's and uniform Disney's equal the oracle's. The MIS kernels do not trace a BRDF ray
whose pdf is 0 (tests/test_gpu_live_tiles.py), so their counts are held to the figures the commit before
this change gave (tests/golden/sky_tiles/mis_rays.json, written by tests/golden/make_sky_tiles_fixture.py),
and stay at or below the oracle's.

Reference: IS pass1.fsh:846-871 (camera ray, sky, running mean), IS:184-189 (sampleHdr).
"""
import json
from pathlib import Path

import numpy as np
import pytest

import oracle
import parity
import adaptive_ref as ar
import variance_ref as vr
from opengl_ray_tracing_amd import FLAG_MEGAKERNEL, FLAG_PRIMARY_PASS, FLAG_REGEN, Renderer, orbit_camera, scenes
from test_gpu_live_tiles import (FORCED, behind_camera, gpu_frames, live_tiles, oracle_frames, pixel_triangle)

pytestmark = pytest.mark.gpu

F = np.float32
EYE, ROT = orbit_camera(20.0, 10.0, 4.0)
MIS_RAYS_FILE = Path(__file__).parent / "golden" / "sky_tiles" / "mis_rays.json"
RECORD = None  # make_sky_tiles_fixture.py: a dict that takes the MIS counts instead of checking them


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_rays(integrator, gpu, orc, key):
    if integrator != "mis":
        assert gpu == orc, (key, gpu, orc)
    elif RECORD is not None:
        RECORD[key] = int(gpu)
    else:
        want = json.loads(MIS_RAYS_FILE.read_text())[key]
        assert gpu == want and gpu <= orc, (key, gpu, want, orc)


@pytest.fixture(scope="module")
def env():
    return scenes.synthetic_env(64, 32)


def inner_triangle(w, h, off):
    """A 2 x 2 pixel half-rectangle in the image's last tile, its corner `off` pixels inside the tile: 2.3
    keeps the bins' 2-pixel margin inside the tile (every other bin is empty); 0.6 puts the tile to the
    left and the one below within the margin, so their bins are non-empty though all their pixels are sky."""
    tx, ty = (w - 1) // 8, (h - 1) // 8
    x0, y0 = 8 * tx + off, 8 * ty + off
    return pixel_triangle(EYE, ROT, w, h, x0, y0, x0 + 2.0, y0 + 2.0), (ty, tx)


# ------------------------------------------------------------------ 1. no pass tile
@pytest.mark.parametrize("w,h", [(70, 45), (1, 1), (5, 3), (8, 1)])
def test_no_pass_tile(env, w, h):
    """One triangle behind the camera: the pass list is empty, no pass is launched, and the update shades
    every pixel. 70 x 45 has edge tiles with lanes outside the image (and share tiles wholly outside it),
    which count no ray."""
    frames = 7
    tris, nodes = behind_camera(EYE, ROT, w, h)
    ref, rays, hit = oracle_frames(tris, nodes, env, w, h, "lambert", EYE, ROT, frames)
    assert not hit.any() and rays == w * h * frames
    for mode in ((7,), (3, 3, 1), "stream"):
        g, n = gpu_frames(tris, nodes, env, w, h, "lambert", EYE, ROT, frames, mode)
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), f"no pass tile/{w}x{h}/{mode}")
        assert n == w * h * frames, (mode, n)


# ------------------------------------------------------------------ 2. one pass tile among empty ones
@pytest.mark.parametrize("w,h", [(70, 45), (16, 16), (160, 32)])
@pytest.mark.parametrize("off", [2.3, 0.6], ids=["inside", "margin"])
@pytest.mark.parametrize("integrator", ["lambert", "mis"])
def test_one_pass_tile(env, integrator, off, w, h):
    frames = 3
    (tris, nodes), tile = inner_triangle(w, h, off)
    ref, rays, hit = oracle_frames(tris, nodes, env, w, h, integrator, EYE, ROT, frames)
    assert live_tiles(hit) == {tile}
    for mode in ("stream", (2, 1)):
        g, n = gpu_frames(tris, nodes, env, w, h, integrator, EYE, ROT, frames, mode)
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), f"one pass tile/{integrator}/{off}/{w}x{h}/{mode}")
        check_rays(integrator, n, rays, f"one pass tile/{off}/{w}x{h}/{mode}")


# ------------------------------------------------------------------ 3. stale masks
@pytest.mark.parametrize("how", ["camera", "upload", "refit"])
def test_stale_masks(env, how):
    """Three batches, so both pipeline slots hold tile A's masks; then A's bin becomes empty and another
    tile's does not -- by a camera move, by another scene, by a geometry update in place -- and three more
    batches must find A's masks 0 in both slots."""
    w, h = 64, 40
    eye2, rot2 = orbit_camera(20.0, 10.0, 6.0)
    tris, nodes = pixel_triangle(EYE, ROT, w, h, 4.0, 3.0, 22.0, 15.0, depth=1.5)
    tris2, nodes2 = pixel_triangle(EYE, ROT, w, h, 40.0, 20.0, 62.0, 38.0, depth=2.0)
    first = (tris, nodes, EYE, ROT)
    second = (tris, nodes, eye2, rot2) if how == "camera" else (tris2, nodes2, EYE, ROT)
    refs = [oracle_frames(t, n, env, w, h, "lambert", e, m, 6) for t, n, e, m in (first, second)]
    la, lb = (live_tiles(r[2]) for r in refs)
    assert la - lb and lb - la
    with Renderer(w, h, "lambert", flags=FORCED) as r:
        r.upload_env(env)
        r.upload_scene(tris, nodes)
        seen = 0
        for k, ((t, n, e, m), (ref, rays, _)) in enumerate(zip((first, second), refs)):
            if k == 1 and how == "upload":
                r.upload_scene(t, n)
            if k == 1 and how == "refit":
                r.update_geometry(np.asarray(t, F).reshape(-1, 36))
            for f in (0, 2, 4):
                r.render_frames(e, m, f, 2)
            r.synchronize()
            parity.assert_parity(r.accum().reshape(-1, 4), ref.reshape(-1, 4), f"stale masks/{how}/{k}")
            st = r.stats()
            assert st.regen == 1 and st.rays - seen == rays, (how, k, st.rays - seen, rays)
            seen = st.rays


# ------------------------------------------------------------------ 4. the update's samples are the pass's
@pytest.mark.parametrize("env_size", [(64, 32), (33, 17)])
@pytest.mark.parametrize("scene", ["sky", "triangle"])
def test_update_equals_pass(env_size, scene):
    """Streamed batches (the update shades the empty-bin tiles) against PT_FLAG_SERIAL_FRAMES and display()
    calls (not pipelined: the pass shades them), on an env of even and of odd size."""
    w, h, frames = 70, 45, 5
    hdr = scenes.synthetic_env(*env_size)
    tris, nodes = behind_camera(EYE, ROT, w, h) if scene == "sky" else inner_triangle(w, h, 0.6)[0]
    ref, rays, _ = oracle_frames(tris, nodes, hdr, w, h, "lambert", EYE, ROT, frames)
    out = [gpu_frames(tris, nodes, hdr, w, h, "lambert", EYE, ROT, frames, m) for m in ((3, 2), "serial", "call")]
    for g, n in out:
        assert np.array_equal(bits(g), bits(out[0][0])) and n == out[0][1] == rays
    parity.assert_parity(out[0][0].reshape(-1, 4), ref.reshape(-1, 4), f"update equals pass/{scene}/{env_size}")


# ------------------------------------------------------------------ 5. moments and adaptive contexts
@pytest.mark.parametrize("scene", ["sky", "triangle"])
def test_moments(env, scene):
    w, h, frames = 70, 45, 5
    tris, nodes = behind_camera(EYE, ROT, w, h) if scene == "sky" else inner_triangle(w, h, 0.6)[0]
    orc = oracle.Oracle(tris, nodes, env)
    acc, m = np.zeros((h, w, 4), F), np.zeros((h, w, 2), F)
    for k in range(frames):
        s, _ = orc.render(w, h, "lambert", 0, EYE, ROT, accum=np.zeros((h, w, 4), F), max_bounce=2, sample_rank=k,
                          sample_world=frames)
        acc = vr.mix_sample(acc, s, k)
        m = vr.moments_update(m, s, k)
    with Renderer(w, h, "lambert", flags=FORCED, moments=True) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(env)
        r.render_frames(EYE, ROT, 0, 3)
        r.render_frames(EYE, ROT, 3, 2)
        assert r.moments_frames() == frames
        assert np.array_equal(bits(r.accum()), bits(acc))
        assert np.array_equal(bits(r.moments()), bits(m))


ADAPT = dict(threshold=4 / 255, limit=1.5, min_frames=2)
ADAPT_BATCHES = (4, 3, 2)


def adaptive_want(env, w, h):
    """-> (tests/adaptive_ref.py's run over the oracle's samples with an update after each batch, the rays of
    the samples it takes)."""
    tris, nodes = inner_triangle(w, h, 0.6)[0]
    orc = oracle.Oracle(tris, nodes, env)
    frames = sum(ADAPT_BATCHES)
    samples = [orc.render(w, h, "lambert", 0, EYE, ROT, accum=np.zeros((h, w, 4), F), max_bounce=2, sample_rank=k,
                          sample_world=frames)[0] for k in range(frames)]
    want = ar.run(samples, 0, ADAPT, updates_at=np.cumsum(ADAPT_BATCHES).tolist())
    rays = 0
    for f, active in enumerate(want["active"]):
        ys, xs = np.nonzero(active)
        if ys.size:  # (an empty pixel list would mean every pixel)
            rays += orc.render(w, h, "lambert", f, EYE, ROT, pixels=np.stack([xs, ys], -1), max_bounce=2)[1].rays
    return (tris, nodes), want, rays


def test_adaptive(env):
    """The all-sky tiles retire at the first update and the triangle's tile stays: the update then takes no
    sample of a retired tile and counts no ray for it. Accumulation, moments, retirement plane and ray count equal tests/adaptive_ref.py's run over
    the oracle's samples. (A PT_FLAG_MOMENTS context cannot be created with PT_FLAG_SERIAL_FRAMES, so
    there is no unpipelined adaptive context to compare with; the restatement is the reference, as in
    tests/test_gpu_adaptive.py.)"""
    w, h = 70, 45
    (tris, nodes), want, rays = adaptive_want(env, w, h)
    tiles = want["retired_at"].size
    assert 0 < want["counts"][0] < tiles and rays < sum(ADAPT_BATCHES) * w * h
    with Renderer(w, h, "lambert", flags=FORCED, adaptive=True) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(env)
        f = 0
        for k, n in enumerate(ADAPT_BATCHES):
            r.render_frames(EYE, ROT, f, n)
            f += n
            r.adaptive_update(**ADAPT)
            acc, m, _, at = want["history"][k]
            assert np.array_equal(bits(r.accum()), bits(acc)), k
            assert np.array_equal(bits(r.moments()), bits(m)), k
            assert np.array_equal(r.tile_error()[1], at), k
            assert r.adaptive_status().retired == want["counts"][k], k
        assert r.stats().rays == rays


# ------------------------------------------------------------------ 6. other frame kernels behind a pass
@pytest.mark.parametrize("integrator,mb,flags", [("disney", 5, FLAG_MEGAKERNEL | FLAG_PRIMARY_PASS),
                                                 ("mis", 8, FLAG_MEGAKERNEL | FLAG_PRIMARY_PASS),
                                                 ("mis", 3, FLAG_REGEN | FLAG_PRIMARY_PASS)],
                         ids=["megakernel-disney5", "megakernel-mis8", "regen-mis3"])
def test_other_kernels_behind_a_pass(env, integrator, mb, flags):
    w, h, frames = 70, 45, 7
    tris, nodes = pixel_triangle(EYE, ROT, w, h, 30.0, 12.0, w - 1.2, h - 1.2)
    ref, rays, hit = oracle_frames(tris, nodes, env, w, h, integrator, EYE, ROT, frames, mb)
    assert 1 < len(live_tiles(hit)) < 54
    with Renderer(w, h, integrator, max_bounce=mb, flags=flags) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(env)
        f = 0
        for n in (3, 3, 1):
            r.render_frames(EYE, ROT, f, n)
            f += n
        r.synchronize()
        st = r.stats()
        assert st.regen == (1 if flags & FLAG_REGEN else 0)
        parity.assert_parity(r.accum().reshape(-1, 4), ref.reshape(-1, 4), f"behind a pass/{integrator}{mb}")
        check_rays(integrator, st.rays, rays, f"behind a pass/{integrator}{mb}/{flags:#x}")


# ------------------------------------------------------------------ 7. screen-tile shares
@pytest.mark.parametrize("w,h,world", [(40, 40, 8), (160, 32, 3)])
def test_screen_tile_shares(env, w, h, world):
    """40 x 40 is 2 x 2 screen tiles of 32 x 32 split 8 ways (ranks 4-7 own nothing); 160 x 32 is 5 x 1 split
    3 ways. Each rank's own pixels equal the oracle's, the others stay 0, and the ranks' rays sum to its count."""
    frames = 3
    tris, nodes = pixel_triangle(EYE, ROT, w, h, 3.0, 2.0, 20.0, 14.0)  # inside screen tile 0
    ref, rays, hit = oracle_frames(tris, nodes, env, w, h, "lambert", EYE, ROT, frames)
    assert hit.any()
    sx, sy = (w + 31) // 32, (h + 31) // 32
    total = 0
    for rank in range(world):
        a, n = gpu_frames(tris, nodes, env, w, h, "lambert", EYE, ROT, frames, "stream", tile_rank=rank, tile_world=world)
        mine = np.zeros((h, w), bool)
        for t in range(rank, sx * sy, world):
            ty, tx = divmod(t, sx)
            mine[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] = True
        assert np.array_equal(bits(a[mine]), bits(ref[mine])) and not a[~mine].any(), rank
        if not mine.any():
            assert n == 0, (rank, n)
        total += n
    assert total == rays
