"""Guide buffers and the edge-avoiding a-trous denoised display on the GPU (pt_render_guides,
pt_denoise, pt_display_denoised) against the float32 restatement tests/denoise_ref.py, bit for bit:
the camera's first hits against the oracle's closest-hit search, the filter at sizes from one
pixel to several workgroups with LDS-staged and direct passes, the accumulation left untouched,
a screen-tile split, the 8-bit display, the quality gate and the error paths.

Reference: IS pass1.fsh:846-850 (the camera ray), :335-382 (hitBVH), :63-71 / :251-300 (the hit
record); Dammertz et al., HPG 2010 (the filter); pass3.fsh:14-24 (tonemap and display).
"""
import numpy as np
import pytest

import denoise_ref as dr
import oracle
from post_common import INVALID, NOSCENE, _unorm8, bits, config, rc_of
from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
from opengl_ray_tracing_amd.scene import Material, Scene

pytestmark = pytest.mark.gpu

F = np.float32
TERMS_OFF = [dict(sigma_c=0.0), dict(sigma_z=0.0), dict(sigma_a=0.0), dict(normal_log2=-1)]


def triangle_scene():
    s = Scene()
    v = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]], F)
    s.add_mesh(v, np.array([[0, 1, 2]], np.int32), Material(baseColor=(0.8, 0.6, 0.4)))
    s.build_bvh("sah", 8)
    return s.encode()


def renderer(name, w, h, **kw):
    cfg, tris, nodes, hdr, _, _ = config(name)
    r = Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


# ------------------------------------------------------------------ guides
def check_guides(tris, nodes, w, h, eye, rot):
    orc = oracle.Oracle(tris, nodes, None)
    want, rays, t, tri = dr.guides(orc, tris, w, h, eye, rot)
    with Renderer(w, h, "lambert") as r:
        r.upload_scene(tris, nodes)
        r.upload_env(scenes.synthetic_env(64, 32))
        r.render_frame(eye, rot, 0)
        before = r.stats()
        r.render_guides(eye, rot)
        got = r.guides()
        after = r.stats()
    assert (before.rays, before.launches, before.frames) == (after.rays, after.launches, after.frames)
    # the hit search: pt_trace_closest's semantics, the oracle's hitBVH of the restated rays
    assert np.array_equal(got["tri"].reshape(-1), tri)
    assert np.array_equal(bits(got["pos_t"][..., 3]).reshape(-1), bits(t))
    for k in ("pos_t", "nrm_tri", "albedo"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    return got, rays, tri


@pytest.mark.parametrize("w,h", [(33, 31), (100, 76)])
def test_guides_equal_the_restatement_c2(w, h):
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    got, _, tri = check_guides(tris, nodes, w, h, eye, rot)
    assert (tri >= 0).sum() > w * h // 4


def test_guides_single_triangle_front_and_back():
    """Most pixels miss; from behind the shading normal is flipped to face the camera."""
    tris, nodes = triangle_scene()
    w, h = 48, 40
    nz = []
    for angle in (15.0, 195.0):
        eye, rot = orbit_camera(angle, 10.0, 3.0)
        got, rays, tri = check_guides(tris, nodes, w, h, eye, rot)
        hit = tri >= 0
        assert 0 < hit.sum() < w * h // 2
        miss = ~hit.reshape(h, w)
        assert np.all(got["pos_t"][miss] == (0, 0, 0, dr.MISS_T)) and not got["albedo"][miss].any()
        n = got["nrm_tri"][..., :3].reshape(-1, 3)[hit]
        assert np.all(np.einsum("ij,ij->i", n, rays[hit, 3:6]) < 0)  # facing the camera
        nz.append(np.sign(n[:, 2]))
    assert np.all(nz[0] == 1) and np.all(nz[1] == -1)


# ------------------------------------------------------------------ the filter
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 31), (100, 76)])
@pytest.mark.parametrize("name", ["c4", "c2"])
def test_filter_equals_the_restatement(name, w, h):
    """1, 3 and 5 passes (8 at 33x31: every off-centre tap of the last passes is outside the
    image) with the defaults into the context's buffer, each of the four terms off in turn and
    the defaults again into a caller's buffer. 100x76 is no multiple of the 16-pixel tile and has
    interior LDS tiles; passes of stride >= 4 take the direct-load kernel."""
    import torch
    cfg, tris, nodes, hdr, eye, rot = config(name)
    with renderer(name, w, h) as r:
        for f in range(2):
            r.render_frame(eye, rot, f)
        acc = r.accum()
        r.render_guides(eye, rot)
        g = r.guides()
        for passes in [1, 3, 5] + ([8] if (w, h) == (33, 31) else []):
            got = r.denoise(passes=passes)
            want = dr.atrous(acc, g, **{**dr.DEFAULTS, "passes": passes})
            assert np.array_equal(bits(got), bits(want)), passes
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()  # the fill (torch's stream) before the renderer's stream writes it
        for prm in TERMS_OFF + [dict(passes=3)]:
            assert r.denoise(out.data_ptr(), **prm) is None
            r.synchronize()
            assert r.denoised_device_ptr() == out.data_ptr()
            want = dr.atrous(acc, g, **{**dr.DEFAULTS, **prm})
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), prm
        assert np.array_equal(bits(r.accum()), bits(acc))


def test_accumulation_is_untouched_and_frames_continue():
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h = 100, 76
    with renderer("c2", w, h) as r, renderer("c2", w, h) as plain:
        for f in range(2):
            r.render_frame(eye, rot, f)
            plain.render_frame(eye, rot, f)
        acc = r.accum()
        r.render_guides(eye, rot)
        den = r.denoise()
        assert np.array_equal(bits(r.accum()), bits(acc))
        assert not np.array_equal(den, acc)
        for f in range(2, 4):
            r.render_frame(eye, rot, f)
            plain.render_frame(eye, rot, f)
        assert np.array_equal(bits(r.accum()), bits(plain.accum()))


def test_screen_tile_split_rank0_denoises_the_gathered_mean():
    """Two tile_world = 2 contexts on one device: rank 0 unpacks rank 1's packed mean, renders the
    guides (every pixel, its non-owned ones included) and denoises: an unsplit context's result."""
    import torch
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h, world = 100, 76, 2
    with renderer("c2", w, h) as r:
        for f in range(2):
            r.render_frame(eye, rot, f)
        r.render_guides(eye, rot)
        g_full = r.guides()
        want = r.denoise()
    ranks = [renderer("c2", w, h, tile_rank=k, tile_world=world) for k in range(world)]
    try:
        for rr in ranks:
            for f in range(2):
                rr.render_frame(eye, rot, f)
        buf = torch.zeros((ranks[1].owned_pixel_count(), 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ranks[1].pack_owned(buf.data_ptr())
        ranks[1].synchronize()
        ranks[0].unpack_rank(1, world, buf.data_ptr())
        ranks[0].render_guides(eye, rot)
        g = ranks[0].guides()
        got = ranks[0].denoise()
    finally:
        for rr in ranks:
            rr.close()
    for k in ("pos_t", "nrm_tri", "albedo"):
        assert np.array_equal(bits(g[k]), bits(g_full[k])), k
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------ display
@pytest.mark.parametrize("gamma", [0.0, 2.2])
def test_display_denoised_is_pass3_of_the_denoised_image(gamma):
    """Every pixel's pass3 tonemap of the denoised image (the GPU's own f32 tonemap, pt_tonemap
    of that image uploaded as an accumulation) as an 8-bit unsigned-normalised RGBA pixel, alpha 255."""
    import torch
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h = 100, 76
    with renderer("c2", w, h) as r:
        for f in range(2):
            r.render_frame(eye, rot, f)
        r.render_guides(eye, rot)
        den = r.denoise()
        img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.display_denoised(img.data_ptr(), 1.5, gamma)
        r.synchronize()
        r.set_accum(den)
        t = r.tonemap(1.5, gamma)
    got = img.cpu().numpy()
    assert np.array_equal(got[..., :3], _unorm8(t)) and np.all(got[..., 3] == 255)


# ------------------------------------------------------------------ quality
@pytest.mark.parametrize("name", ["c4", "c2"])
def test_defaults_gain_at_least_2_db_on_the_gpu(name):
    """tests/test_denoise_ref.py's quality case with the GPU's own 4- and 256-frame means."""
    cfg, tris, nodes, hdr, eye, rot = config(name)
    w, h = 160, 90
    with renderer(name, w, h) as r:
        r.render_guides(eye, rot)
        r.render_frames(eye, rot, 0, 4)
        r.synchronize()
        noisy = r.accum()
        filtered = r.denoise()
        mask = r.guides()["tri"] >= 0
        r.render_frames(eye, rot, 4, 252)
        r.synchronize()
        clean = r.accum()
    before = dr.psnr_tm(noisy, clean, mask)
    after = dr.psnr_tm(filtered, clean, mask)
    print(f"{name}: PSNR {before:.2f} dB -> {after:.2f} dB (gain {after - before:+.2f} dB)")
    assert after - before >= 2.0, (name, before, after)


# ------------------------------------------------------------------ errors
def test_error_paths():
    import torch
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    w, h = 33, 31
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with Renderer(w, h, "lambert") as r:
        assert rc_of(r.render_guides, eye, rot) == NOSCENE
        assert rc_of(r.denoise) == NOSCENE
        assert rc_of(r.guides) == NOSCENE
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        r.render_frame(eye, rot, 0)
        assert rc_of(r.denoise) == INVALID  # before any render_guides
        assert rc_of(r.guides) == INVALID
        assert rc_of(r.display_denoised, img.data_ptr()) == INVALID  # before any denoise
        assert rc_of(r.denoised_device_ptr) == INVALID
        r.render_guides(eye, rot)
        for bad in (dict(passes=0), dict(passes=9), dict(normal_log2=-2), dict(normal_log2=11), dict(limit=0.0),
                    dict(limit=-1.0)):
            assert rc_of(r.denoise, **bad) == INVALID, bad
        assert rc_of(r.display_denoised, img.data_ptr()) == INVALID  # the failed calls denoised nothing
        r.denoise(passes=1)
        r.display_denoised(img.data_ptr())
        r.synchronize()
        r.upload_scene(tris, nodes)  # invalidates the guides
        assert rc_of(r.denoise) == INVALID
        assert rc_of(r.guides) == INVALID
        r.render_guides(eye, rot)
        r.denoise(passes=1)
    with Renderer(32, 32, "basic", basic_samples=1) as b:
        b.upload_shapes(scenes.cornell_shapes())
        assert rc_of(b.render_guides, eye, rot) == INVALID
        assert rc_of(b.denoise) == INVALID
