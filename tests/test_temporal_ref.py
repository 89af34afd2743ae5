"""The temporal resolve's ABI surface and its float32 restatement (tests/temporal_ref.py), on the
CPU: the projection is the inverse of the camera ray, a resolve without a history is the
accumulation, rejected history taps and history misses never reach the output, max_history caps the
counts, and over a drag of 8 cameras (1 frame each) the resolved image of the last camera beats
its raw 1-spp image by at least 2 dB of tone-mapped PSNR against the 256-frame mean.

Reference: OpenglRayTracing/main.cpp mouse() / mouseWheel() (frameCounter = 0 on every camera
move); IS pass1.fsh:846-850 (the camera ray that the projection inverts).
"""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import oracle
import temporal_ref as tr
from opengl_ray_tracing_amd import _native, orbit_camera, scenes

F = np.float32
NEW_SYMBOLS = ["pt_temporal_defaults", "pt_temporal_params_size", "pt_temporal_resolve", "pt_temporal_commit",
               "pt_temporal_reset", "pt_resolved_device_ptr", "pt_download_resolved", "pt_display_resolved",
               "pt_denoise_from"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------ ABI
def test_abi_version_and_symbols():
    lib = _native.load()
    assert lib.pt_abi_version() >= 9
    assert _native.ABI_VERSION >= 9
    for name in NEW_SYMBOLS:
        assert getattr(lib, name, None) is not None, name


def test_temporal_defaults_and_struct_size():
    lib = _native.load()
    assert C.sizeof(_native.PtTemporalParams) == lib.pt_temporal_params_size() == 12
    p = _native.PtTemporalParams()
    lib.pt_temporal_defaults(C.byref(p))
    got = (p.sigma_z, p.normal_cos, p.max_history)
    assert got == (F(0.02), F(0.9), F(32))
    assert got == tuple(F(v) for v in tr.DEFAULTS.values())


def test_null_context_is_invalid():
    lib = _native.load()
    ptr = C.c_void_p()
    buf = (C.c_float * 4)()
    assert lib.pt_temporal_resolve(None, None, 1, None) == -1
    assert lib.pt_temporal_commit(None) == -1
    assert lib.pt_temporal_reset(None) == -1
    assert lib.pt_resolved_device_ptr(None, C.byref(ptr)) == -1
    assert lib.pt_download_resolved(None, buf) == -1
    assert lib.pt_display_resolved(None, 1.5, 0.0, None) == -1
    assert lib.pt_denoise_from(None, None, None, None) == -1


# ------------------------------------------------------------------ synthetic guides
def floor_guides(w, h, eye, rot, y0=-0.5):
    """Guide planes of the floor y = y0 seen by a camera: exact ray / plane hits of the restated
    camera rays (a ray that does not look down misses)."""
    rays = dr.camera_rays(w, h, eye, rot)
    o, d = rays[:, 0:3], rays[:, 3:6]
    hit = d[:, 1] < F(-1e-3)
    with np.errstate(all="ignore"):
        t = ((F(y0) - o[:, 1]) / d[:, 1]).astype(F)
    P = (o + d * t[:, None]).astype(F)
    pos_t = np.zeros((h * w, 4), F)
    nrm = np.zeros((h * w, 4), F)
    pos_t[:, 3] = dr.MISS_T
    pos_t[hit, 0:3] = P[hit]
    pos_t[hit, 3] = t[hit]
    nrm[hit, 1] = 1
    nrm[:, 3] = np.where(hit, 0, -1).astype(np.int32).view(F)
    return {"pos_t": pos_t.reshape(h, w, 4), "nrm_tri": nrm.reshape(h, w, 4)}


def random_image(rng, h, w, count):
    c = np.empty((h, w, 4), F)
    c[..., :3] = rng.uniform(0, 4, (h, w, 3))
    c[..., 3] = count
    return c


def test_no_history_is_the_accumulation():
    rng = np.random.default_rng(3)
    w, h = 37, 23
    eye, rot = orbit_camera(10.0, 30.0, 4.0)
    g = floor_guides(w, h, eye, rot)
    c = random_image(rng, h, w, 1.0)
    out = tr.resolve(c, 5, g, None)
    assert np.array_equal(bits(out[..., :3]), bits(c[..., :3]))
    assert np.all(out[..., 3] == 5)


def test_projection_inverts_the_camera_ray():
    """Every hit pixel of c2's camera at 160x90 projects onto its own centre: f32 rounding is about
    1e-4 px here, a wrong half-pixel, focal length or transposed rotation 0.5 px or more."""
    cfg, tris, nodes, hdr = scenes.build_config("c2")
    eye, rot = orbit_camera(*cfg.camera)
    w, h = 160, 90
    orc = oracle.Oracle(tris, nodes, None)
    g, _, _, _ = dr.guides(orc, tris, w, h, eye, rot)
    hit = dr.hit_mask(g)
    assert hit.sum() > 1000
    fx, fy, cz = tr.project(g["pos_t"][..., :3], eye, rot, w, h)
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    ex, ey = np.abs(fx - px)[hit].max(), np.abs(fy - py)[hit].max()
    print(f"projection error: {ex:.2e} px, {ey:.2e} px")
    assert ex <= 0.01 and ey <= 0.01
    assert np.all(cz[hit] < 0)
    # a rotated camera (not symmetric): the transposed rotation would be far off
    eye2, rot2 = orbit_camera(35.0, 25.0, 4.0)
    g2 = floor_guides(w, h, eye2, rot2)
    hit2 = dr.hit_mask(g2)
    assert hit2.sum() > 1000
    fx, fy, cz = tr.project(g2["pos_t"][..., :3], eye2, rot2, w, h)
    assert np.abs(fx - px)[hit2].max() <= 0.01 and np.abs(fy - py)[hit2].max() <= 0.01


def test_rejected_taps_and_history_misses_are_isolated():
    """History colours of 1e6 at the history's miss pixels, at pixels without samples and at
    pixels whose taps the plane or the normal test rejects change no output bit."""
    rng = np.random.default_rng(5)
    w, h = 61, 47
    eyeA, rotA = orbit_camera(10.0, 30.0, 4.0)
    eyeB, rotB = orbit_camera(12.0, 30.0, 4.0)
    gA, gB = floor_guides(w, h, eyeA, rotA), floor_guides(w, h, eyeB, rotB)
    hitA = dr.hit_mask(gA)
    assert hitA.any() and (~hitA).any()
    kind = np.where(hitA, rng.integers(0, 12, (h, w)), -1)  # 1..4: rejected, each in its own way
    gA["nrm_tri"][..., 3] = np.where(kind == 1, -1, gA["nrm_tri"][..., 3].view(np.int32)).astype(np.int32).view(F)
    gA["nrm_tri"][kind == 2, 1] = -1                    # faces away
    gA["pos_t"][kind == 3, 1] += 1e4                    # off the plane, whatever t_p is
    histc = random_image(rng, h, w, 3.0)
    histc[kind == 4, 3] = 0                             # no samples
    bad = (kind >= 1) & (kind <= 4) | ~hitA
    c = random_image(rng, h, w, 1.0)
    out = tr.resolve(c, 1, gB, tr.commit(histc, gA, eyeA, rotA))
    took = out[..., 3] > 1
    assert took.sum() > 200 and not np.array_equal(out[took][:, :3], c[took][:, :3])
    poisoned = histc.copy()
    poisoned[bad, :3] = 1e6
    out2 = tr.resolve(c, 1, gB, tr.commit(poisoned, gA, eyeA, rotA))
    assert np.array_equal(bits(out2), bits(out))
    assert out2[..., :3].max() < 5
    miss = ~dr.hit_mask(gB)
    assert np.array_equal(bits(out[miss][:, :3]), bits(c[miss][:, :3])) and np.all(out[miss][:, 3] == 1)


def test_max_history_caps_the_counts():
    rng = np.random.default_rng(9)
    w, h = 61, 47
    top = {}
    for mh in (2.5, 32.0):
        hist = None
        for k in range(3):
            eye, rot = orbit_camera(10.0 + 2.0 * k, 30.0, 4.0)
            g = floor_guides(w, h, eye, rot)
            out = tr.resolve(random_image(rng, h, w, 1.0), 2, g, hist, max_history=mh)
            hist = tr.commit(out, g, eye, rot)
        top[mh] = out[..., 3]
    assert top[2.5].max() == 4.5 and (top[2.5] == 4.5).sum() > 200   # min(4, 2.5) + 2
    assert top[32.0].max() == 6.0 and (top[32.0] == 6.0).sum() > 100  # 2 + 2 + 2
    assert top[2.5].min() == 2.0


# ------------------------------------------------------------------ quality
W, H = 160, 90
CAMERAS, STEP, CLEAN_FRAMES = 8, 2.0, 256


def drag_cameras(cfg, n=CAMERAS, step=STEP):
    """n cameras on the orbit, `step` degrees apart, ending at the config's camera."""
    angle, up, r = cfg.camera
    return [orbit_camera(angle - (n - 1 - k) * step, up, r) for k in range(n)]


def quality_row(name, raw, resolved, g, clean):
    mask = dr.hit_mask(g)
    cols = [raw, resolved, dr.atrous(raw, g, **dr.DEFAULTS), dr.atrous(resolved, g, **dr.DEFAULTS)]
    p = [dr.psnr_tm(x, clean, mask) for x in cols]
    print(f"{name}, {STEP:g} deg: raw 1 spp {p[0]:.2f} dB | resolved {p[1]:.2f} | a-trous only {p[2]:.2f} | "
          f"resolved + a-trous {p[3]:.2f}")
    return p


@pytest.mark.parametrize("name", ["c4", "c2"])
def test_drag_gains_at_least_2_db(name):
    """Tone-mapped PSNR over the hit pixels of the last camera against its 256-frame mean: the
    resolved image of an 8-camera drag (2 degrees apart, 1 frame each, frameCounter 0) beats the raw
    1-spp image by at least 2 dB (the prototype measured +5.0 dB on c2 and +8.4 dB on c4; the gate
    sits far below, where a wrong weight or projection still shows)."""
    cfg, tris, nodes, hdr = scenes.build_config(name)
    orc = oracle.Oracle(tris, nodes, hdr)
    hist = None
    for eye, rot in drag_cameras(cfg):
        raw, _ = orc.render(W, H, cfg.integrator, 0, eye, rot, accum=np.zeros((H, W, 4), F), max_bounce=cfg.max_bounce)
        g, _, _, _ = dr.guides(orc, tris, W, H, eye, rot)
        resolved = tr.resolve(raw, 1, g, hist)
        hist = tr.commit(resolved, g, eye, rot)
    clean = np.zeros((H, W, 4), F)
    for f in range(CLEAN_FRAMES):
        clean, _ = orc.render(W, H, cfg.integrator, f, eye, rot, accum=clean, max_bounce=cfg.max_bounce)
    assert dr.hit_mask(g).sum() > 1000
    p = quality_row(name, raw, resolved, g, clean)
    assert p[1] - p[0] >= 2.0, (name, p)
