"""The sample moments' and the variance-guided filter's ABI surface and their float32 restatement
(tests/variance_ref.py), on the CPU: the samples folded with the accumulation's own update
reproduce the oracle's running mean bit for bit and their moments are the mean and the mean square;
with its terms off a pass is denoise_ref's pass and propagates a constant variance by
sum(k^2) / sum(k)^2; miss pixels stay out of the filter; and against the oracle's 2048-frame mean
the filter keeps gaining where the fixed-width a-trous filter saturates.

Reference: Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017); Dammertz et al.
(HPG 2010); pass3.fsh:14-24 (the tonemap whose luminance the variance is of).
"""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import oracle
import variance_ref as vr
from opengl_ray_tracing_amd import _native, orbit_camera, scenes
from test_denoise_ref import synthetic_guides

F = np.float32
NEW_SYMBOLS = ["pt_moments_frames", "pt_download_moments", "pt_moments_device_ptr", "pt_denoise_var_defaults",
               "pt_denoise_var_params_size", "pt_denoise_var", "pt_download_variance"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------ ABI
def test_abi_version_and_symbols():
    lib = _native.load()
    assert lib.pt_abi_version() >= 10
    assert _native.ABI_VERSION >= 10
    for name in NEW_SYMBOLS:
        assert getattr(lib, name, None) is not None, name


def test_denoise_var_defaults_and_struct_size():
    lib = _native.load()
    assert C.sizeof(_native.PtDenoiseVarParams) == lib.pt_denoise_var_params_size() == 28
    p = _native.PtDenoiseVarParams()
    lib.pt_denoise_var_defaults(C.byref(p))
    got = (p.passes, p.sigma_l, p.sigma_z, p.sigma_a, p.normal_log2, p.limit, p.min_temporal)
    assert got == (5, F(4.0), F(0.02), F(0.2), 6, F(1.5), 8)
    assert got == tuple(F(v) if isinstance(v, float) else v for v in vr.DEFAULTS.values())


def test_null_context_is_invalid():
    lib = _native.load()
    ptr = C.c_void_p()
    n = C.c_uint32()
    buf = (C.c_float * 4)()
    assert lib.pt_moments_frames(None, C.byref(n)) == -1
    assert lib.pt_download_moments(None, buf) == -1
    assert lib.pt_moments_device_ptr(None, C.byref(ptr)) == -1
    assert lib.pt_denoise_var(None, None, None, None) == -1
    assert lib.pt_download_variance(None, buf) == -1


# ------------------------------------------------------------------ moments
def oracle_samples(orc, cfg, w, h, eye, rot, n):
    """Sample k alone: frame 0 of sample rank k of n, so its weight is 1 and its sample index k."""
    return [orc.render(w, h, cfg.integrator, 0, eye, rot, accum=np.zeros((h, w, 4), F), max_bounce=cfg.max_bounce,
                       sample_rank=k, sample_world=n)[0] for k in range(n)]


def test_moments_restatement_against_the_oracle():
    """Folding the 7 samples with mixf in f32 gives the oracle's own 7-frame accumulation bit for bit
    (the samples are the right ones), and their moments are the f64 mean and mean square of the
    luminance within 1e-5 relative: seven f32 mixes of three roundings each, each under 6e-8."""
    cfg, tris, nodes, hdr = scenes.build_config("c2")
    eye, rot = orbit_camera(*cfg.camera)
    w, h, n = 33, 31, 7
    orc = oracle.Oracle(tris, nodes, hdr)
    samples = oracle_samples(orc, cfg, w, h, eye, rot, n)
    want = np.zeros((h, w, 4), F)
    acc = np.zeros((h, w, 4), F)
    for k in range(n):
        want, _ = orc.render(w, h, cfg.integrator, k, eye, rot, accum=want, max_bounce=cfg.max_bounce)
        acc = vr.mix_sample(acc, samples[k], k)
    assert np.array_equal(bits(acc), bits(want))
    m = vr.moments(samples)
    s = np.stack([x[..., :3] for x in samples]).astype(np.float64)
    l = (0.3 * s[..., 0] + 0.6 * s[..., 1]) + 0.1 * s[..., 2]
    m1, m2 = l.mean(0), (l * l).mean(0)
    assert m1.max() > 0
    e1 = np.abs(m[..., 0] - m1).max() / m1.max()
    e2 = np.abs(m[..., 1] - m2).max() / m2.max()
    r1 = (np.abs(m[..., 0] - m1) / np.where(m1 > 0, m1, 1)).max()
    r2 = (np.abs(m[..., 1] - m2) / np.where(m2 > 0, m2, 1)).max()
    print(f"moments: m1 rel {r1:.2e} (of max {e1:.2e}), m2 rel {r2:.2e} (of max {e2:.2e})")
    assert r1 <= 1e-5 and r2 <= 1e-5
    # a restart at frame 0 forgets what the plane held
    again = vr.moments(samples[:2], 0, m)
    assert np.array_equal(bits(again), bits(vr.moments(samples[:2])))


# ------------------------------------------------------------------ step A and B on synthetic guides
def random_colour(rng, h, w):
    return np.concatenate([rng.uniform(0, 4, (h, w, 3)), np.ones((h, w, 1))], -1).astype(F)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_terms_off_is_the_atrous_pass_and_propagates_the_variance(s):
    rng = np.random.default_rng(17 + s)
    h, w = 19, 23
    g = synthetic_guides(h, w, rng)
    c = random_colour(rng, h, w)
    v = np.full((h, w), 0.37, F)
    out, v_out = vr.var_pass(c, v, g, s, 0.0, 0.0, 0.0, -1, 1.5)
    assert np.array_equal(bits(out), bits(dr.atrous_pass(c, g, s, 0.0, 0.0, 0.0, -1, 1.5)))
    # an interior pixel sees all 25 taps: w = k, so v_out = v sum(k^2) / sum(k)^2 (sum(k) = 1)
    k1 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    k2 = np.outer(k1, k1)
    want = 0.37 * (k2 ** 2).sum() / k2.sum() ** 2
    inner = v_out[2 * s:h - 2 * s, 2 * s:w - 2 * s]
    assert inner.size > 0
    assert np.abs(inner / want - 1).max() <= 1e-5, (inner.min(), inner.max(), want)


def test_miss_pixels_stay_out_of_the_filter():
    """A miss pixel comes out bit-identical, variance 0 from step A and copied by step B; no hit
    pixel's colour or variance depends on a miss pixel's colour, moments or variance."""
    rng = np.random.default_rng(23)
    h, w = 21, 26
    g = synthetic_guides(h, w, rng, miss_fraction=0.3)
    miss = ~dr.hit_mask(g)
    assert miss.any() and (~miss).any()
    c = random_colour(rng, h, w)
    m1 = rng.uniform(0.5, 2, (h, w))
    m = np.stack([m1, m1 * m1 + rng.uniform(0.01, 1, (h, w))], -1).astype(F)
    c2, m2 = c.copy(), m.copy()
    c2[miss, :3] = rng.uniform(50, 1e6, (int(miss.sum()), 3)).astype(F)
    m2[miss] = (1e3, 1e9)
    for frames in (2, 9):  # spatial, temporal
        out, v0 = vr.denoise_var(c, g, m, frames, passes=3, with_variance=True)
        assert np.all(v0[miss] == 0) and (v0[~miss] > 0).any()
        assert np.array_equal(bits(out[miss]), bits(c[miss]))
        assert not np.array_equal(out[~miss], c[~miss])  # the hits were filtered
        out2, v02 = vr.denoise_var(c2, g, m2, frames, passes=3, with_variance=True)
        assert np.array_equal(bits(out2[~miss]), bits(out[~miss])), frames
        assert np.array_equal(bits(v02), bits(v0)), frames
        assert np.array_equal(bits(out2[miss]), bits(c2[miss]))
    # the propagated variance: poison the miss pixels' input variance of one pass
    v = rng.uniform(0.01, 1, (h, w)).astype(F)
    vp = v.copy()
    vp[miss] = 1e9
    o1, v1 = vr.var_pass(c, v, g, 1, 4.0, 0.02, 0.2, 6, 1.5)
    o2, v2 = vr.var_pass(c2, vp, g, 1, 4.0, 0.02, 0.2, 6, 1.5)
    assert np.array_equal(bits(o1[~miss]), bits(o2[~miss])) and np.array_equal(bits(v1[~miss]), bits(v2[~miss]))
    assert np.array_equal(bits(v1[miss]), bits(v[miss])) and np.array_equal(bits(v2[miss]), bits(vp[miss]))


def test_n_p_is_the_larger_of_the_count_and_the_frames():
    """A resolved image's .w above the frame count divides the variance by it; below, kf does."""
    rng = np.random.default_rng(29)
    h, w = 9, 11
    g = synthetic_guides(h, w, rng)
    c = random_colour(rng, h, w)
    m = np.stack([np.ones((h, w)), np.full((h, w), 3.0)], -1).astype(F)
    v9 = vr.initial_variance(c, g, m, 9)
    c[..., 3] = 4
    assert np.array_equal(bits(vr.initial_variance(c, g, m, 9)), bits(v9))
    c[..., 3] = 36
    v36 = vr.initial_variance(c, g, m, 9)
    assert np.abs(v36 * 4 / v9 - 1).max() <= 1e-6


# ------------------------------------------------------------------ quality
W, H = 160, 90
CLEAN_FRAMES = 2048
STOPS = (4, 16, 64, 256)


def quality_rows(name):
    """PSNR rows of a config: the oracle's running mean and moments at STOPS frames, raw, through
    dr.atrous and through vr.denoise_var (defaults both), against its 2048-frame mean."""
    cfg, tris, nodes, hdr = scenes.build_config(name)
    eye, rot = orbit_camera(*cfg.camera)
    orc = oracle.Oracle(tris, nodes, hdr)
    g, _, _, _ = dr.guides(orc, tris, W, H, eye, rot)
    mask = dr.hit_mask(g)
    assert mask.sum() > 1000
    acc = np.zeros((H, W, 4), F)
    m = np.zeros((H, W, 2), F)
    snap = {}
    for k in range(CLEAN_FRAMES):
        s, _ = orc.render(W, H, cfg.integrator, 0, eye, rot, accum=np.zeros((H, W, 4), F), max_bounce=cfg.max_bounce,
                          sample_rank=k, sample_world=CLEAN_FRAMES)
        acc = vr.mix_sample(acc, s, k)
        if k < max(STOPS):
            m = vr.moments_update(m, s, k)
        if k + 1 in STOPS:
            snap[k + 1] = (acc, m)
    rows = {}
    for k, (a, mm) in snap.items():
        rows[k] = (dr.psnr_tm(a, acc, mask), dr.psnr_tm(dr.atrous(a, g, **dr.DEFAULTS), acc, mask),
                   dr.psnr_tm(vr.denoise_var(a, g, mm, k, **vr.DEFAULTS), acc, mask))
        print(f"{name}, {k:3d} frames: raw {rows[k][0]:.2f} dB | pt_denoise {rows[k][1]:.2f} | "
              f"pt_denoise_var {rows[k][2]:.2f}")
    return rows


@pytest.fixture(scope="module")
def quality():
    """Measured with this restatement (dB; raw, pt_denoise, pt_denoise_var):
    c2: 4 frames 8.81 20.89 20.34 | 16: 12.69 24.68 23.48 | 64: 17.95 26.61 28.90 | 256: 24.15 26.64 31.21
    c4: 4 frames 18.85 29.38 31.62 | 16: 24.81 29.69 33.27 | 64: 30.68 30.00 35.42 | 256: 36.63 30.13 37.64"""
    return {name: quality_rows(name) for name in ("c4", "c2")}


@pytest.mark.parametrize("name", ["c4", "c2"])
def test_gate_a_gain_at_4_frames(quality, name):
    raw, _, var = quality[name][4]
    assert var - raw >= 2.0, (name, quality[name][4])


@pytest.mark.parametrize("name", ["c4", "c2"])
def test_gate_b_converged_images_are_not_blurred(quality, name):
    raw, atrous, var = quality[name][256]
    assert var >= raw, (name, quality[name][256])
    assert var >= atrous + 2.0, (name, quality[name][256])


def test_gate_c_c4_at_64_frames(quality):
    """The defect the filter is for: the fixed-width filter is below the raw mean there."""
    raw, atrous, var = quality["c4"][64]
    assert atrous < raw, quality["c4"][64]
    assert var >= raw + 2.0, quality["c4"][64]


def test_gate_d_c2_cost_of_sigma_l_4(quality):
    """The known cost of sigma_l = 4 on c2's few frames, bounded so that it cannot grow unseen."""
    for k in (4, 16):
        raw, atrous, var = quality["c2"][k]
        assert var >= atrous - 2.0, (k, quality["c2"][k])
