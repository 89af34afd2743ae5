"""The numpy restatements of the display post-processing on pixels that are not finite, on the CPU:
what denoise_ref, variance_ref, adaptive_ref, temporal_ref and post_common._unorm8 do with a NaN, an
infinity, an overflowing luminance, a negative, a signed zero and a denormal, pinned on crafted planes
(tests/nonfinite_planes.py) with synthetic guides. tests/test_gpu_nonfinite.py holds the GPU kernels
to these restatements; the set relations asserted here keep those comparisons from being vacuous.

The behaviour pinned is the restatements' docstrings': the filters' `sw > 0` is false for a NaN (the
centre is kept), `d > 0 ? d : 0` is 0 for a NaN, a NaN never wins `v > e ? v : e`, the temporal
resolve's `ok` and `valid` are selects (a valid tap of weight 0 still adds NaN * 0), NaN -> 0 in the
8-bit form.
"""
import numpy as np
import pytest

import adaptive_ref as ar
import denoise_ref as dr
import nonfinite_planes as nf
import temporal_ref as tr
import variance_ref as vr
from post_common import _unorm8, bits, config, same
from opengl_ray_tracing_amd import orbit_camera

F = np.float32
W, H, MISS_COLUMN = 33, 31, 20


def finite_plane(h, w, seed=1):
    c = np.ones((h, w, 4), F)
    c[..., 0:3] = np.random.default_rng(seed).uniform(0.05, 2.0, (h, w, 3))
    return c


@pytest.fixture(scope="module")
def crafted():
    """(plane, guides, record): specials on a flat wall with one column of misses; read-only."""
    g = nf.synthetic_guides(H, W, MISS_COLUMN)
    c, rec = nf.craft(finite_plane(H, W), g)
    c.setflags(write=False)
    return c, g, rec


def changed(a, b):
    """(h, w) bool: the pixel's r, g or b differs (NaN equal to NaN)."""
    return ~same(a[..., 0:3], b[..., 0:3]).all(-1)


def check_centres_kept(c, g, out):
    """The statements of an edge-stopping term that is on: a NaN in it makes every weight it enters
    a NaN, so sw is a NaN and the centre stays."""
    hit = dr.hit_mask(g)
    bad = nf.nonfinite(c)
    assert (bad & hit).sum() >= 5 and (bad & ~hit).sum() >= 1, "the plane holds non-finite hit and miss pixels"
    assert same(out[bad], c[bad]).all(), "a non-finite pixel keeps its centre"
    assert not nf.nonfinite(out)[~bad].any(), "no finite pixel becomes non-finite"
    assert same(out[~hit], c[~hit]).all(), "a miss pixel is copied"
    assert same(out[..., 3], c[..., 3]).all()
    good = hit & ~bad
    n = int(changed(out, c)[good].sum())
    print(f"non-finite pixels {int(bad.sum())} before and after; {n} of {int(good.sum())} finite hit pixels changed")
    assert n > good.sum() // 2, "most finite hit pixels are filtered"


def check_spread(c, g, out):
    """The statements with the term off: the weights are finite, so a non-finite colour enters the sums."""
    hit = dr.hit_mask(g)
    bad = nf.nonfinite(c)
    assert (bad & hit).sum() >= 5 and (bad & ~hit).sum() >= 1, "the plane holds non-finite hit and miss pixels"
    after = nf.nonfinite(out)
    print(f"non-finite pixels {int(bad.sum())} before, {int(after.sum())} of {bad.size} after")
    assert after[hit].sum() > hit.sum() // 2, "the NaN spreads over more than half of the hit pixels"
    assert same(out[~hit], c[~hit]).all(), "and into no miss pixel"
    assert (after & ~bad)[hit].any() and not (after & ~bad)[~hit].any()


# ------------------------------------------------------------------ 1, 2: pt_denoise's restatement
def test_atrous_defaults_keep_the_centre_of_a_non_finite_pixel(crafted):
    c, g, rec = crafted
    check_centres_kept(c, g, dr.atrous(c, g))


def test_atrous_without_the_colour_term_spreads_the_nan(crafted):
    c, g, rec = crafted
    check_spread(c, g, dr.atrous(c, g, sigma_c=0.0))


# ------------------------------------------------------------------ 3: pt_denoise_var's restatement
def test_denoise_var_defaults_and_without_the_luminance_term(crafted):
    c, g, rec = crafted
    out, v0 = vr.denoise_var(c, g, with_variance=True)
    check_centres_kept(c, g, out)
    check_spread(c, g, vr.denoise_var(c, g, sigma_l=0.0))
    # step A: a window that holds a NaN luminance has variance max(NaN, 0) = 0, by the select
    hit = dr.hit_mask(g)
    with np.errstate(all="ignore"):
        lnan = hit & np.isnan(vr.lum_tm(c, 1.5))
    window = nf._grow(lnan, 3) & hit
    assert lnan.sum() >= 5 and (hit & ~window).sum() >= 5
    assert not bits(v0[window]).any(), "+0 where the 7 x 7 window holds a NaN"
    assert np.isfinite(v0).all() and (v0[hit & ~window] > 0).all() and not v0[~hit].any()


# ------------------------------------------------------------------ 4: pt_adaptive_update's restatement
def test_adaptive_update_on_nan_and_infinite_moments():
    """Four tiles of a 32 x 8 image at L = 0 (v = (m2 - m1 m1) / kf): every moment a NaN; one NaN pixel
    among pixels below the threshold; one NaN pixel and one pixel above it; one infinite variance."""
    h, w, frames = 8, 32, 4
    prm = dict(threshold=0.1, limit=1.5, min_frames=4)  # thr2 = 0.01
    acc = np.zeros((h, w, 4), F)
    m = np.zeros((h, w, 2), F)
    m[..., 1] = F(0.004)                # v = 0.001
    m[:, 0:8] = np.nan
    m[3, 12] = (np.nan, np.nan)
    m[3, 20] = (np.nan, np.nan)
    m[6, 17, 1] = F(0.4)                # v = 0.1
    m[2, 29, 1] = np.inf
    e0, a0 = np.zeros((1, 4), F), np.zeros((1, 4), np.uint32)
    e, at = ar.update(e0, a0, acc, m, frames, prm)
    assert np.array_equal(bits(e), bits(np.array([[0, F(0.004) / F(4), F(0.4) / F(4), np.inf]], F)))
    assert np.array_equal(at, np.array([[4, 4, 0, 0]], np.uint32))
    # before min_frames nothing retires, the all-NaN tile included; an infinite variance never does
    e1, a1 = ar.update(e0, a0, acc, m, frames, {**prm, "min_frames": 5})
    assert np.array_equal(bits(e1), bits(e)) and not a1.any()
    e2, a2 = ar.update(e0, a0, acc, m, frames, {**prm, "threshold": 1e18})
    assert np.array_equal(a2, np.array([[4, 4, 4, 0]], np.uint32)) and np.isinf(e2[0, 3])
    # a NaN accumulation: gd is a NaN, so is v, and the pixel never wins either
    acc[5, 18, 0] = np.nan
    m[5, 18, 1] = F(40.0)
    assert np.array_equal(bits(ar.update(e0, a0, acc, m, frames, prm)[0]), bits(e))


# ------------------------------------------------------------------ 5: pt_temporal_resolve's restatement
def wall(w, h, eye, rot, n):
    """Guide planes of the camera's view of the plane through the origin with normal n, every pixel a hit."""
    rays = dr.camera_rays(w, h, eye, rot)
    o, d = rays[:, 0:3], rays[:, 3:6]
    t = (-(o @ n) / (d @ n)).astype(F)
    g = nf.synthetic_guides(h, w)
    g["pos_t"][..., 0:3] = (o + d * t[:, None]).astype(F).reshape(h, w, 3)
    g["pos_t"][..., 3] = t.reshape(h, w)
    g["nrm_tri"][..., 0:3] = n
    return g


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_temporal_resolve_carries_a_history_nan_through_its_valid_taps(delta):
    """A wall seen by the history camera and by one `delta` degrees on (0: the projection lands on
    pixel centres, so three of the four taps weigh exactly 0)."""
    w, h, frames = W, H, 2
    angle, up, rad = config("c2")[0].camera
    eyeA, rotA = orbit_camera(angle, up, rad)
    eyeB, rotB = orbit_camera(angle + delta, up, rad)
    n = (np.asarray(eyeA, F) / F(np.linalg.norm(eyeA))).astype(F)
    gA, gB = wall(w, h, eyeA, rotA, n), wall(w, h, eyeB, rotB, n)
    histc = finite_plane(h, w, 2)
    histc[..., 3] = F(frames)
    c = finite_plane(h, w, 3)
    qy, qx = 12, 17
    clean = tr.resolve(c, frames, gB, tr.commit(histc, gA, eyeA, rotA))
    assert np.isfinite(clean).all() and (clean[..., 3] > frames).sum() > w * h // 2
    kept = histc[qy, qx, 1]
    histc[qy, qx, 1] = np.nan
    out = tr.resolve(c, frames, gB, tr.commit(histc, gA, eyeA, rotA))
    # the pixels whose 2 x 2 taps hold (qx, qy): from the documented projection alone
    fx, fy, cz = tr.project(gB["pos_t"][..., 0:3], eyeA, rotA, w, h)
    ok = (cz < 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
    ix, iy = np.floor(fx), np.floor(fy)
    taps = ok & ((ix == qx) | (ix + 1 == qx)) & ((iy == qy) | (iy + 1 == qy))
    zero = taps & (((ix + 1 == qx) & (fx == ix)) | ((iy + 1 == qy) & (fy == iy)))  # the tap's weight is 0
    print(f"delta {delta:g}: {int(taps.sum())} pixels take the NaN tap, {int(zero.sum())} of them with weight 0")
    assert taps.sum() >= 4 and (delta != 0.0 or zero.sum() >= 3)
    assert np.array_equal(nf.nonfinite(out), taps)
    assert same(out[~taps], clean[~taps]).all()
    # a NaN of the current accumulation stays where it is
    histc[qy, qx, 1] = kept
    c[7, 9, 0] = np.nan
    c[20, 30, 2] = np.inf
    out = tr.resolve(c, frames, gB, tr.commit(histc, gA, eyeA, rotA))
    here = np.zeros((h, w), bool)
    here[7, 9] = here[20, 30] = True
    assert np.array_equal(nf.nonfinite(out), here)
    assert np.isnan(out[7, 9, 0]) and np.isfinite(out[7, 9, 1:]).all() and out[20, 30, 2] == np.inf
    assert same(out[~here], clean[~here]).all()


# ------------------------------------------------------------------ 6: the 8-bit form
def test_unorm8_of_the_special_values():
    x = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 1e-41, 2.0, 0.5, 1.0], F)
    assert _unorm8(x).tolist() == [0, 255, 0, 0, 0, 0, 255, 128, 255]
