"""The specification of pt_update_env's PT_ENV_RGBE quantiser (include/pt_rgbe.h pt_rgbe_quantise) in
float32 numpy, and a restatement of the texel test of pt_envcache.hip envCompactKernel -- TEST
INFRASTRUCTURE ONLY: helpers, no tests (tests/test_env_update_ref.py, tests/test_gpu_env_update.py).

quantise, per texel:
  c   -> c > 0 ? min(c, 255 * 2^119) : 0      negative values, -0 and NaN become 0, +inf the largest RGBE value
  mx   = the largest channel; mx < 1e-32f (Radiance's writer threshold) gives a black texel
  E    = exponent(mx) + 128 (frexp's exponent), 22 .. 255
  c   -> floor(c * 2^(136 - E)) * 2^(E - 136)
  ... and black again if that leaves the largest channel below 1e-32f. 1e-32f is no RGBE value: it lies
  between 207 and 208 * 2^-114, so a largest channel in [1e-32f, 208 * 2^-114) would be stored as
  207 * 2^-114, below the threshold, and a second pass would blacken it. The threshold therefore holds
  for the stored value, which makes the function idempotent; the smallest texel kept is 208 * 2^-114.

It equals env_maps.rgbe_quantise wherever no channel is negative and the largest channel is at least
1e-32f (below that env_maps.rgbe_quantise keeps values, or overflows its scale for E < 9).
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
RGBE_MAX = np.ldexp(F(255), 119).astype(F)  # E = 255, mantissa 255
RGBE_MIN = F(1e-32)
RGBE_KEPT = np.ldexp(F(208), -114).astype(F)  # the smallest largest channel that is kept


def quantise(img) -> np.ndarray:
    img = np.asarray(img, F)
    with np.errstate(invalid="ignore"):
        c = np.where(img > 0, np.minimum(img, RGBE_MAX), F(0)).astype(F)
    mx = c.max(axis=-1, keepdims=True)
    live = mx >= RGBE_MIN
    _, ex = np.frexp(np.where(live, mx, F(1)))
    e = ex.astype(np.int32) + 128
    up = np.ldexp(F(1), 136 - e).astype(F)
    down = np.ldexp(F(1), e - 136).astype(F)
    q = (np.floor(c * up).astype(F) * down).astype(F)
    live &= q.max(axis=-1, keepdims=True) >= RGBE_MIN
    return np.where(live, q, F(0)).astype(F)


def compact_texel_ok(img) -> np.ndarray:
    """envCompactKernel's decision per texel (the colour part): every channel >= 0, the RGBE bytes are
    integers <= 255, and decodeHdr8 of them gives the texel's bits back. -> bool array of img.shape[:-1]."""
    c = np.asarray(img, F)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (c >= 0).all(-1)
        mx = np.fmax(c[..., 0], np.fmax(c[..., 1], c[..., 2]))
        lit = ok & (mx > 0)
        _, ex = np.frexp(np.where(lit, mx, F(1)))
        e = ex.astype(np.int32) + 128
        ok &= ~lit | ((e >= 0) & (e <= 255))
        e = np.clip(e, 0, 255)
        m = (c * np.ldexp(F(1), 136 - e).astype(F)[..., None]).astype(F)
        whole = ((m == np.floor(m)) & (m <= 255)).all(-1)
        ok &= ~lit | whole
        word = np.where((lit & ok)[..., None], m, F(0))
        word = np.where(np.isfinite(word), word, F(0)).astype(np.uint32).astype(F)
        back = (word * np.ldexp(F(1), np.where(lit & ok, e, 0) - 136).astype(F)[..., None]).astype(F)
        ok &= (back.view(np.uint32) == c.view(np.uint32)).all(-1)
    return ok


def _exact(v: float) -> float:
    """The RGBE value of one positive channel that is its texel's largest, in exact float64 arithmetic."""
    _, ex = math.frexp(v)
    return math.floor(v * 2.0 ** (8 - ex)) * 2.0 ** (ex - 8)


_BELOW = np.nextafter(RGBE_MIN, F(0))
_ABOVE = np.nextafter(RGBE_MAX, F(np.inf))
# (texel, what the quantiser must make of it): the documented value of every edge
EDGE_TEXELS = [
    ((-1.0, 0.5, 0.25), (0.0, 0.5, 0.25)),                       # a negative channel
    ((-0.0, -0.0, 0.5), (0.0, 0.0, 0.5)),                        # -0 becomes +0
    ((np.nan, 1.0, np.nan), (0.0, 1.0, 0.0)),                    # NaN
    ((np.inf, 1.0, 0.0), (float(RGBE_MAX), 0.0, 0.0)),           # +inf: the largest value; 1 is below its last bit
    ((1e-45, 0.0, 0.0), (0.0, 0.0, 0.0)),                        # the smallest subnormal
    ((float(_BELOW), float(_BELOW), 0.0), (0.0, 0.0, 0.0)),      # just below the threshold
    ((float(RGBE_MIN), 0.0, 0.0), (0.0, 0.0, 0.0)),              # at it: it would be stored as 207 * 2^-114, below it
    ((float(RGBE_KEPT), 1e-45, 0.0), (float(RGBE_KEPT), 0.0, 0.0)),  # the smallest texel kept, E = 22
    ((float(np.nextafter(RGBE_KEPT, F(1))), 0.0, 0.0), (_exact(float(np.nextafter(RGBE_KEPT, F(1)))), 0.0, 0.0)),
    ((float(RGBE_MAX), float(RGBE_MAX), 0.0), (float(RGBE_MAX), float(RGBE_MAX), 0.0)),
    ((float(_ABOVE), 3.0e38, 2.0 ** 119), (float(RGBE_MAX), float(RGBE_MAX), 2.0 ** 119)),  # above it: clamped
]


def edge_texels():
    """-> (texels (n, 3) f32, expected (n, 3) f32)"""
    return np.array([t for t, _ in EDGE_TEXELS], F), np.array([q for _, q in EDGE_TEXELS], F)


def unquantised_map(w: int, h: int, seed: int) -> np.ndarray:
    """env_maps.random_map's distribution without its rounding: channels log-uniform over 2^-6 .. 2^3, a
    few zero; almost no texel is an RGBE value."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-6, 3, (h, w, 3)))
    img[rng.random((h, w, 3)) < 0.05] = 0.0
    return img.astype(F)
