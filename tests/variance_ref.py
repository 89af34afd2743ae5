"""float32 numpy restatement of the per-pixel sample moments and the variance-guided a-trous
filter (include/pt_abi.h PT_FLAG_MOMENTS / pt_denoise_var) -- TEST INFRASTRUCTURE, and the
specification: csrc/pt_display.hip (mixFrames) and csrc/pt_variance.hip mirror every operation below in the
same order, so the GPU output equals this file's bit for bit (no fused multiply-adds, + - * / sqrt
correctly rounded, the one transcendental include/pt_fmath.h ptm_expf through denoise_ref.expf).

Every array is float32; rows are pixels in image order (row 0 = the bottom row), colour planes are
(h, w, 4), the moments (h, w, 2) = (m1, m2), a variance plane (h, w). lum(c) = (0.3 r + 0.6 g) + 0.1 b
and tm(c) are pt_tonemap's (denoise_ref.tm). "max(x, 0)" below is the select x > 0 ? x : 0 (0 for
NaN) and max(a, b) is a > b ? a : b.

Moments: sample f of a running mean that holds frameCounter + f frames, l = lum(sample colour):
      w = 1 / (float)(frameCounter + f + 1);  m1 = mixf(m1, l, w);  m2 = mixf(m2, l l, w)
  with mixf(x, y, a) = x (1 - a) + y a, the accumulation's own update.

Filter (Schied et al. 2017, "Spatiotemporal Variance-Guided Filtering", the spatial part):
Step A, the variance v of the tone-mapped luminance of the input c; a miss pixel 0; kf = (float)frames
of the moments:
  temporal (moments given and kf >= min_temporal):
      L = lum(c_p);  q = 1 + L / limit;  gd = 1 / (q q);  n_p = max(c_p.w, kf)
      v = (max(m2 - m1 m1, 0) / n_p) (gd gd)
  spatial: over the 7 x 7 window q = p + (dx, dy), dy = -3..3 outer, dx = -3..3 inner, the pixels that
      are inside the image and hits: l_q = lum(tm(c_q)); s1 += l_q; s2 += l_q l_q; cnt += 1 (a pixel
      that takes no part adds +0 to each)
      v = max(s2 / cnt - (s1 / cnt) (s1 / cnt), 0)
Step B, pass i = 0 .. passes-1, s = 2^i, inputs c and v, l = lum(tm(c)): a miss pixel copies c and v;
a hit pixel p:
      vt_p = sum(v_q g) / sum(g) over the 3 x 3 window q = p + (dx, dy), dy = -1..1 outer, dx = -1..1
             inner, g = G[|dx|] G[|dy|], G = {0.5, 0.25}, of the pixels inside the image that are hits
      lden = sigma_l sqrt(vt_p) + 1e-6
  and the taps q = p + s (dx, dy) of denoise_ref.atrous_pass, with its k and n:
      a = |Np.(Pq - Pp)| / (sigma_z t_p) + |l_q - l_p| / lden + |Aq - Ap|^2 / (sigma_a sigma_a)
      w = (k n) expf(-a)   (0, with colour 0 and variance 0, outside the image or on a miss pixel)
      sw += w;  sum += c_q w;  sv += v_q (w w)
  out.rgb = sum / sw and v_out = sv / (sw sw) when sw > 0 (false for NaN), else c_p.rgb and v_p;
  out.w = c_p.w. sigma_l is the same in every pass: the propagated variance shrinks instead.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import H3, _dot, _shift, expf, hit_mask, tm

F = np.float32
G2 = (F(0.5), F(0.25))
DEFAULTS = dict(passes=5, sigma_l=4.0, sigma_z=0.02, sigma_a=0.2, normal_log2=6, limit=1.5, min_temporal=8)


def lum(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c, F)
    return (F(0.3) * c[..., 0] + F(0.6) * c[..., 1]) + F(0.1) * c[..., 2]


def mixf(x, y, a):
    return x * (F(1) - a) + y * a


def mix_sample(acc: np.ndarray, sample: np.ndarray, count: int) -> np.ndarray:
    """The accumulation's update with one sample colour plane (h, w, >= 3) when it holds `count` frames."""
    w = F(1) / F(count + 1)
    out = np.empty(acc.shape[:2] + (4,), F)
    out[..., 0:3] = mixf(np.asarray(acc, F)[..., 0:3], np.asarray(sample, F)[..., 0:3], w)
    out[..., 3] = F(1)
    return out


def moments_update(m: np.ndarray, sample: np.ndarray, count: int) -> np.ndarray:
    """The moments (h, w, 2) after one more sample colour plane when they hold `count` frames."""
    w = F(1) / F(count + 1)
    l = lum(sample)
    with np.errstate(all="ignore"):
        return np.stack([mixf(m[..., 0], l, w), mixf(m[..., 1], l * l, w)], -1).astype(F)


def moments(samples, frame_counter: int = 0, m=None) -> np.ndarray:
    """The moments after the sample colour planes `samples` (frames frame_counter, frame_counter + 1, ...)."""
    for f, s in enumerate(samples):
        if m is None:
            m = np.zeros(np.asarray(s).shape[:2] + (2,), F)
        m = moments_update(m, s, frame_counter + f)
    return m


def lum_tm(c: np.ndarray, limit) -> np.ndarray:
    return lum(tm(c, limit))


def initial_variance(c, g, m=None, frames: int = 0, limit=1.5, min_temporal=8) -> np.ndarray:
    """Step A -> (h, w)."""
    c = np.ascontiguousarray(c, F)
    hit = hit_mask(g)
    kf = F(frames)
    with np.errstate(all="ignore"):
        if m is not None and kf >= F(min_temporal):
            L = lum(c)
            q = F(1) + L / F(limit)
            gd = F(1) / (q * q)
            n = np.where(c[..., 3] > kf, c[..., 3], kf).astype(F)
            d = m[..., 1] - m[..., 0] * m[..., 0]
            d = np.where(d > F(0), d, F(0)).astype(F)
            v = (d / n) * (gd * gd)
        else:
            l = lum_tm(c, limit)
            pad = 3
            l_ = np.pad(l, pad)
            h_ = np.pad(hit, pad)
            s1 = np.zeros(l.shape, F)
            s2 = np.zeros(l.shape, F)
            cnt = np.zeros(l.shape, F)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    valid = _shift(h_, pad, dx, dy)
                    lq = np.where(valid, _shift(l_, pad, dx, dy), F(0)).astype(F)
                    s1 = s1 + lq
                    s2 = s2 + lq * lq
                    cnt = cnt + np.where(valid, F(1), F(0)).astype(F)
            mu = s1 / cnt
            d = s2 / cnt - mu * mu
            v = np.where(d > F(0), d, F(0)).astype(F)
        return np.where(hit, v, F(0)).astype(F)


def prefilter(v: np.ndarray, hit: np.ndarray) -> np.ndarray:
    """vt: the 3 x 3 mean of v over the hit pixels inside the image (meaningful at hit pixels)."""
    v_ = np.pad(np.asarray(v, F), 1)
    h_ = np.pad(hit, 1)
    sg = np.zeros(v.shape, F)
    sv = np.zeros(v.shape, F)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                valid = _shift(h_, 1, dx, dy)
                gq = np.where(valid, G2[abs(dx)] * G2[abs(dy)], F(0)).astype(F)
                vq = np.where(valid, _shift(v_, 1, dx, dy), F(0)).astype(F)
                sg = sg + gq
                sv = sv + vq * gq
        return sv / sg


def var_pass(c, v, g, s: int, sigma_l, sigma_z, sigma_a, normal_log2: int, limit):
    """One pass at tap stride s of colour plane c (h, w, 4) and variance plane v (h, w) -> (out, v_out)."""
    c = np.ascontiguousarray(c, F)
    v = np.ascontiguousarray(v, F)
    hit = hit_mask(g)
    P, tp = g["pos_t"][..., 0:3], g["pos_t"][..., 3]
    N, A = g["nrm_tri"][..., 0:3], g["albedo"][..., 0:3]
    l = lum_tm(c, limit)
    pad = 2 * s
    pw = ((pad, pad), (pad, pad), (0, 0))
    cq_ = np.pad(c[..., 0:3], pw)
    Pq_, Nq_, Aq_ = np.pad(P, pw), np.pad(N, pw), np.pad(A, pw)
    lq_, vq_ = np.pad(l, pad), np.pad(v, pad)
    hq_ = np.pad(hit, pad)
    sw = np.zeros(c.shape[:2], F)
    sm = np.zeros(c.shape[:2] + (3,), F)
    sv = np.zeros(c.shape[:2], F)
    sl, sz, sa = F(sigma_l), F(sigma_z), F(sigma_a)
    with np.errstate(all="ignore"):
        zden = sz * tp
        aden = sa * sa
        if sl > 0:
            lden = sl * np.sqrt(prefilter(v, hit)) + F(1e-6)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = s * dx, s * dy
                valid = _shift(hq_, pad, ox, oy)
                k = H3[abs(dx)] * H3[abs(dy)]
                if normal_log2 >= 0:
                    Nq = _shift(Nq_, pad, ox, oy)
                    d = _dot(N[..., 0], N[..., 1], N[..., 2], Nq[..., 0], Nq[..., 1], Nq[..., 2])
                    n = np.where(d > F(0), d, F(0)).astype(F)
                    for _ in range(normal_log2):
                        n = n * n
                else:
                    n = np.ones(c.shape[:2], F)
                a = np.zeros(c.shape[:2], F)
                if sz > 0:
                    D = _shift(Pq_, pad, ox, oy) - P
                    a = a + np.abs(_dot(N[..., 0], N[..., 1], N[..., 2], D[..., 0], D[..., 1], D[..., 2])) / zden
                if sl > 0:
                    a = a + np.abs(_shift(lq_, pad, ox, oy) - l) / lden
                if sa > 0:
                    D = _shift(Aq_, pad, ox, oy) - A
                    a = a + _dot(D[..., 0], D[..., 1], D[..., 2], D[..., 0], D[..., 1], D[..., 2]) / aden
                wgt = (k * n) * expf(-a)
                wgt = np.where(valid, wgt, F(0)).astype(F)
                cq = np.where(valid[..., None], _shift(cq_, pad, ox, oy), F(0)).astype(F)
                vq = np.where(valid, _shift(vq_, pad, ox, oy), F(0)).astype(F)
                sw = sw + wgt
                sm = sm + cq * wgt[..., None]
                sv = sv + vq * (wgt * wgt)
        use = hit & (sw > F(0))
        out = c.copy()
        out[..., 0:3] = np.where(use[..., None], sm / sw[..., None], c[..., 0:3])
        v_out = np.where(use, sv / (sw * sw), v).astype(F)
    return out, v_out


def denoise_var(c, g, m=None, frames: int = 0, passes=5, sigma_l=4.0, sigma_z=0.02, sigma_a=0.2, normal_log2=6,
                limit=1.5, min_temporal=8, with_variance=False):
    """pt_denoise_var of colour plane c (h, w, 4) with the guide planes g, the moments m (h, w, 2; None:
    a context without them) and their frame count. -> out, or (out, step A's variance)."""
    out = np.ascontiguousarray(c, F)
    v0 = initial_variance(out, g, m, frames, limit, min_temporal)
    v = v0
    for i in range(passes):
        out, v = var_pass(out, v, g, 1 << i, sigma_l, sigma_z, sigma_a, normal_log2, limit)
    return (out, v0) if with_variance else out
