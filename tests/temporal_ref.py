"""float32 numpy restatement of the temporal resolve (include/pt_abi.h pt_temporal_resolve /
pt_temporal_commit) -- TEST INFRASTRUCTURE, and the specification: csrc/pt_temporal.hip mirrors
every operation below in the same order, so the GPU output equals this file's bit for bit (the build
keeps fused multiply-adds off on both sides; + - * / and floor are correctly rounded / exact; there
is no transcendental).

Every array is float32; planes are (h, w, 4), row 0 = the bottom row, like the accumulation and the
guide planes of tests/denoise_ref.py.

The scene is static, so the first-hit position Pp a pixel's guide holds projects straight into the
previous (history) camera E', M' -- the inverse of denoise_ref.camera_rays: with c0 = M'[0..2],
c1 = M'[4..6], c2 = M'[8..10] a camera ray is d ~ x c0 + y c1 - 1.5 c2, so for v = Pp - E'
    a = c0.v, b = c1.v, cz = c2.v;  s = -1.5 / cz;  x = a s, y = b s
    fx = (x + 1) (0.5 W) - 0.5, fy = (y + 1) (0.5 H) - 0.5        (pixel centres at integers)
Per pixel p (c the accumulation, kf = (float)frames):
    out = (c.rgb, kf)
    with a history, for a hit pixel:
      ok = cz < 0 and -1 < fx < W and -1 < fy < H                  (false for NaN)
      (ix, iy) = floor(fx, fy), (tx, ty) = the fractions
      the taps q = (ix + i, iy + j), j = 0, 1 outer, i = 0, 1 inner, wt = (i ? tx : 1 - tx) (j ? ty : 1 - ty),
      valid = ok and q inside the image and a hit of the history and hist[q].w > 0
              and |Np.(Pq - Pp)| <= sigma_z t_p and Np.Nq >= normal_cos
      wv = valid ? wt : 0;  sw += wv;  sum += (valid ? hist[q].rgb : 0) wv;  sn += (valid ? hist[q].w : 0) wv
      ok and sw > 0:  hc = sum / sw;  n = min(sn / sw, max_history);  wgt = kf / (n + kf)
                      out = (hc (1 - wgt) + c.rgb wgt, n + kf)
A miss pixel shows the environment texel directly, so it takes no history.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import _dot, hit_mask

F = np.float32
DEFAULTS = dict(sigma_z=0.02, normal_cos=0.9, max_history=32.0)


def project(P: np.ndarray, eye, rot, w: int, h: int):
    """Positions P (..., 3) in the camera (eye, rot) -> (fx, fy, cz): continuous pixel coordinates
    (a pixel's centre at its integer index) and the camera-space depth term (< 0 in front)."""
    M = np.ascontiguousarray(rot, F).reshape(16)
    E = np.ascontiguousarray(eye, F).reshape(3)
    P = np.asarray(P, F)
    with np.errstate(all="ignore"):
        vx, vy, vz = P[..., 0] - E[0], P[..., 1] - E[1], P[..., 2] - E[2]
        a = _dot(M[0], M[1], M[2], vx, vy, vz)
        b = _dot(M[4], M[5], M[6], vx, vy, vz)
        cz = _dot(M[8], M[9], M[10], vx, vy, vz)
        s = F(-1.5) / cz
        x = a * s
        y = b * s
        fx = (x + F(1)) * (F(0.5) * F(w)) - F(0.5)
        fy = (y + F(1)) * (F(0.5) * F(h)) - F(0.5)
    return fx.astype(F), fy.astype(F), cz.astype(F)


def commit(resolved: np.ndarray, g: dict, eye, rot) -> dict:
    """pt_temporal_commit: the resolved image, the guides' pos_t / nrm_tri and their camera."""
    return {"rgba": np.array(resolved, F), "pos_t": np.array(g["pos_t"], F), "nrm_tri": np.array(g["nrm_tri"], F),
            "eye": np.array(eye, F).reshape(3), "rot": np.array(rot, F).reshape(16)}


def resolve(c, frames: int, g: dict, hist: dict | None, sigma_z=0.02, normal_cos=0.9, max_history=32.0) -> np.ndarray:
    """pt_temporal_resolve of the accumulation c (h, w, 4) holding `frames` frames, with the guide
    planes g of its camera and the committed history (None: no history) -> (h, w, 4), .w = count."""
    c = np.ascontiguousarray(c, F)
    h, w = c.shape[:2]
    kf = F(frames)
    out = c.copy()
    out[..., 3] = kf
    if hist is None:
        return out
    sz, nc, mh = F(sigma_z), F(normal_cos), F(max_history)
    hit = hit_mask(g)
    Pp, tp = g["pos_t"][..., 0:3], g["pos_t"][..., 3]
    Np = g["nrm_tri"][..., 0:3]
    H4, HP, HN = hist["rgba"], hist["pos_t"], hist["nrm_tri"]
    hhit = HN[..., 3].view(np.int32) >= 0
    with np.errstate(all="ignore"):
        fx, fy, cz = project(Pp, hist["eye"], hist["rot"], w, h)
        ok = (cz < F(0)) & (fx > F(-1)) & (fx < F(w)) & (fy > F(-1)) & (fy < F(h))
        gx = np.where(ok, fx, F(0)).astype(F)
        gy = np.where(ok, fy, F(0)).astype(F)
        flx, fly = np.floor(gx), np.floor(gy)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = gx - flx, gy - fly
        zt = sz * tp
        sw = np.zeros((h, w), F)
        sn = np.zeros((h, w), F)
        sm = np.zeros((h, w, 3), F)
        for j in range(2):
            wy = ty if j else F(1) - ty
            for i in range(2):
                wt = (tx if i else F(1) - tx) * wy
                qx, qy = ix + i, iy + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                hq, Pq, Nq = H4[cy, cx], HP[cy, cx, 0:3], HN[cy, cx, 0:3]
                D = Pq - Pp
                plane = np.abs(_dot(Np[..., 0], Np[..., 1], Np[..., 2], D[..., 0], D[..., 1], D[..., 2])) <= zt
                nrm = _dot(Np[..., 0], Np[..., 1], Np[..., 2], Nq[..., 0], Nq[..., 1], Nq[..., 2]) >= nc
                valid = ok & inside & hhit[cy, cx] & (hq[..., 3] > F(0)) & plane & nrm
                wv = np.where(valid, wt, F(0)).astype(F)
                hc = np.where(valid[..., None], hq[..., 0:3], F(0)).astype(F)
                hn = np.where(valid, hq[..., 3], F(0)).astype(F)
                sw = sw + wv
                sm = sm + hc * wv[..., None]
                sn = sn + hn * wv
        use = hit & ok & (sw > F(0))
        hc = sm / sw[..., None]
        n = sn / sw
        n = np.where(n < mh, n, mh).astype(F)
        wgt = kf / (n + kf)
        rgb = hc * (F(1) - wgt)[..., None] + c[..., 0:3] * wgt[..., None]
        out[..., 0:3] = np.where(use[..., None], rgb, c[..., 0:3])
        out[..., 3] = np.where(use, n + kf, kf)
    return out
