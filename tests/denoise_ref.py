"""float32 numpy restatement of the guide buffers and the edge-avoiding a-trous filter
(include/pt_abi.h pt_render_guides / pt_denoise) -- TEST INFRASTRUCTURE, and the specification:
csrc/pt_guides.hip and csrc/pt_denoise.hip mirror every operation below in the same order, so the
GPU output equals this file's bit for bit (the build keeps fused multiply-adds off on both sides,
+ - * / sqrt are correctly rounded, and the one transcendental is include/pt_fmath.h ptm_expf,
taken here through pt_fmath_host(5, ...)).

Every array is float32; rows are pixels in image order (row 0 = the bottom row, like the
accumulation), planes are (h, w, 4).

Filter (Dammertz et al. 2010, "Edge-Avoiding A-Trous Wavelet Transform for fast Global
Illumination Filtering"), pass i = 0 .. passes-1, s = 2^i, sc = sigma_c * 2^-i, c = the pass's input:
  a miss pixel is copied; a hit pixel p sums the taps q = p + s (dx, dy), dy = -2..2 outer,
  dx = -2..2 inner, each with
      k = H[|dx|] H[|dy|],  H = {0.375, 0.25, 0.0625}
      n = max(0, Np.Nq) squared normal_log2 times         (1 with the term off)
      a = |Np.(Pq - Pp)| / (sigma_z t_p) + |tm(cq) - tm(cp)|^2 / (sc sc) + |Aq - Ap|^2 / (sigma_a sigma_a)
      w = (k n) expf(-a)
  a tap outside the image or on a miss pixel takes part with w = 0 and colour 0 (adding +0 is exact).
  out.rgb = sum / sw when sw > 0 (false for NaN), else cp.rgb; out.w = cp.w.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

F = np.float32
MISS_T = F(2147483648.0)
H3 = (F(0.375), F(0.25), F(0.0625))
DEFAULTS = dict(passes=5, sigma_c=2.0, sigma_z=0.02, sigma_a=0.2, normal_log2=6, limit=1.5)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def expf(x: np.ndarray) -> np.ndarray:
    """ptm_expf of include/pt_fmath.h, evaluated by the library on the host."""
    from opengl_ray_tracing_amd import _native
    x = np.ascontiguousarray(x, F)
    out = np.empty_like(x)
    fp = C.POINTER(C.c_float)
    rc = _native.load().pt_fmath_host(5, x.ctypes.data_as(fp), None, x.size, out.ctypes.data_as(fp))
    assert rc == 0, rc
    return out


def camera_rays(w: int, h: int, eye, rot) -> np.ndarray:
    """The frame kernels' camera ray (pt_frame.h cameraDir) through each pixel centre: the jitter terms are 0.
    -> (h * w, 6) origin, direction; pixel (px, py) at row py * w + px."""
    M = np.ascontiguousarray(rot, F).reshape(16)
    px = np.tile(np.arange(w, dtype=np.int64), h)
    py = np.repeat(np.arange(h, dtype=np.int64), w)
    pixx = (2 * px + 1).astype(F) / F(w) - F(1)
    pixy = (2 * py + 1).astype(F) / F(h) - F(1)
    x = pixx + F(0)
    y = pixy + F(0)
    z = F(-1.5)
    d = []
    for k in range(3):
        d.append((M[0 + k] * x + M[4 + k] * y) + (M[8 + k] * z + M[12 + k] * F(0)))
    inv = F(1) / np.sqrt(_dot(d[0], d[1], d[2], d[0], d[1], d[2]))
    rays = np.empty((w * h, 6), F)
    e = np.ascontiguousarray(eye, F).reshape(3)
    for k in range(3):
        rays[:, k] = e[k]
        rays[:, 3 + k] = d[k] * inv
    return rays


def finish_hit(tris, rays, t, tri, w: int, h: int):
    """finishHit (pt_trace.h) of the closest hits (t, tri) of `rays` over the uploaded
    Triangle_encoded rows -> the three guide planes {"pos_t", "nrm_tri", "albedo"}, (h, w, 4) f32;
    nrm_tri[..., 3] holds the triangle index's int bits."""
    T = np.ascontiguousarray(tris, F).reshape(-1, 36)
    t = np.asarray(t, F)
    tri = np.asarray(tri, np.int32)
    hit = tri >= 0
    R = T[np.where(hit, tri, 0)]
    o, d = rays[:, 0:3], rays[:, 3:6]
    p1, p2, p3 = R[:, 0:3], R[:, 3:6], R[:, 6:9]
    n1, n2, n3 = R[:, 9:12], R[:, 12:15], R[:, 15:18]
    with np.errstate(all="ignore"):
        # the geometric normal: normalize(cross(p2 - p1, p3 - p1)) (pt_scene_prep.cpp nrm3)
        e1, e2 = p2 - p1, p3 - p1
        cx = e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2]
        cy = e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0]
        cz = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
        ginv = F(1) / np.sqrt((cx * cx + cy * cy) + cz * cz)
        inside = _dot(cx * ginv, cy * ginv, cz * ginv, d[:, 0], d[:, 1], d[:, 2]) > F(0)
        P = o + d * t[:, None]
        eps = F(0.00005)
        Px, Py = P[:, 0], P[:, 1]
        alpha = (-(Px - p2[:, 0]) * (p3[:, 1] - p2[:, 1]) + (Py - p2[:, 1]) * (p3[:, 0] - p2[:, 0])) / \
                (-(p1[:, 0] - p2[:, 0] - eps) * (p3[:, 1] - p2[:, 1] + eps) +
                 (p1[:, 1] - p2[:, 1] + eps) * (p3[:, 0] - p2[:, 0] + eps))
        beta = (-(Px - p3[:, 0]) * (p1[:, 1] - p3[:, 1]) + (Py - p3[:, 1]) * (p1[:, 0] - p3[:, 0])) / \
               (-(p2[:, 0] - p3[:, 0] - eps) * (p1[:, 1] - p3[:, 1] + eps) +
                (p2[:, 1] - p3[:, 1] + eps) * (p1[:, 0] - p3[:, 0] + eps))
        gama = F(1) - alpha - beta
        v = (n1 * alpha[:, None] + n2 * beta[:, None]) + n3 * gama[:, None]
        inv = F(1) / np.sqrt(_dot(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2]))
        Ns = v * inv[:, None]
        N = np.where(inside[:, None], -Ns, Ns)
    pos_t = np.zeros((h * w, 4), F)
    nrm = np.zeros((h * w, 4), F)
    alb = np.zeros((h * w, 4), F)
    pos_t[:, 3] = MISS_T
    pos_t[hit, 0:3] = P[hit]
    pos_t[hit, 3] = t[hit]
    nrm[hit, 0:3] = N[hit]
    nrm[:, 3] = np.where(hit, tri, -1).astype(np.int32).view(F)
    alb[hit, 0:3] = R[hit, 21:24]
    alb[hit, 3] = F(1)
    return {"pos_t": pos_t.reshape(h, w, 4), "nrm_tri": nrm.reshape(h, w, 4), "albedo": alb.reshape(h, w, 4)}


def guides(orc, tris, w: int, h: int, eye, rot):
    """The guide planes of a camera: the oracle's closest hits (oracle.Oracle.trace_closest) of
    the restated camera rays, then finish_hit. -> (planes, rays, t, tri)"""
    rays = camera_rays(w, h, eye, rot)
    t, tri, _ = orc.trace_closest(rays)
    t = np.where(tri >= 0, t, MISS_T).astype(F)
    return finish_hit(tris, rays, t, tri, w, h), rays, t, tri


def hit_mask(g) -> np.ndarray:
    return g["nrm_tri"][..., 3].view(np.int32) >= 0


def tm(c: np.ndarray, limit) -> np.ndarray:
    """pt_tonemap's expression (pass3.fsh:14-24), gamma off, of (..., >= 3) colours -> (..., 3)."""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        lum = (F(0.3) * c[..., 0] + F(0.6) * c[..., 1]) + F(0.1) * c[..., 2]
        s = F(1) / (F(1) + lum / F(limit))
        return c[..., 0:3] * s[..., None]


def _shift(a: np.ndarray, pad: int, ox: int, oy: int) -> np.ndarray:
    """a (padded by `pad` on both image axes) seen from every pixel at offset (ox, oy)."""
    hh, ww = a.shape[0] - 2 * pad, a.shape[1] - 2 * pad
    return a[pad + oy:pad + oy + hh, pad + ox:pad + ox + ww]


def atrous_pass(c, g, s: int, sigma_c, sigma_z, sigma_a, normal_log2: int, limit) -> np.ndarray:
    """One pass at tap stride s of colour plane c (h, w, 4); sigma_c is the pass's own (already halved)."""
    c = np.ascontiguousarray(c, F)
    hit = hit_mask(g)
    P, tp = g["pos_t"][..., 0:3], g["pos_t"][..., 3]
    N, A = g["nrm_tri"][..., 0:3], g["albedo"][..., 0:3]
    T = tm(c, limit)
    pad = 2 * s
    pw = ((pad, pad), (pad, pad), (0, 0))
    cq_ = np.pad(c[..., 0:3], pw)
    Tq_, Pq_, Nq_, Aq_ = np.pad(T, pw), np.pad(P, pw), np.pad(N, pw), np.pad(A, pw)
    vq_ = np.pad(hit, ((pad, pad), (pad, pad)))
    sw = np.zeros(c.shape[:2], F)
    sm = np.zeros(c.shape[:2] + (3,), F)
    sc, sz, sa = F(sigma_c), F(sigma_z), F(sigma_a)
    with np.errstate(all="ignore"):
        zden = sz * tp
        cden = sc * sc
        aden = sa * sa
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = s * dx, s * dy
                valid = _shift(vq_, pad, ox, oy)
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
                if sc > 0:
                    D = _shift(Tq_, pad, ox, oy) - T
                    a = a + _dot(D[..., 0], D[..., 1], D[..., 2], D[..., 0], D[..., 1], D[..., 2]) / cden
                if sa > 0:
                    D = _shift(Aq_, pad, ox, oy) - A
                    a = a + _dot(D[..., 0], D[..., 1], D[..., 2], D[..., 0], D[..., 1], D[..., 2]) / aden
                wgt = (k * n) * expf(-a)
                wgt = np.where(valid, wgt, F(0)).astype(F)
                cq = np.where(valid[..., None], _shift(cq_, pad, ox, oy), F(0)).astype(F)
                sw = sw + wgt
                sm = sm + cq * wgt[..., None]
        use = hit & (sw > F(0))
        out = c.copy()
        out[..., 0:3] = np.where(use[..., None], sm / sw[..., None], c[..., 0:3])
    return out


def atrous(c, g, passes=5, sigma_c=2.0, sigma_z=0.02, sigma_a=0.2, normal_log2=6, limit=1.5) -> np.ndarray:
    """pt_denoise of colour plane c (h, w, 4) with the guide planes g."""
    out = np.ascontiguousarray(c, F)
    for i in range(passes):
        sc = F(sigma_c) * F(2.0 ** -i)
        out = atrous_pass(out, g, 1 << i, sc, sigma_z, sigma_a, normal_log2, limit)
    return out


def psnr_tm(img, ref, mask, limit=1.5) -> float:
    """PSNR (peak 1) of the tone-mapped colours over the pixels of mask, in float64."""
    a = tm(img, limit).astype(np.float64)[mask]
    b = tm(ref, limit).astype(np.float64)[mask]
    mse = np.mean((a - b) ** 2)
    return float(10.0 * np.log10(1.0 / mse))
