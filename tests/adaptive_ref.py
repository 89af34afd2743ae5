"""float32 numpy restatement of adaptive sampling's decision (include/pt_abi.h PT_FLAG_ADAPTIVE /
pt_adaptive_update) -- TEST INFRASTRUCTURE, and the specification: csrc/pt_adaptive.hip
(tileErrorKernel) mirrors every operation below in the same order, so the GPU's err2 and retired_at
equal this file's bit for bit (no fused multiply-adds, + - * / correctly rounded).

Every array is float32 unless said; the accumulation is (h, w, 4), the moments (h, w, 2) = (m1, m2),
rows in image order (row 0 = the bottom row). The tile planes are (tilesY, tilesX), tilesX =
(w + 7) // 8: tile (tx, ty) holds the pixels (8 tx .. 8 tx + 7, 8 ty .. 8 ty + 7) inside the image;
err2 is float32, retired_at uint32 (0: active).

One update, with kf = (float)frames of the moments and thr2 = threshold * threshold, for every tile
that is not retired, over its pixels (variance_ref.initial_variance's temporal expression with
n_p = kf and no guides):
      L = lum(acc);  q = 1 + L / limit;  gd = 1 / (q q)
      d = m2 - m1 m1;  d = d > 0 ? d : 0;  v = (d / kf) (gd gd)
      err2[T] = e, from e = 0:  e = v > e ? v : e   (a NaN never wins, so the order does not matter)
      frames >= min_frames and err2[T] <= thr2:  retired_at[T] = frames
A tile retired earlier keeps both. Rendering: a retired tile's pixels take no further sample -- their
accumulation and moments stay as they were at the update that retired the tile; every other pixel's
are variance_ref's mix_sample / moments_update of every frame.
"""
from __future__ import annotations

import numpy as np

from variance_ref import lum, mix_sample, moments_update

F = np.float32
DEFAULTS = dict(threshold=1 / 255, limit=1.5, min_frames=16)


def tiles_of(h: int, w: int):
    return (h + 7) // 8, (w + 7) // 8


def pixel_variance(acc, m, frames: int, limit) -> np.ndarray:
    """v per pixel -> (h, w)."""
    acc = np.asarray(acc, F)
    m = np.asarray(m, F)
    kf = F(frames)
    with np.errstate(all="ignore"):
        L = lum(acc)
        q = F(1) + L / F(limit)
        gd = F(1) / (q * q)
        d = m[..., 1] - m[..., 0] * m[..., 0]
        d = np.where(d > F(0), d, F(0)).astype(F)
        return ((d / kf) * (gd * gd)).astype(F)


def tile_error(acc, m, frames: int, limit) -> np.ndarray:
    """err2 of every tile as an update that finds it active computes it -> (tilesY, tilesX)."""
    v = pixel_variance(acc, m, frames, limit)
    h, w = v.shape
    ty, tx = tiles_of(h, w)
    pad = np.zeros((8 * ty, 8 * tx), F)  # a pixel outside the image leaves e as it is: v = 0 does the same
    pad[:h, :w] = v
    t = pad.reshape(ty, 8, tx, 8)
    e = np.zeros((ty, tx), F)
    with np.errstate(all="ignore"):
        for y in range(8):
            for x in range(8):
                vq = t[:, y, :, x]
                e = np.where(vq > e, vq, e).astype(F)
    return e


def update(err2, retired_at, acc, m, frames: int, prm=None):
    """One pt_adaptive_update -> (err2, retired_at), new arrays."""
    P = {**DEFAULTS, **(prm or {})}
    thr = F(P["threshold"])
    thr2 = thr * thr
    active = np.asarray(retired_at) == 0
    e = tile_error(acc, m, frames, P["limit"])
    err2 = np.where(active, e, np.asarray(err2, F)).astype(F)
    with np.errstate(all="ignore"):
        retire = active & (frames >= int(P["min_frames"])) & (err2 <= thr2)
    retired_at = np.where(retire, np.uint32(frames), np.asarray(retired_at, np.uint32)).astype(np.uint32)
    return err2, retired_at


def pixel_mask(retired_at, h: int, w: int) -> np.ndarray:
    """(h, w) bool: the pixel's tile is retired."""
    return np.repeat(np.repeat(np.asarray(retired_at) != 0, 8, 0), 8, 1)[:h, :w]


def run(samples, update_every: int, prm=None, updates_at=None):
    """The samples (frame k's colour plane, k = 0 ..) rendered in order with an update after every
    update_every frames (or after the frame counts in updates_at) -> dict: acc, m, err2, retired_at,
    counts (retired tiles after each update), max_err2 (over the active tiles after each update),
    history (after each update: copies of acc, m, err2, retired_at), active (per frame: the (h, w)
    bool plane of the pixels that took the frame's sample)."""
    P = {**DEFAULTS, **(prm or {})}
    h, w = np.asarray(samples[0]).shape[:2]
    ty, tx = tiles_of(h, w)
    acc = np.zeros((h, w, 4), F)
    m = np.zeros((h, w, 2), F)
    err2 = np.zeros((ty, tx), F)
    at = np.zeros((ty, tx), np.uint32)
    counts, max_err2, history, active = [], [], [], []
    when = set(updates_at) if updates_at is not None else {k for k in range(update_every, len(samples) + 1, update_every)}
    for k, s in enumerate(samples):
        gone = pixel_mask(at, h, w)
        active.append(~gone)
        acc = np.where(gone[..., None], acc, mix_sample(acc, s, k)).astype(F)
        m = np.where(gone[..., None], m, moments_update(m, s, k)).astype(F)
        if k + 1 in when:
            err2, at = update(err2, at, acc, m, k + 1, P)
            counts.append(int((at != 0).sum()))
            live = err2[at == 0]
            max_err2.append(F(live.max()) if live.size else F(0))
            history.append((acc.copy(), m.copy(), err2.copy(), at.copy()))
    return dict(acc=acc, m=m, err2=err2, retired_at=at, counts=counts, max_err2=max_err2, history=history,
                active=active)
