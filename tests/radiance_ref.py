"""What the radiance query is specified against (include/pt_abi.h pt_radiance_device,
pt_camera_rays_device) -- TEST INFRASTRUCTURE: the frame kernels' jittered camera rays restated in
float32 numpy, the default ray ids, and the oracle's single samples. Helpers only, no tests.

The contract under test: a ray that is bit for bit the camera ray of pixel (px, py) of sample s yields
that frame's sample of the pixel bit for bit, so the reference of every radiance test is the oracle's
frame (oracle/pt_oracle.c), sample by sample.
"""
from __future__ import annotations

import numpy as np

import oracle

F = np.float32
MISS_T = F(2147483648.0)


def jitter_draws(w: int, h: int, sample_index: int) -> np.ndarray:
    """(h * w, 2): the first two random draws of every pixel's seed, pixel (px, py) at row py * w + px."""
    return np.stack([oracle.pixel_rng(px, py, sample_index & 0xFFFFFFFF, 2) for py in range(h) for px in range(w)]).astype(F)


def camera_rays(w: int, h: int, eye, rot, sample_index: int, draws=None) -> np.ndarray:
    """pt_frame.h cameraRay of sample `sample_index` for every pixel of a w x h image: denoise_ref.camera_rays
    with the jitter ax = (r0 - 0.5) / W, ay = (r1 - 0.5) / H, (r0, r1) the pixel's first two draws (`draws`
    replaces them); every operation one f32 operation in cameraDir's order.
    -> (h * w, 6) origin, direction; pixel (px, py) at row py * w + px."""
    M = np.ascontiguousarray(rot, F).reshape(16)
    r = jitter_draws(w, h, sample_index) if draws is None else np.ascontiguousarray(draws, F).reshape(-1, 2)
    px = np.tile(np.arange(w, dtype=np.int64), h)
    py = np.repeat(np.arange(h, dtype=np.int64), w)
    ax = (r[:, 0] - F(0.5)) / F(w)
    ay = (r[:, 1] - F(0.5)) / F(h)
    pixx = (2 * px + 1).astype(F) / F(w) - F(1)
    pixy = (2 * py + 1).astype(F) / F(h) - F(1)
    x = pixx + ax
    y = pixy + ay
    z = F(-1.5)
    d = [(M[0 + k] * x + M[4 + k] * y) + (M[8 + k] * z + M[12 + k] * F(0)) for k in range(3)]
    inv = F(1) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    rays = np.empty((w * h, 6), F)
    e = np.ascontiguousarray(eye, F).reshape(3)
    for k in range(3):
        rays[:, k] = e[k]
        rays[:, 3 + k] = d[k] * inv
    return rays


def pixel_ids(w: int, h: int) -> np.ndarray:
    """(h * w, 2) int32: (px, py) row-major, the ids pt_camera_rays_device writes."""
    return np.stack([np.tile(np.arange(w), h), np.repeat(np.arange(h), w)], axis=1).astype(np.int32)


def default_ids(n: int) -> np.ndarray:
    """(n, 2) int32: the id of ray k when none is given, (k & 4095, k >> 12)."""
    k = np.arange(n, dtype=np.int64)
    return np.stack([k & 4095, k >> 12], axis=1).astype(np.int32)


def pixel_seed(ids, sample_index: int) -> np.ndarray:
    """pass1.fsh main's seed of each id, uint32."""
    i = np.asarray(ids).astype(np.uint64)
    return (((i[:, 0] * 1973 + i[:, 1] * 9277 + (sample_index & 0xFFFFFFFF) * 26699) & 0xFFFFFFFF) | 1).astype(np.uint32)


def oracle_sample(orc, w: int, h: int, integ, mb: int, eye, rot, s: int) -> np.ndarray:
    """The oracle's sample s alone, (h, w, 4): frame 0 of sample rank s of a world larger than s on a zero
    accumulation, so its weight is 1 and its sample index s (as tests/adaptive_common.py samples)."""
    out, _ = orc.render(w, h, integ, 0, eye, rot, accum=np.zeros((h, w, 4), F), max_bounce=mb, sample_rank=s,
                        sample_world=s + 1)
    return out
