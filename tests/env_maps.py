"""Small environment maps at the edges of the env-map path (test infrastructure, shared by
tests/test_hdr.py and tests/test_gpu_env.py): generated from seeds, every texel RGBE-exact as a
decoded Radiance file's is, so pt_upload_env keeps its compact forms for them.

Sizes are width x height; an image is (height, width, 3) float32.
"""
from __future__ import annotations

import numpy as np


def rgbe_quantise(img) -> np.ndarray:
    """Each texel as an RGBE texel holds it: floor(c * 2^(136 - E)) * 2^(E - 136), E the shared
    exponent byte of the largest channel m (m = f * 2^(E - 128), f in [0.5, 1)); a black texel stays black."""
    img = np.asarray(img, np.float32)
    mx = img.max(axis=-1, keepdims=True)
    _, ex = np.frexp(mx)
    e = ex.astype(np.int32) + 128
    assert ((e >= 0) & (e <= 255))[mx > 0].all()
    up = np.ldexp(np.float32(1), 136 - e).astype(np.float32)
    down = np.ldexp(np.float32(1), e - 136).astype(np.float32)
    q = np.floor(img * up) * down
    return np.where(mx > 0, q, np.float32(0)).astype(np.float32)


def same_bits_or_nan(a, b) -> bool:
    """Equal bit for bit, a NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def random_map(w: int, h: int, seed: int) -> np.ndarray:
    """Channels log-uniform over 2^-6 .. 2^3 (ten RGBE exponents), a few of them zero."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-6, 3, (h, w, 3)))
    img[rng.random((h, w, 3)) < 0.05] = 0.0
    return rgbe_quantise(img)


def constant_map(w: int, h: int) -> np.ndarray:
    return rgbe_quantise(np.broadcast_to(np.float32([0.75, 0.5, 0.25]), (h, w, 3)))


def hot_texel_map(w: int, h: int) -> np.ndarray:
    img = np.zeros((h, w, 3), np.float32)
    img[h // 3, (2 * w) // 3] = (6.0, 5.0, 7.0)
    return rgbe_quantise(img)


def black_rows_map(w: int, h: int, seed: int) -> np.ndarray:
    """The first two, the last and every third row black."""
    img = random_map(w, h, seed)
    img[0:2] = 0
    img[-1] = 0
    img[4::3] = 0
    return img


def black_columns_map(w: int, h: int, seed: int) -> np.ndarray:
    """The first, the last two and every third column black: zero marginals, whose conditional CDFs
    are NaN."""
    img = random_map(w, h, seed)
    img[:, 0] = 0
    img[:, -2:] = 0
    img[:, 5::3] = 0
    return img


def black_map(w: int, h: int) -> np.ndarray:
    return np.zeros((h, w, 3), np.float32)


# name -> image: the maps of the env-cache tests. 64 x 64 is exactly one chunk of the GPU's serial
# luminance sum (pt_envcache.hip SUM_CHUNK = 4096), 64 x 65 one chunk and a 64-value tail, 241 x 17 and
# 4097 x 1 one chunk and a tail of one value (no multiple of 4), the others less than a chunk
def cache_maps() -> dict:
    m = {f"random {w}x{h}": random_map(w, h, 1000 + w * h)
         for w, h in [(1, 1), (2, 1), (5, 3), (37, 19), (64, 64), (241, 17), (100, 50), (64, 65), (4097, 1)]}
    m["constant 37x19"] = constant_map(37, 19)
    m["hot texel 37x19"] = hot_texel_map(37, 19)
    m["black rows 40x20"] = black_rows_map(40, 20, 7)
    m["black columns 40x20"] = black_columns_map(40, 20, 8)
    m["black 8x4"] = black_map(8, 4)
    return m


CACHE_MAP_NAMES = ["random 1x1", "random 2x1", "random 5x3", "random 37x19", "random 64x64", "random 241x17",
                   "random 100x50", "random 64x65", "random 4097x1", "constant 37x19", "hot texel 37x19",
                   "black rows 40x20", "black columns 40x20", "black 8x4"]
