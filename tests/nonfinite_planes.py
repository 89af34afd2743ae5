"""Colour planes with pixels that are not finite, or extreme, for the tests of the display
post-processing on such pixels (test_nonfinite_ref.py, test_gpu_nonfinite.py): helpers only, no tests
and no fixtures.

The filters read the context's own guide planes, which cannot be injected, so where the special
values go is decided from the guides a camera rendered: craft() takes a finite (h, w, 4) image and
its guide planes and overwrites chosen pixels' channels. The values:
    NaN, +Inf, -Inf, 3e38 (its luminance overflows), -1.0, -0.0, 1e-41 (a denormal)
The placements, each of which craft() asserts to occur:
    row       one whole row with hits and misses: pixel x holds value x % 7 in channel x % 3
    corner    the four image corners (NaN, +Inf in r, -Inf in g, 3e38)
    seam_x    pixels 15 and 16 of one row, seam_y pixels 15 and 16 of one column: both sides of the
              16-pixel tile seam (hit pixels where the guides have such a pair)
    block     a 3 x 3 block of NaN pixels on hits
    interior  hit pixels whose 5 x 5 neighbourhood is all hits
    edge      hit pixels with a miss pixel beside them (left, right, below or above)
    miss      miss pixels
    isolated  the pixels of the last three kinds: each is placed at least 3 pixels (Chebyshev) from
              every other special pixel, so its 5 x 5 neighbourhood holds no other
The last three kinds take up to seven pixels each, one per value in the order above, all of r, g, b.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import MISS_T, hit_mask

F = np.float32
SPECIALS = (("nan", F(np.nan)), ("+inf", F(np.inf)), ("-inf", F(-np.inf)), ("3e38", F(3e38)), ("-1", F(-1.0)),
            ("-0", F(-0.0)), ("1e-41", F(1e-41)))
PLACEMENTS = ("row", "corner", "seam_x", "seam_y", "block", "interior", "edge", "miss", "isolated")
SIZES = [(33, 31), (100, 76)]  # (w, h): no multiple of the 16-pixel tile; interior LDS tiles at 100 x 76


def _grow(mask: np.ndarray, r: int) -> np.ndarray:
    """mask dilated by r pixels (Chebyshev)."""
    h, w = mask.shape
    p = np.pad(mask, r)
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def _all_hits(hit: np.ndarray, r: int) -> np.ndarray:
    """Pixels whose (2 r + 1)^2 neighbourhood lies inside the image and is all hits."""
    return ~_grow(np.pad(~hit, r, constant_values=True), r)[r:-r, r:-r]


def synthetic_guides(h: int, w: int, miss_column: int | None = None) -> dict:
    """Guide planes of a flat wall facing the camera (every pixel a hit of triangle 0, position
    (0.1 x, 0.1 y, 0), t = 4, normal +z, albedo 0.5 + 0.25 (x % 2)) with one column of misses."""
    y, x = np.mgrid[0:h, 0:w]
    pos = np.zeros((h, w, 4), F)
    pos[..., 0], pos[..., 1], pos[..., 3] = F(0.1) * x.astype(F), F(0.1) * y.astype(F), F(4)
    nrm = np.zeros((h, w, 4), F)
    nrm[..., 2] = F(1)
    nrm[..., 3] = np.zeros((h, w), np.int32).view(F)
    alb = np.empty((h, w, 4), F)
    alb[..., 0:3] = (F(0.5) + F(0.25) * (x % 2).astype(F))[..., None]
    alb[..., 3] = F(1)
    if miss_column is not None:
        pos[:, miss_column] = (0, 0, 0, MISS_T)
        nrm[:, miss_column, 0:3] = 0
        nrm[:, miss_column, 3] = np.full(h, -1, np.int32).view(F)
        alb[:, miss_column] = 0
    return {"pos_t": pos, "nrm_tri": nrm, "albedo": alb}


def craft(img, g) -> tuple:
    """img (h, w, 4), finite, with the special values written into pixels chosen from the guide planes
    g -> (plane, record); record: "pixels", a list of (placement, y, x, channels, value name);
    "where", placement -> list of (y, x); "special", the (h, w) bool plane of the pixels written."""
    hit = hit_mask(g)
    h, w = hit.shape
    out = np.array(img, F).reshape(h, w, 4)
    assert np.isfinite(out).all()
    assert h > 20 and w > 20, "the tile seam at pixels 15 | 16 lies inside the image"
    assert hit.any() and not hit.all(), "the camera shows hits and misses"
    taken = np.zeros((h, w), bool)
    rec = {"pixels": [], "where": {k: [] for k in PLACEMENTS}}

    def put(where, y, x, k, chans=(0, 1, 2)):
        name, v = SPECIALS[k]
        out[y, x, list(chans)] = v
        taken[y, x] = True
        rec["pixels"].append((where, int(y), int(x), tuple(chans), name))
        rec["where"][where].append((int(y), int(x)))

    def free():
        return ~_grow(taken, 2)

    # the row: the one nearest two thirds up that shows hits and misses, clear of the seam rows and the edges
    rows = [y for y in range(3, h - 3) if not 12 <= y <= 19 and hit[y].any() and not hit[y].all()]
    assert rows, "a row with hits and misses"
    ry = min(rows, key=lambda y: abs(y - (2 * h) // 3))
    for x in range(w):
        put("row", ry, x, x % 7, (x % 3,))
    for (y, x), k, ch in zip([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)], (0, 1, 2, 3),
                             ((0, 1, 2), (0,), (1,), (0, 1, 2))):
        put("corner", y, x, k, ch)

    # both sides of the tile seam, on hits where there are such
    def seam(pairs, where, ks, chans):
        ok = [p for p in pairs if all(free()[q] for q in p)]
        assert ok, where
        both = [p for p in ok if all(hit[q] for q in p)]
        for q, k, ch in zip((both or ok)[0], ks, chans):
            put(where, *q, k, ch)
    seam([((y, 15), (y, 16)) for y in range(3, h - 3)], "seam_x", (0, 4), ((2,), (0, 1, 2)))
    seam([((15, x), (16, x)) for x in range(3, w - 3)], "seam_y", (1, 6), ((0, 1, 2), (0, 1, 2)))

    # the block: NaN on 3 x 3 hits, clear of everything so far
    grown = _grow(taken, 3)
    cand = np.argwhere(_all_hits(hit, 1) & ~grown)
    assert len(cand), "a 3 x 3 block of hits"
    by, bx = cand[len(cand) // 2]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            put("block", by + dy, bx + dx, 0)

    # the isolated pixels of the three kinds of place, one per value
    beside = np.zeros((h, w), bool)  # a miss pixel left, right, below or above
    beside[:, 1:] |= ~hit[:, :-1]
    beside[:, :-1] |= ~hit[:, 1:]
    beside[1:] |= ~hit[:-1]
    beside[:-1] |= ~hit[1:]
    kinds = (("interior", _all_hits(hit, 2)), ("edge", hit & beside), ("miss", ~hit))
    for k in range(len(SPECIALS)):
        for where, mask in kinds:
            cand = np.argwhere(mask & free())
            if len(cand):
                y, x = cand[(len(cand) * (k + 1)) // (len(SPECIALS) + 1)]
                put(where, y, x, k)
                rec["where"]["isolated"].append((int(y), int(x)))
    for where in PLACEMENTS:
        assert rec["where"][where], where
    for y, x in rec["where"]["isolated"]:
        assert taken[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].sum() == 1, (y, x)
    for where in ("interior", "edge", "miss"):
        assert rec["pixels"][[p[0] for p in rec["pixels"]].index(where)][4] == "nan", where
    rec["special"] = taken
    return out, rec


def nonfinite(a) -> np.ndarray:
    """(h, w) bool: the pixel holds a value that is not finite in r, g or b."""
    return ~np.isfinite(np.asarray(a, F)[..., 0:3]).all(-1)
