"""float32 numpy restatement of the sky texel decision (pt_device.h toSpherical + texIndex,
sphTexelExact and sphTexel) and the directions that aim at its edges (test infrastructure, shared by
tests/test_fmath.py and tests/test_gpu_env.py).

numpy's float32 +, -, *, / are the IEEE operations the kernels use; the transcendentals come in as
arrays (float64 numpy rounded to float for the reference, pt_fmath_host for the restatements).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from fmath_sets import same_bits_or_nan

f32 = np.float32
PT_PI = f32(3.1415926)  # pt_device.h PT_PI (IS:23), not pi
SIZES = [(1, 1), (3, 2), (64, 32), (333, 197), (1000, 500), (2048, 1024), (16384, 8192), (65535, 32768)]


def kernel_margin() -> float:
    """The fallback zone of pt_device.h sphTexel, in units of the map's size, read from its source."""
    src = (Path(__file__).resolve().parent.parent / "opengl_ray_tracing_amd" / "csrc" / "pt_device.h").read_text()
    body = src[src.index("int sphTexel(int W, int H, V3 v)"):]
    body = body[:body.index("return sphTexelExact")]
    mx = re.search(r"fabsf\(fx - rintf\(fx\)\) > ([0-9.e+-]+)f \* \(float\)W", body)
    my = re.search(r"fabsf\(fy - rintf\(fy\)\) > ([0-9.e+-]+)f \* \(float\)H", body)
    assert mx and my and mx.group(1) == my.group(1), "sphTexel's fallback zone is no longer written as the tests read it"
    return float(mx.group(1))


def normalize(v) -> np.ndarray:
    """pt_device.h normalize in float32: v * (1 / sqrt((x x + y y) + z z))."""
    v = np.ascontiguousarray(v, f32)
    with np.errstate(all="ignore"):
        d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        inv = f32(1.0) / np.sqrt(d)
        return (v * inv[:, None]).astype(f32)


def coords(a, b, W: int, H: int):
    """toSpherical's (u, w) from atan2 / asin values and the texel coordinates texXY floors:
    (u * W, w * H), all float32."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        a = a / (f32(2.0) * PT_PI)
        b = b / PT_PI
        a = a + f32(0.5)
        b = b + f32(0.5)
        return a * f32(W), (f32(1.0) - b) * f32(H)


def texel_of(fx, fy, W: int, H: int) -> np.ndarray:
    """texIndex: floor, clamp to the map (fmaxf / fminf: a NaN becomes 0), y * W + x."""
    with np.errstate(all="ignore"):
        x = np.fmin(np.fmax(np.floor(fx), f32(0.0)), f32(W - 1)).astype(np.int64)
        y = np.fmin(np.fmax(np.floor(fy), f32(0.0)), f32(H - 1)).astype(np.int64)
    return y * W + x


def fast_decides(fx, fy, W: int, H: int, margin: float) -> np.ndarray:
    """sphTexel's condition on the approximate coordinates (false for a NaN)."""
    m = f32(margin)
    with np.errstate(all="ignore"):
        return (np.abs(fx - np.rint(fx)) > m * f32(W)) & (np.abs(fy - np.rint(fy)) > m * f32(H))


def edge_distance(fx, fy, W: int, H: int) -> np.ndarray:
    """The smaller distance of the two coordinates from a texel edge, in units of the map's size."""
    with np.errstate(all="ignore"):
        dx = np.abs(fx.astype(np.float64) - np.rint(fx)) / W
        dy = np.abs(fy.astype(np.float64) - np.rint(fy)) / H
    return np.minimum(dx, dy)


def dir_of(u, v) -> np.ndarray:
    """In float64, the direction whose toSpherical is (u, v); rounded to float32 and normalised as
    the kernels' normalize does."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    a = (u - 0.5) * (2.0 * np.float64(PT_PI))
    b = ((1.0 - v) - 0.5) * np.float64(PT_PI)
    d = np.stack([np.cos(b) * np.cos(a), np.sin(b), np.cos(b) * np.sin(a)], 1)
    return normalize(d.astype(f32))


def _edges(rng, n: int, size: int) -> np.ndarray:
    """n coordinates in [0, 1], each a texel edge k / size +- a log-uniform offset of 1e-9 .. 1e-5;
    nine in ten at an inner edge where the map has one (the two outer edges of the elevation are the
    poles, where a float direction cannot resolve such an offset)."""
    inner = rng.integers(1, size, n) if size > 1 else rng.integers(0, 2, n) * size
    outer = rng.integers(0, 2, n) * size
    k = np.where(rng.random(n) < 0.9, inner, outer)
    off = np.exp(rng.uniform(np.log(1e-9), np.log(1e-5), n)) * rng.choice([-1.0, 1.0], n)
    return np.clip(k / size + off, 0.0, 1.0)


def aimed_directions(W: int, H: int, n: int, seed: int) -> np.ndarray:
    """n directions with u, v or both (a third each) aimed at a texel edge of a W x H map."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 3, n)
    u = np.where(which != 1, _edges(rng, n, W), rng.random(n))
    v = np.where(which != 0, _edges(rng, n, H), np.arccos(rng.uniform(-1, 1, n)) / np.pi)
    return dir_of(u, v)


def special_directions(seed: int) -> np.ndarray:
    """Directions taken as they are (not all of them unit vectors): uniformly random ones; the poles,
    y = +-1 and +-(1 - k ulp); the seam, x < 0 with z = +-0 and +- a denormal; the axes and the other
    zero-component cases with both signs of zero, the zero vector included; vectors a few ulps off
    unit length; |y| = 1 + 1 ulp, where asin is a NaN."""
    rng = np.random.default_rng(seed)
    one = f32(1.0)
    den = [f32(1.401298464324817e-45), np.uint32(0x007fffff).view(f32), f32(1e-41)]
    out = [normalize(rng.normal(size=(40000, 3)))]
    # the poles
    for k in range(0, 40):
        y = (one.view(np.int32) - np.int32(k)).view(f32)
        r = np.sqrt(max(0.0, 1.0 - float(y) ** 2))
        t = rng.uniform(-np.pi, np.pi, 16)
        for s in (1, -1):
            p = np.stack([r * np.cos(t), np.full(16, s * float(y)), r * np.sin(t)], 1).astype(f32)
            out += [p, normalize(p)]
    z = [f32(0.0), f32(-0.0)]
    out.append(f32([[a, s, b] for a in z for b in z for s in (1, -1)]))
    # the seam
    t = rng.uniform(-1.5, 1.5, 400)
    for zz in z + den + [-d for d in den]:
        out.append(np.stack([-np.cos(t), np.sin(t), np.full(t.size, zz)], 1).astype(f32))
        out.append(f32([[-1.0, 0.0, zz], [-1.0, -0.0, zz], [-0.5, 0.0, zz], [1.0, 0.0, zz]]))
    # components that are +-0, +-1 or +-sqrt(1/2), every combination
    vals = [f32(0.0), f32(-0.0), f32(1.0), f32(-1.0), f32(np.sqrt(0.5)), -f32(np.sqrt(0.5))]
    out.append(f32([[a, b, c] for a in vals for b in vals for c in vals]))
    # a few ulps off unit length
    v = normalize(rng.normal(size=(20000, 3)))
    out.append((v * (one + f32(2.0 ** -23) * rng.integers(-4, 5, (20000, 1)).astype(f32))).astype(f32))
    # |y| = 1 + 1 ulp
    up = (one.view(np.int32) + np.int32(1)).view(f32)
    t = rng.uniform(-np.pi, np.pi, 64)
    for s in (1, -1):
        out.append(np.stack([1e-4 * np.cos(t), np.full(64, s * float(up)), 1e-4 * np.sin(t)], 1).astype(f32))
        out.append(f32([[0.0, s * up, 0.0], [-0.0, s * up, -0.0], [-1e-3, s * up, 0.0]]))
    return np.ascontiguousarray(np.concatenate(out), f32)


def reference_texel(dirs, W: int, H: int):
    """The reference: toSpherical + texIndex in float32 with atan2 and asin the float64 values
    rounded to float. -> (texel, atan2 values, asin values)"""
    d = np.asarray(dirs, np.float64)
    with np.errstate(all="ignore"):
        a = np.arctan2(d[:, 2], d[:, 0]).astype(f32)
        b = np.arcsin(d[:, 1]).astype(f32)
    fx, fy = coords(a, b, W, H)
    return texel_of(fx, fy, W, H), a, b


def restate(dirs, W: int, H: int, host, margin: float) -> dict:
    """Both of sphTexel's branches restated from pt_fmath_host (host(fn, x[, y])) on directions as
    given: "exact" the texel of the correctly rounded functions (fn 2 / 3), "fast_texel" the texel of
    the approximations (fn 7 / 8), "fast" where sphTexel takes the latter, "diff" |fast - exact|
    coordinate difference in units of the map's size (NaN where a coordinate is), "edge" the
    approximate coordinates' distance from a texel edge in the same units, and "atan2" / "asin" the
    correctly rounded values."""
    d = np.ascontiguousarray(dirs, f32)
    x, y, z = (np.ascontiguousarray(d[:, k]) for k in range(3))
    a, b = host(2, z, x), host(3, y)
    ex, ey = coords(a, b, W, H)
    fx, fy = coords(host(7, z, x), host(8, y), W, H)
    with np.errstate(all="ignore"):
        diff = np.maximum(np.abs(fx.astype(np.float64) - ex) / W, np.abs(fy.astype(np.float64) - ey) / H)
    return {"exact": texel_of(ex, ey, W, H), "fast_texel": texel_of(fx, fy, W, H),
            "fast": fast_decides(fx, fy, W, H, margin), "diff": diff, "edge": edge_distance(fx, fy, W, H),
            "atan2": a, "asin": b}


AIMED_PER_SIZE = 200_000
# 1 x 1: its only elevation edges are the poles, where y rounds to +-1 and the approximate coordinate
# lands on the edge itself, so two thirds of the aimed directions can only fall back
NO_FAST_SHARE = {(1, 1)}


def check_restated_decision(W, H, host_fn, margin):
    """The conditions of the texel decision that need no GPU: on directions aimed within 1e-9 .. 1e-5
    of texel edges, and on the special ones, the approximations decide the same texel as the
    correctly rounded functions wherever sphTexel lets them, their coordinates differ by less than
    the fallback zone, and the aimed set exercises both branches. -> (the directions, restate()'s dict, the reference texels)"""
    aimed = aimed_directions(W, H, AIMED_PER_SIZE, 1000 * W + H)
    dirs = np.concatenate([aimed, special_directions(7)])
    r = restate(dirs, W, H, host_fn, margin)
    ref, a, b = reference_texel(dirs, W, H)
    # (ptm_asinf(-0) is +0 where numpy's is -0: toSpherical adds 0.5 to either)
    assert same_bits_or_nan(r["atan2"], a).all() and (same_bits_or_nan(r["asin"], b) | ((r["asin"] == 0) & (b == 0))).all()
    assert np.array_equal(r["exact"], ref)
    fast = r["fast"]
    assert np.array_equal(r["fast_texel"][fast], ref[fast])
    worst = float(np.nanmax(r["diff"]))
    n = AIMED_PER_SIZE
    share = float(fast[:n].mean())
    close = float((r["edge"][:n][fast[:n]] <= 2 * margin).mean()) if fast[:n].any() else 0.0
    print(f"sphTexel {W}x{H}: max |fast - exact| {worst:.3e} of the size (fallback zone {margin:g}); aimed: "
          f"{100 * share:.1f} % fast, {100 * (1 - share):.1f} % fallback, {100 * close:.1f} % of the fast within "
          f"{2 * margin:g} of an edge")
    assert worst < margin
    assert 1 - share >= 0.2
    if (W, H) not in NO_FAST_SHARE:
        assert share >= 0.2 and close >= 0.01
    return dirs, r, ref
