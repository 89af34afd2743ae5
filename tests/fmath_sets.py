"""Structured input sets for include/pt_fmath.h and the check that a float32 result is a nearest
float to the exact value (test infrastructure, shared by tests/test_fmath.py and
tests/test_gpu_env.py).

The sets are built by structure, not drawn uniformly: every float binade of a function's documented
range with a fixed number of random mantissas and both ends of the binade, per sign; +-0; the
smallest and the largest denormal; and per function the inputs where its evaluation is most
delicate (the floats nearest k pi/2 for the trigonometric reduction, the denormal results and the
cut-offs of exp, 1 +- k ulp for log and pow, 1 - k ulp and 0.5 +- k ulp for asin, the breakpoint
ratios and the diagonal for atan2). Inputs with an infinite or NaN argument come separately, with
the result the header defines for them (specials()).

Function ids are pt_fmath_host's: 0 sin, 1 cos, 2 atan2(x, y), 3 asin, 4 log, 5 exp, 6 pow(x, y),
7 ptm_atan2f_fast, 8 ptm_asinf_fast, 9 / 10 the sine / cosine of ptm_sincosf.
"""
from __future__ import annotations

import functools

import mpmath
import numpy as np

MP_BITS = 160  # >= 120: the working precision of the mpmath reference
F32_MAX = np.float32(3.4028234663852886e38)
DEN_MIN = np.float32(1.401298464324817e-45)
DEN_MAX = np.uint32(0x007fffff).view(np.float32)
NAMES = {0: "sin", 1: "cos", 2: "atan2", 3: "asin", 4: "log", 5: "exp", 6: "pow", 7: "atan2_fast", 8: "asin_fast",
         9: "sincos.s", 10: "sincos.c"}


def host(fn: int, x, y=None) -> np.ndarray:
    """pt_fmath_host: function fn of float32 x (and y) on the CPU."""
    import ctypes as C

    from opengl_ray_tracing_amd import _native
    fp = C.POINTER(C.c_float)
    x = np.ascontiguousarray(x, np.float32)
    y = None if y is None else np.ascontiguousarray(y, np.float32)
    out = np.empty_like(x)
    rc = _native.load().pt_fmath_host(fn, x.ctypes.data_as(fp), None if y is None else y.ctypes.data_as(fp), x.size,
                                      out.ctypes.data_as(fp))
    assert rc == 0, rc
    return out


def bits(u) -> np.ndarray:
    return np.asarray(u, np.uint32).view(np.float32)


def step(x, k) -> np.ndarray:
    """The float k ulps from x (k an int or an int array; away from zero for k > 0), for x != 0."""
    x = np.asarray(x, np.float32)
    return (x.view(np.int32) + np.asarray(k, np.int32)).astype(np.int32).view(np.float32)


def binades(rng, e_lo: int, e_hi: int, per: int, signs=(0, 1)) -> np.ndarray:
    """Per sign and per biased exponent e_lo..e_hi (0 = the denormals): `per` random mantissas and
    both ends of the binade."""
    out = []
    for e in range(e_lo, e_hi + 1):
        m = np.concatenate([rng.integers(0, 1 << 23, per, dtype=np.uint32), np.uint32([0, 0x7fffff])])
        if e == 0:
            m[m == 0] = 1  # (0 is not a denormal: +-0 are added by the callers)
        for s in signs:
            out.append(np.uint32(s << 31) | np.uint32(e << 23) | m)
    return bits(np.concatenate(out))


def _around(centres, k=4) -> np.ndarray:
    c = np.asarray(centres, np.float32).reshape(-1, 1)
    return step(np.repeat(c, 2 * k + 1, 1), np.arange(-k, k + 1, dtype=np.int32)[None, :]).reshape(-1)


ZEROS = np.float32([0.0, -0.0])
DENORMS = np.float32([DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX])


def _trig_set(rng, per):
    # |x| < 2^19: biased exponents 0 .. 127 + 18
    x = [binades(rng, 0, 127 + 18, per), ZEROS, DENORMS]
    # the floats nearest k pi/2 (and their neighbours): the worst cancellation of the reduction
    kmax = int(2 ** 19 / (np.pi / 2)) - 1
    k = np.unique(np.concatenate([np.arange(1, 200), np.geomspace(200, kmax, 1500).astype(np.int64),
                                  rng.integers(1, kmax, 1500), [kmax]]))
    near = (k * (np.pi / 2)).astype(np.float32)
    x += [_around(near, 1), -near]
    x = np.concatenate(x)
    return (x[np.abs(x) < 2.0 ** 19],)


def _asin_set(rng, per):
    x = [binades(rng, 0, 126, per), ZEROS, DENORMS, np.float32([1.0, -1.0])]
    k = np.arange(1, 65, dtype=np.int32)
    x += [step(np.float32(1.0), -k), -step(np.float32(1.0), -k), _around([0.5, -0.5], 64)]
    return (np.concatenate(x),)


def _log_set(rng, per):
    x = [binades(rng, 0, 254, per, signs=(0,)), np.float32([DEN_MIN, DEN_MAX, 1.0, F32_MAX])]
    k = np.arange(1, 65, dtype=np.int32)
    x += [step(np.float32(1.0), k), step(np.float32(1.0), -k), bits(np.arange(1, 258, dtype=np.uint32))]
    return (np.concatenate(x),)


def _exp_set(rng, per):
    x = [binades(rng, 0, 127 + 7, per), ZEROS, DENORMS]
    x += [np.linspace(-104.5, -87.0, 20000).astype(np.float32), np.linspace(88.0, 88.9, 4000).astype(np.float32)]
    x += [_around([88.8, -104.0, 88.72284, -103.27893, -103.97208, -87.33655], 8)]
    return (np.concatenate(x),)


ATAN_BREAKS = [0.09849140335716425, 0.3033466836073424, 0.5345111359507916, 0.8206787908286602, 1.0]
ATAN_CENTRES = [0.198912367379658, 0.41421356237309503, 0.6681786379192989]
FAST_BREAKS = [0.4142135623730950, 2.414213562373095]


def _atan2_set(rng, per):
    a = binades(rng, 0, 254, per)
    ys, xs = [a, rng.permutation(a)], [rng.permutation(a), a]
    # a narrow band of exponents too, so that most ratios lie where the polynomials work
    b = binades(rng, 120, 134, 8 * per)
    ys += [b, ZEROS.repeat(2), DENORMS, np.float32([1, 1, -1, -1]), DENORMS]
    xs += [rng.permutation(b), np.tile(ZEROS, 2), np.float32([1, 1, -1, -1]), DENORMS, DENORMS[::-1].copy()]
    # the ratios |y| / |x| at the breakpoints +- ulps, both ways round, every quadrant
    for r in ATAN_BREAKS + ATAN_CENTRES + FAST_BREAKS:
        x = bits(rng.integers(0x3f800000 - (20 << 23), 0x3f800000 + (20 << 23), 24 * per, dtype=np.uint32))
        y = (x.astype(np.float64) * r).astype(np.float32)
        y = step(y, rng.integers(-3, 4, y.size).astype(np.int32))
        sy, sx = rng.choice(np.float32([1, -1]), y.size), rng.choice(np.float32([1, -1]), y.size)
        ys += [y * sy, x * sx]
        xs += [x * sx, y * sy]
    # the diagonal |y| = |x|, denormal and huge magnitudes included
    d = binades(rng, 0, 254, 2, signs=(0,))
    for sy in (1, -1):
        for sx in (1, -1):
            ys.append(d * np.float32(sy))
            xs.append(d * np.float32(sx))
    return np.concatenate(ys), np.concatenate(xs)


POW_Y = np.float32([DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX, 0.5, -0.5, 1, -1, 2, -2, 1 / 2.2, 2.2, 100, -100])


def _pow_set(rng, per):
    k = np.arange(1, 33, dtype=np.int32)
    x = np.concatenate([binades(rng, 0, 254, max(per // 4, 2), signs=(0,)), np.float32([DEN_MIN, DEN_MAX, F32_MAX]),
                        step(np.float32(1.0), k), step(np.float32(1.0), -k)])
    xs, ys = [np.repeat(x, POW_Y.size)], [np.tile(POW_Y, x.size)]
    # products y log x at the cut-offs (88.8 and -104) and at the largest and smallest finite results
    for y in POW_Y[4:]:
        for w in (88.8, -104.0, 88.72284, -103.27893, -103.97208, -87.33655):
            with np.errstate(over="ignore"):
                c = np.float32(np.exp(np.float64(w) / np.float64(y)))
            if np.isfinite(c) and c > 0:
                a = _around([c], 12)
                xs.append(a)
                ys.append(np.full(a.size, y, np.float32))
    x, y = np.concatenate(xs), np.concatenate(ys)
    keep = np.isfinite(x) & (x > 0)
    return x[keep], y[keep]


_BUILD = {0: _trig_set, 1: _trig_set, 9: _trig_set, 10: _trig_set, 2: _atan2_set, 7: _atan2_set, 3: _asin_set,
          8: _asin_set, 4: _log_set, 5: _exp_set, 6: _pow_set}
_SEED = {0: 11, 1: 12, 9: 11, 10: 12, 2: 13, 7: 13, 3: 14, 8: 14, 4: 15, 5: 16, 6: 17}


@functools.lru_cache(maxsize=None)
def _inputs(fn: int, per: int):
    args = tuple(np.ascontiguousarray(a, np.float32) for a in _BUILD[fn](np.random.default_rng(_SEED[fn]), per))
    for a in args:
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return args


def dense_fast_inputs(fn: int, n: int = 4_000_000):
    """For the two float approximations, whose error is spread over their whole range and not
    gathered at structural points: n inputs as pt_device.h sphTexel feeds them (atan2: points of
    circles of random radius around 1 at uniformly random angles, both arguments; asin: uniform in
    [-1, 1])."""
    rng = np.random.default_rng(70 + fn)
    if fn == 7:
        t, r = rng.uniform(-np.pi, np.pi, n), np.exp(rng.uniform(-3, 3, n))
        return (r * np.sin(t)).astype(np.float32), (r * np.cos(t)).astype(np.float32)
    return (rng.uniform(-1, 1, n).astype(np.float32),)


def inputs(fn: int, per: int = 48):
    """The finite structured inputs of function fn: a tuple of one or two float32 arrays (read-only)."""
    return _inputs(fn, per)


def specials(fn: int):
    """Inputs with a zero, infinite or NaN argument and the result the header defines for them:
    (args, want); want's NaNs mean "a NaN", its zeros carry their sign."""
    inf, nan, pi = np.float32(np.inf), np.float32(np.nan), np.float64(np.pi)
    f = np.float32
    if fn in (0, 1, 9, 10):  # (no infinite or NaN argument: outside the documented range)
        # (sin(-0) is +0, not libm's -0: the reduction's fused multiply-adds end in +0)
        return (f([0.0, -0.0]),), (f([0, 0]) if fn in (0, 9) else f([1, 1]))
    if fn in (2, 7):
        y = f([0, -0.0, 0, -0.0, 1, -1, 1, -1, inf, -inf, inf, -inf, 1, -1, 1, -1, nan, 1, nan, 0, -0.0])
        x = f([0, 0, -0.0, -0.0, 0, 0, -0.0, -0.0, 1, 1, -1, -1, inf, inf, -inf, -inf, 1, nan, nan, 1, 1])
        w = [0, -0.0, pi, -pi, pi / 2, -pi / 2, pi / 2, -pi / 2, pi / 2, -pi / 2, pi / 2, -pi / 2, 0, -0.0, pi, -pi,
             nan, nan, nan, 0, -0.0]
        if fn == 2:  # both infinite: ptm_atan2f only (ptm_atan2f_fast gives NaN, test_fmath.py's named case)
            y = np.concatenate([y, f([inf, -inf, inf, -inf])])
            x = np.concatenate([x, f([inf, inf, -inf, -inf])])
            w += [pi / 4, -pi / 4, 3 * pi / 4, -3 * pi / 4]
        return (y, x), np.float64(w).astype(np.float32)
    if fn in (3, 8):
        x = f([0, -0.0, 1, -1, step(f(1), 1), -step(f(1), 1), 2, -2, inf, -inf, nan])
        # (ptm_asinf(-0) is +0, not libm's -0; ptm_asinf_fast keeps the sign)
        return (x,), np.float64([0, -0.0 if fn == 8 else 0.0, pi / 2, -pi / 2] + [nan] * 7).astype(np.float32)
    if fn == 4:
        x = f([0, -0.0, 1, inf, -inf, nan, -1, -DEN_MIN])
        return (x,), f([-inf, -inf, 0, inf, nan, nan, nan, nan])
    if fn == 5:
        x = f([0, -0.0, inf, -inf, nan, F32_MAX, -F32_MAX])
        return (x,), f([1, 1, inf, 0, nan, inf, 0])
    if fn == 6:  # the header's definition: x >= 0 (a negative x is a NaN)
        x = f([2, nan, 0, inf, 1, 1, 1, 0, 0, 0, 0, -1, -0.5, nan, 2, inf, inf, inf, inf, 2, 2, 0.5, 0.5, -inf])
        y = f([0, 0, 0, 0, nan, inf, -inf, 2, -2, inf, -inf, 2, 0.5, 1, nan, 2, -2, inf, -inf, inf, -inf, inf, -inf, 1])
        w = f([1, 1, 1, 1, 1, 1, 1, 0, inf, 0, inf, nan, nan, nan, nan, inf, 0, inf, 0, inf, 0, 0, inf, nan])
        return (x, y), w
    raise ValueError(fn)


def with_specials(fn: int, per: int = 48):
    """inputs(fn) followed by specials(fn)'s arguments (for host / device bit comparisons)."""
    return tuple(np.concatenate([a, b]) for a, b in zip(inputs(fn, per), specials(fn)[0]))


# ---- references
def f64_ref(fn: int, args) -> np.ndarray:
    """The function in float64 numpy (about 1e-16 relative: enough wherever the exact value is not
    within 1e-9 of a rounding midpoint)."""
    a = [np.asarray(v, np.float64) for v in args]
    with np.errstate(all="ignore"):
        if fn in (0, 9):
            return np.sin(a[0])
        if fn in (1, 10):
            return np.cos(a[0])
        if fn in (2, 7):
            return np.arctan2(a[0], a[1])
        if fn in (3, 8):
            return np.arcsin(a[0])
        if fn == 4:
            return np.log(a[0])
        if fn == 5:
            return np.exp(a[0])
        return np.power(a[0], a[1])


def _mpf(v) -> mpmath.mpf:
    return mpmath.mpf(float(v))  # a float32 / float64 is an exact mpf


def mp_ref(fn: int, *v) -> mpmath.mpf:
    """The exact function of float arguments at MP_BITS bits."""
    with mpmath.workprec(MP_BITS):
        a = [_mpf(t) for t in v]
        if fn in (0, 9):
            return mpmath.sin(a[0])
        if fn in (1, 10):
            return mpmath.cos(a[0])
        if fn in (2, 7):
            return mpmath.atan2(a[0], a[1])
        if fn in (3, 8):
            return mpmath.asin(a[0])
        if fn == 4:
            return mpmath.log(a[0])
        if fn == 5:
            return mpmath.exp(a[0])
        return mpmath.power(a[0], a[1])


def neighbours(got: np.ndarray):
    """In float64: the midpoints between each finite float32 of `got` and the floats below and above
    it (beyond +-F32_MAX: the midpoint to 2^128, where rounding turns to infinity; for an infinite
    `got` that same midpoint and the infinity)."""
    g = np.asarray(got, np.float32)
    top = np.float64(2.0 ** 128) * (1.0 - 2.0 ** -25)
    with np.errstate(all="ignore"):
        lo = np.nextafter(g, np.float32(-np.inf)).astype(np.float64)
        hi = np.nextafter(g, np.float32(np.inf)).astype(np.float64)
        gd = g.astype(np.float64)
        mlo = np.where(np.isinf(lo), -top, 0.5 * (gd + lo))
        mhi = np.where(np.isinf(hi), top, 0.5 * (gd + hi))
        mlo = np.where(gd == np.inf, top, np.where(gd == -np.inf, -np.inf, mlo))
        mhi = np.where(gd == -np.inf, -top, np.where(gd == np.inf, np.inf, mhi))
    return mlo, mhi


def mp_is_nearest(fn: int, got, *v) -> bool:
    """Whether float32 `got` is a nearest float to the exact fn(*v), decided at MP_BITS bits against
    both of got's float neighbours (nothing is rounded through float64)."""
    if np.isnan(got):
        return False
    mlo, mhi = neighbours(np.float32([got]))
    with mpmath.workprec(MP_BITS):
        e = mp_ref(fn, *v)
        return bool(_mpf(mlo[0]) <= e <= _mpf(mhi[0]))


def not_nearest(fn: int, got: np.ndarray, args, mp_subset: int = 400, seed: int = 0):
    """The indices at which float32 got[i] is not a nearest float to the exact fn(args[i]).

    The bulk is decided by float64 numpy: got is nearest when the float64 value lies between the
    midpoints to got's two float neighbours, by more than 1e-9 relative. Every input whose float64
    value lies within 1e-9 relative of one of those midpoints -- on either side -- is decided by
    mpmath instead, and so is a fixed random subset of mp_subset inputs whatever float64 says.
    -> (bad indices, number decided by mpmath)"""
    got = np.asarray(got, np.float32)
    ref = f64_ref(fn, args)
    mlo, mhi = neighbours(got)
    with np.errstate(all="ignore"):
        tol = 1e-9
        near = (np.abs(ref - mlo) <= tol * np.abs(mlo)) | (np.abs(ref - mhi) <= tol * np.abs(mhi))
        inside = (ref >= mlo) & (ref <= mhi)
    bad = ~inside & ~near
    bad |= np.isnan(got) | np.isnan(ref)
    pick = np.zeros(got.size, bool)
    pick[np.random.default_rng(seed).choice(got.size, min(mp_subset, got.size), replace=False)] = True
    todo = np.nonzero((near | pick) & ~np.isnan(got))[0]
    for i in todo:
        bad[i] = not mp_is_nearest(fn, got[i], *[a[i] for a in args])
    return np.nonzero(bad)[0], int(todo.size)


def ulp_error(fn: int, got: np.ndarray, args) -> np.ndarray:
    """|got - exact| in units of the float32 spacing at the exact value (float64 reference: its own
    error is below 1e-8 of such a unit)."""
    ref = f64_ref(fn, args)
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126)))
        ulp = np.exp2(e - 23)
        return np.abs(np.asarray(got, np.float64) - ref) / ulp


def same_bits_or_nan(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: equal bits, or both NaN (a NaN's sign and payload differ between an x86 host and the GPU)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
