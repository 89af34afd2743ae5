"""include/pt_fmath.h: the shared transcendentals are the correctly rounded float values
(float64 numpy, i.e. glibc's double functions, rounded to float), special values, and their
distance from glibc's own float functions (sinf ... powf); on the structured input sets of
tests/fmath_sets.py each result is a nearest float to the exact value by mpmath; the float
approximations ptm_atan2f_fast / ptm_asinf_fast stay within their 4 / 3 ulp, and the sky texel
decision built on them (pt_device.h sphTexel, restated in tests/sph_texel_ref.py) agrees with the
correctly rounded functions at directions aimed at texel edges."""
import ctypes as C

import numpy as np
import pytest

import fmath_sets as fs
import sph_texel_ref as sph

host = fs.host  # pt_fmath_host


N = 400_000


def _gen(seed):
    rng = np.random.default_rng(seed)
    return rng


# (fn id, name, glibc float function, input generator, float64 reference); the ranges cover every
# use in the kernels (IS:148-149,176,489-490,502-505,525,582,639,660) and beyond
CASES = [
    (0, "sin", "sinf", lambda r, n: (r.uniform(-8, 8, n),), lambda x: np.sin(x[0])),
    (1, "cos", "cosf", lambda r, n: (r.uniform(-8, 8, n),), lambda x: np.cos(x[0])),
    (2, "atan2", "atan2f", lambda r, n: (r.normal(size=n), r.normal(size=n)), lambda x: np.arctan2(x[0], x[1])),
    (3, "asin", "asinf", lambda r, n: (r.uniform(-1, 1, n),), lambda x: np.arcsin(x[0])),
    (4, "log", "logf", lambda r, n: (np.exp(r.uniform(-100, 88, n)),), lambda x: np.log(x[0])),
    (5, "exp", "expf", lambda r, n: (r.uniform(-100, 88, n),), lambda x: np.exp(x[0])),
    (6, "pow", "powf", lambda r, n: (r.uniform(1e-6, 1, n), r.uniform(0, 2, n)), lambda x: np.power(x[0], x[1])),
]


@pytest.mark.parametrize("fn,name,gname,gen,ref", CASES, ids=[c[1] for c in CASES])
def test_correctly_rounded(fn, name, gname, gen, ref):
    """Every value is the float64 result rounded to float (no exception in 4e5 inputs)."""
    x = [a.astype(np.float32) for a in gen(_gen(100 + fn), N)]
    got = host(fn, *x)
    want = ref([a.astype(np.float64) for a in x]).astype(np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (name, bad.size, [a[bad[:3]] for a in x], got[bad[:3]], want[bad[:3]])


# glibc's float functions are not correctly rounded everywhere: the share of inputs where they
# differ from pt_fmath (always by one ulp), measured on 1e5 inputs of the same ranges
GLIBC_DIFFER_AT_MOST = {"sin": 0.02, "cos": 0.02, "atan2": 0.2, "asin": 0.1, "log": 0.002, "exp": 0.002, "pow": 0.002}


@pytest.mark.parametrize("fn,name,gname,gen,ref", CASES, ids=[c[1] for c in CASES])
def test_distance_from_glibc_float_functions(fn, name, gname, gen, ref):
    m = C.CDLL("libm.so.6")
    x = [a.astype(np.float32) for a in gen(_gen(200 + fn), 100_000)]
    f = getattr(m, gname)
    f.restype = C.c_float
    f.argtypes = [C.c_float] * len(x)
    g = np.array([f(*[float(a[i]) for a in x]) for i in range(x[0].size)], np.float32)
    p = host(fn, *x)
    ulp = np.abs(p.view(np.int32).astype(np.int64) - g.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, (name, ulp.max())
    assert (ulp > 0).mean() <= GLIBC_DIFFER_AT_MOST[name], (name, (ulp > 0).mean())


def test_special_values():
    a = host(2, np.array([0, 0, 1, -1, 0, -0.0], np.float32), np.array([0, -1, 0, 0, 1, -1], np.float32))
    assert np.allclose(a, [0, np.pi, np.pi / 2, -np.pi / 2, 0, -np.pi], atol=1e-7)
    assert np.isnan(host(3, np.array([1.5], np.float32)))[0]
    assert np.array_equal(host(3, np.array([1, -1], np.float32)), np.float32([np.pi / 2, -np.pi / 2]))
    assert host(4, np.array([1.0], np.float32))[0] == 0.0
    assert host(4, np.array([0.0], np.float32))[0] == -np.inf
    assert host(4, np.array([1e-45], np.float32))[0] == np.float32(np.log(np.float64(np.float32(1e-45))))
    assert host(5, np.array([0.0], np.float32))[0] == 1.0
    assert host(5, np.array([-200.0], np.float32))[0] == 0.0
    assert host(5, np.array([89.0], np.float32))[0] == np.inf
    assert host(6, np.array([0.25], np.float32), np.array([0.5], np.float32))[0] == 0.5
    s = host(0, np.array([0.0, np.pi / 2, np.pi], np.float32))
    assert np.array_equal(s, np.sin(np.float32([0.0, np.pi / 2, np.pi]).astype(np.float64)).astype(np.float32))


def test_ranges_used_by_the_kernel():
    # toSpherical inputs: unit vectors -> |asin arg| <= 1, atan2 on the sphere
    rng = _gen(5)
    v = rng.normal(size=(N, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v.astype(np.float32)
    a = host(2, v[:, 2], v[:, 0])
    assert np.all(np.abs(a) <= np.float32(np.pi))
    b = host(3, v[:, 1])
    assert np.all(np.abs(b) <= np.float32(np.pi / 2))


# ---- the structured sets (tests/fmath_sets.py) against mpmath
# Inputs of the sets below at which a function is not correctly rounded: fn -> {argument bits}.
#
# POW_TOP_OF_BINADE: ptm_powf(x, 0.5) and ptm_powf(x, -1) at x = 2^e (2 - 2^-23), the last float of
# a binade. sqrt(4 (1 - 2^-24)) = 2 - 2^-24 - 2^-50 ... and 1 / (2 - 2^-23) = 1/2 + 2^-25 + 2^-49 ...
# lie 2^-49 relative from the midpoint of two floats, and ptm_powf's w = y log x carries log's 1e-16
# relative error as an absolute one, |w| 1e-16, into exp: beyond |w| ~ 10 (x far from 1) that
# exceeds 2^-49 and the result is the float on the other side of the midpoint, one ulp off. (In the
# kernels SampleGTR1's exponent is a random number in (0, 1] and the tonemap's is the caller's
# 1 / gamma, of colours near 1.) Listed by x's biased exponent; the mantissa is 0x7fffff.
POW_TOP_OF_BINADE = {
    0.5: [4, 6, 12, 14, 20, 22, 28, 34, 38, 42, 46, 50, 54, 58, 62, 76, 80, 82, 84, 156, 158, 160, 162, 164, 166, 176,
          180, 184, 198, 202, 206, 210, 214, 218, 220, 226, 234, 240, 242, 248, 250],
    -1.0: [5, 6, 13, 14, 21, 22, 28, 29, 219, 220, 226, 227, 234, 235, 242, 243, 249, 250],
}
KNOWN_NOT_NEAREST = {
    6: {(e << 23 | 0x7fffff, int(np.float32(y).view(np.uint32))) for y, es in POW_TOP_OF_BINADE.items() for e in es},
}


def _args_bits(args, i):
    return tuple(int(a.view(np.uint32)[i]) for a in args)


@pytest.mark.parametrize("fn", [0, 1, 2, 3, 4, 5, 6, 9, 10], ids=lambda f: fs.NAMES[f])
def test_structured_sets_are_correctly_rounded(fn):
    """fn 0-6 and the two results of ptm_sincosf: on every finite input of the structured set the
    result is a nearest float to the exact value (mpmath at fs.MP_BITS bits wherever float64 cannot
    decide, and on a fixed subset) -- except exactly the named known cases above, each one ulp off."""
    args = fs.inputs(fn)
    got = host(fn, *args)
    bad, n_mp = fs.not_nearest(fn, got, args)
    print(f"{fs.NAMES[fn]}: {got.size} inputs, {n_mp} decided by mpmath, {bad.size} not nearest")
    found = {_args_bits(args, i) for i in bad}
    known = set(KNOWN_NOT_NEAREST.get(fn, []))
    if bad.size:  # a known case is the neighbouring float, never farther
        assert fs.ulp_error(fn, got[bad], [a[bad] for a in args]).max() < 1.0
    assert found == known, (fs.NAMES[fn], [(tuple(float(a[i]) for a in args), float(got[i])) for i in bad[:5]],
                            sorted(found ^ known)[:5])


@pytest.mark.parametrize("fn", range(11), ids=lambda f: fs.NAMES[f])
def test_special_arguments(fn):
    """Zero, infinite and NaN arguments give what the header defines (NaN compared as NaN, a zero
    with its sign)."""
    args, want = fs.specials(fn)
    got = host(fn, *args)
    if fn in (7, 8):  # the approximations: the same NaNs and signs, the values within their bound
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
        assert fs.ulp_error(fn, got[ok], [a[ok] for a in args]).max() <= FAST_ULP[fn]
    else:
        assert fs.same_bits_or_nan(got, want).all(), (args, got, want)


def test_sincos_equals_sin_and_cos():
    """ptm_sincosf's two results are ptm_sinf's and ptm_cosf's bits."""
    for fn in (0, 1):
        (x,) = fs.inputs(fn)
        assert np.array_equal(host(9, x).view(np.uint32), host(0, x).view(np.uint32))
        assert np.array_equal(host(10, x).view(np.uint32), host(1, x).view(np.uint32))


# pt_fmath.h: the float approximations are at most 4 (atan2) / 3 (asin) ulp from the exact value
FAST_ULP = {7: 4.0, 8: 3.0}


@pytest.mark.parametrize("fn", [7, 8], ids=lambda f: fs.NAMES[f])
def test_fast_approximations_within_their_bound(fn):
    """ptm_atan2f_fast <= 4 ulp and ptm_asinf_fast <= 3 ulp from the exact value, on the structured
    set and on 4e6 inputs spread over the range pt_device.h sphTexel uses. Measured: 3.11 ulp (atan2)
    and 2.32 ulp (asin)."""
    args = tuple(np.concatenate(p) for p in zip(fs.inputs(fn), fs.dense_fast_inputs(fn)))
    got = host(fn, *args)
    assert np.isfinite(got).all()
    err = fs.ulp_error(fn, got, args)
    k = int(np.argmax(err))
    print(f"{fs.NAMES[fn]}: max {err.max():.3f} ulp over {got.size} inputs, at {[float(a[k]) for a in args]}")
    assert err.max() <= FAST_ULP[fn], (err.max(), [float(a[k]) for a in args])
    # the largest errors again at mpmath's precision
    worst = np.argsort(err)[-200:]
    for i in worst:
        e = fs.mp_ref(fn, *[a[i] for a in args])
        r = float(e)
        u = 2.0 ** (max(np.floor(np.log2(abs(r))), -126) - 23) if r != 0 else 2.0 ** -149
        assert abs(fs.mpmath.mpf(float(got[i])) - e) / u <= FAST_ULP[fn]
    # the same signs as the correctly rounded functions
    exact = host(fn - 5, *args)
    assert np.array_equal(np.signbit(got)[exact != 0], np.signbit(exact)[exact != 0])


def test_atan2_fast_of_two_infinities_is_nan():
    """The one named case outside ptm_atan2f_fast's bound: both arguments infinite divide to a NaN
    where atan2 is +-pi/4 or +-3pi/4. pt_device.h sphTexel never decides a texel from a NaN (its
    comparisons fail and the correctly rounded functions decide), and a normalised direction has
    no infinite component."""
    inf = np.float32(np.inf)
    assert np.isnan(host(7, np.float32([inf, -inf, inf, -inf]), np.float32([inf, inf, -inf, -inf]))).all()


# ---- the sky texel decision built on the approximations (pt_device.h sphTexel), restated on the host
@pytest.mark.parametrize("W,H", sph.SIZES, ids=lambda v: str(v))
def test_sph_texel_restated_on_the_host(W, H):
    """The conditions of the texel decision that need no GPU (sph_texel_ref.check_restated_decision),
    with the approximations and the correctly rounded functions from pt_fmath_host."""
    sph.check_restated_decision(W, H, host, sph.kernel_margin())
