"""The ranged ray queries without a GPU: the library exports the four entry points and the binding
declares them, and tests/query_ref.py -- the specification the GPU tests compare against -- gives
what include/pt_abi.h states on hand-made rows."""
import ctypes as C

import numpy as np

import query_ref as qr
from opengl_ray_tracing_amd import Renderer, _native

F = np.float32
QUERIES = ("pt_trace_closest_range", "pt_trace_occluded", "pt_trace_closest_device", "pt_trace_occluded_device")


def test_symbols_exported_and_declared():
    lib = _native.load()
    for name in QUERIES:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is C.c_int
        assert fn.argtypes[0] is C.c_void_p
    assert len(_native.SIGNATURES["pt_trace_closest_range"][1]) == 6
    assert len(_native.SIGNATURES["pt_trace_occluded"][1]) == 5
    assert len(_native.SIGNATURES["pt_trace_closest_device"][1]) == 6
    assert len(_native.SIGNATURES["pt_trace_occluded_device"][1]) == 5
    assert _native.ABI_VERSION == 13 and lib.pt_abi_version() == 13  # additive: the version stays
    for m in ("trace_closest_range", "trace_occluded", "trace_closest_device", "trace_occluded_device"):
        assert callable(getattr(Renderer, m))


def test_null_context_is_invalid():
    lib = _native.load()
    assert lib.pt_trace_closest_range(None, None, None, 0, None, None) == -1
    assert lib.pt_trace_occluded(None, None, None, 0, None) == -1
    assert lib.pt_trace_closest_device(None, None, None, 0, None, None) == -1
    assert lib.pt_trace_occluded_device(None, None, None, 0, None) == -1


# hand-made (t*, tri*) rows: near, ordinary and far hits, the smallest t a hit can have, and a miss
T_STAR = np.array([0.0005, 0.25, 1.0, 3.75, 1.0e6, qr.MISS_T], F)
TRI_STAR = np.array([7, 0, 3, 12345, 2, -1], np.int32)
HIT = TRI_STAR >= 0


def check(kind, want_hit):
    b = qr.bound(kind, T_STAR)
    t, tri, occ = qr.query_ref(T_STAR, TRI_STAR, b)
    want_hit = np.asarray(want_hit, bool)
    assert t.dtype == F and tri.dtype == np.int32 and occ.dtype == np.uint8
    assert np.array_equal(occ, want_hit.astype(np.uint8)), kind
    assert np.array_equal(tri, np.where(want_hit, TRI_STAR, -1)), kind
    assert np.array_equal(t.view(np.uint32), np.where(want_hit, T_STAR, qr.MISS_T).astype(F).view(np.uint32)), kind


def test_no_bound_passes_every_hit():
    t, tri, occ = qr.query_ref(T_STAR, TRI_STAR, None)
    assert np.array_equal(t.view(np.uint32), T_STAR.view(np.uint32))
    assert np.array_equal(tri, TRI_STAR)
    assert np.array_equal(occ, HIT.astype(np.uint8))


def test_bound_is_strict():
    check("t", np.zeros(6, bool))  # b == t*: a miss
    check("t_up", HIT)             # one ulp above: the hit
    check("t_down", np.zeros(6, bool))
    assert np.all(qr.bound("t_up", T_STAR)[HIT] > T_STAR[HIT])
    assert np.all(qr.bound("t_down", T_STAR)[HIT] < T_STAR[HIT])


def test_bounds_at_or_below_the_triangle_test_lower_bound_miss():
    for kind in ("zero", "tmin", "minus_one"):
        check(kind, np.zeros(6, bool))
    assert qr.bound("tmin", T_STAR)[0] == F(0.0005)


def test_infinite_bound_is_no_bound_and_nan_is_a_miss():
    check("inf", HIT)
    check("nan", np.zeros(6, bool))
    assert np.isnan(qr.bound("nan", T_STAR)).all()


def test_a_miss_stays_a_miss_under_every_bound():
    for kind in qr.BOUND_KINDS:
        t, tri, occ = qr.query_ref(T_STAR, TRI_STAR, qr.bound(kind, T_STAR))
        assert t[-1] == qr.MISS_T and tri[-1] == -1 and occ[-1] == 0, kind


def test_mixed_bounds_take_each_kind_in_turn():
    t_star = np.linspace(0.5, 4.0, 32).astype(F)
    m = qr.mixed_bounds(t_star)
    for i, kind in enumerate(qr.BOUND_KINDS):
        want = qr.bound(kind, t_star)[i::len(qr.BOUND_KINDS)]
        assert np.array_equal(m[i::len(qr.BOUND_KINDS)].view(np.uint32), want.view(np.uint32)), kind


def test_hemisphere_rays_leave_along_the_normal_side():
    rs = np.random.RandomState(3)
    P = rs.uniform(-1, 1, (5, 3)).astype(F)
    N = rs.normal(size=(5, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    rays = qr.hemisphere_rays(P, N, 8, 11)
    assert rays.shape == (40, 6) and rays.dtype == F
    assert np.array_equal(rays[:, 0:3], np.repeat(P, 8, axis=0))
    assert np.all(np.einsum("rc,rc->r", rays[:, 3:6].astype(np.float64), np.repeat(N, 8, axis=0)) >= 0)
    assert np.allclose(np.linalg.norm(rays[:, 3:6], axis=1), 1.0, atol=1e-6)
    assert np.array_equal(rays, qr.hemisphere_rays(P, N, 8, 11))
