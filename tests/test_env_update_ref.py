"""pt_update_env on the CPU alone: tests/env_update_ref.py -- the specification of the PT_ENV_RGBE
quantiser -- against env_maps.rgbe_quantise and its documented edge values, the library's own quantiser
(include/pt_rgbe.h, the function pt_envupdate.hip's kernel calls) against the specification through
tests/native/env_quantise_check.cpp, and the four new symbols of the C ABI (loading the library needs
no GPU, as in tests/test_abi.py).
"""
import ctypes as C
import subprocess

import numpy as np

import env_maps
import env_update_ref as eu
from opengl_ray_tracing_amd import _build, _native

F = np.float32
INVALID = -1
SEEDED = [(37, 19, 101), (100, 50, 102), (64, 65, 103)]


def inputs():
    """name -> (h, w, 3) map: every map of env_maps.cache_maps() and unquantised seeded ones"""
    m = dict(env_maps.cache_maps())
    for w, h, seed in SEEDED:
        m[f"unquantised {w}x{h}"] = eu.unquantised_map(w, h, seed)
    return m


def test_reference_equals_env_maps_and_is_idempotent():
    for name, img in inputs().items():
        q = eu.quantise(img)
        assert env_maps.same_bits_or_nan(q, env_maps.rgbe_quantise(img)), name
        assert env_maps.same_bits_or_nan(eu.quantise(q), q), name
        if not name.startswith("unquantised"):
            assert env_maps.same_bits_or_nan(q, img), name  # an RGBE map is left as it is
        else:
            assert (q.view(np.uint32) != img.view(np.uint32)).mean() > 0.5, name


def test_reference_edge_texels():
    t, want = eu.edge_texels()
    got = eu.quantise(t)
    assert env_maps.same_bits_or_nan(got, want), (got, want)
    assert env_maps.same_bits_or_nan(eu.quantise(got), got)
    assert not np.signbit(got).any()  # -0 became +0
    # the largest value: E = 255, mantissa 255
    m, ex = np.frexp(eu.RGBE_MAX)
    assert ex + 128 == 255 and m * 256 == 255
    # the smallest texel kept is the first RGBE value at or above the threshold, E = 22
    assert np.ldexp(F(207), -114) < eu.RGBE_MIN <= eu.RGBE_KEPT and np.frexp(eu.RGBE_KEPT)[1] + 128 == 22
    assert got[7, 0] == eu.RGBE_KEPT == got[8, 0]


def test_every_quantised_texel_passes_the_compact_test():
    for name, img in inputs().items():
        assert eu.compact_texel_ok(eu.quantise(img)).all(), name
    t, _ = eu.edge_texels()
    assert eu.compact_texel_ok(eu.quantise(t)).all()
    # ... which is a test: the unquantised maps do not pass it
    assert eu.compact_texel_ok(eu.unquantised_map(37, 19, 101)).mean() < 0.1


def library_quantise(tmp_path, exe, texels, tag):
    src, dst = tmp_path / f"{tag}_in.bin", tmp_path / f"{tag}_out.bin"
    t = np.ascontiguousarray(texels, F).reshape(-1, 3)
    t.tofile(src)
    out = subprocess.run([str(exe), str(src), str(t.shape[0]), str(dst)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return np.fromfile(dst, F).reshape(np.shape(texels))


def test_library_quantiser_equals_the_reference(tmp_path):
    exe = _build.build_env_quantise_check()
    assert subprocess.run([str(exe)], capture_output=True, timeout=60).returncode == 0  # its own edge check
    for k, (name, img) in enumerate(inputs().items()):
        assert env_maps.same_bits_or_nan(library_quantise(tmp_path, exe, img, f"m{k}"), eu.quantise(img)), name
    t, want = eu.edge_texels()
    assert env_maps.same_bits_or_nan(library_quantise(tmp_path, exe, t, "edge"), want)
    # every binade a float has, and a few values around each power of two
    rng = np.random.default_rng(7)
    wide = np.ldexp(rng.uniform(0.5, 1.0, (4096, 3)), rng.integers(-149, 129, (4096, 3))).astype(F)
    assert env_maps.same_bits_or_nan(library_quantise(tmp_path, exe, wide, "wide"), eu.quantise(wide))


def test_abi_symbols_and_null_context():
    """Fails without the feature: the four symbols of pt_update_env."""
    lib = _native.load()
    for name in ("pt_update_env", "pt_update_env_device", "pt_download_env", "pt_env_size"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert _native.ABI_VERSION == 13 and lib.pt_abi_version() == 13  # additive: the version stays
    m = np.zeros((2, 2, 3), F)
    out = np.zeros((2, 2, 4), F)
    fp = m.ctypes.data_as(_native.c_float_p)
    w, h = C.c_int(0), C.c_int(0)
    assert lib.pt_update_env(None, fp, 2, 2, None, 0) == INVALID
    assert lib.pt_update_env_device(None, C.c_void_p(m.ctypes.data), 2, 2, None, 0) == INVALID
    assert lib.pt_download_env(None, 0, out.ctypes.data_as(_native.c_float_p), None) == INVALID
    assert lib.pt_env_size(None, C.byref(w), C.byref(h)) == INVALID
