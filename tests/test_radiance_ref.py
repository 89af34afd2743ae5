"""tests/radiance_ref.py against what it restates, and the radiance query's symbols, without a GPU."""
import ctypes as C

import numpy as np

import denoise_ref
import radiance_ref as rf
from opengl_ray_tracing_amd import _build, _native, orbit_camera

F = np.float32
SYMBOLS = ("pt_camera_rays_device", "pt_radiance_device", "pt_radiance")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_centre_draws_give_the_guide_rays():
    """Both draws 0.5: the jitter terms are exactly 0 and the rays are the pixel-centre rays, bit for bit."""
    for (w, h), cam in (((33, 31), (0.0, 0.0, 4.0)), ((7, 5), (25.0, 20.0, 0.5)), ((64, 1), (200.0, -15.0, 0.4))):
        eye, rot = orbit_camera(*cam)
        got = rf.camera_rays(w, h, eye, rot, 3, draws=np.full((w * h, 2), 0.5, F))
        assert np.array_equal(bits(got), bits(denoise_ref.camera_rays(w, h, eye, rot)))


def test_jitter_moves_the_rays_within_the_pixel():
    w, h = 9, 6
    eye, rot = orbit_camera(0.0, 0.0, 4.0)
    centre = denoise_ref.camera_rays(w, h, eye, rot)
    a, b = rf.camera_rays(w, h, eye, rot, 0), rf.camera_rays(w, h, eye, rot, 7)
    assert not np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a), bits(centre))
    assert np.array_equal(a[:, 0:3], centre[:, 0:3])
    # half a pixel in NDC is 1 / w: the direction moves by less than that (|d| before normalising >= 1.5)
    assert np.abs(a[:, 3:6] - centre[:, 3:6]).max() < 1.0 / min(w, h)
    draws = rf.jitter_draws(w, h, 7)
    assert draws.shape == (w * h, 2) and (draws >= 0).all() and (draws < 1).all()
    assert np.array_equal(rf.pixel_ids(w, h)[w + 2], [2, 1])


def test_default_ids_have_distinct_seeds():
    n = 1 << 16
    ids = rf.default_ids(n)
    assert ids.dtype == np.int32 and ids.shape == (n, 2)
    assert np.array_equal(ids[4095], [4095, 0]) and np.array_equal(ids[4096], [0, 1]) and np.array_equal(ids[4097], [1, 1])
    for s in (0, 7, 0xFFFFFFFF):
        assert len(np.unique(rf.pixel_seed(ids, s))) == n
    # before the | 1 the sums themselves are distinct: px * 1973 + py * 9277 is injective for px < 9277, py < 1973
    sums = ids[:, 0].astype(np.int64) * 1973 + ids[:, 1].astype(np.int64) * 9277
    assert len(np.unique(sums)) == n


def test_the_library_exports_the_symbols():
    assert _build.LIB.exists(), "build the library first"
    lib = C.CDLL(str(_build.LIB))
    header = (_build.INCLUDE / "pt_abi.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
        assert f"int {name}(" in header, name
