"""What the GPU tests of the display post-processing share (test_gpu_denoise.py,
test_gpu_variance.py, test_gpu_temporal.py): helpers only, no tests and no fixtures."""
import functools
import re

import numpy as np
import pytest

from opengl_ray_tracing_amd import orbit_camera, scenes
from opengl_ray_tracing_amd._native import PtError

F = np.float32
INVALID, NOSCENE = -1, -3


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """Elementwise: equal bits, or both NaN (fmath_sets.same_bits_or_nan: a NaN's sign and payload
    differ between an x86 host and the GPU). Infinities, signed zeros and denormals compare by bits."""
    from fmath_sets import same_bits_or_nan
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, (a.shape, b.shape)
    return same_bits_or_nan(a, b)


@functools.lru_cache(maxsize=None)
def config(name):
    cfg, tris, nodes, hdr = scenes.build_config(name)
    eye, rot = orbit_camera(*cfg.camera)
    return cfg, tris, nodes, hdr, eye, rot


def device_plane(h, w, dtype="float32"):
    import torch
    t = torch.zeros((h, w, 4), dtype=getattr(torch, dtype), device="cuda:0")
    torch.cuda.synchronize()  # the fill (torch's stream) before the renderer's stream writes it
    return t


def _unorm8(x):
    """round(clamp(x, 0, 1) * 255) as the display kernels compute it: one fused multiply-add
    (exact in f64, then one rounding to f32), truncated."""
    c = np.clip(np.nan_to_num(x.astype(F), nan=0.0), 0, 1).astype(np.float64)
    return np.floor((c * 255.0 + 0.5).astype(F)).astype(np.uint8)


def rc_of(fn, *a, **kw):
    with pytest.raises(PtError) as e:
        fn(*a, **kw)
    assert str(e.value).split(": ", 1)[1], "pt_last_error text"
    return int(re.search(r"failed with (-?\d+)", str(e.value)).group(1))
