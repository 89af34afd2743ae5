"""The reference fold of the many-sample radiance query (tests/radiance_mean_ref.py) against the oracle's own
chained frames and the moments' specification, and the library's argument checks, all without a GPU."""
import ctypes as C
import functools

import numpy as np

import oracle
import radiance_mean_ref as mr
import radiance_ref as rf
import variance_ref as vr
from opengl_ray_tracing_amd import _native
from post_common import INVALID, bits, config

F = np.float32
W, H, NS = 33, 31, 5


@functools.lru_cache(maxsize=None)
def c2_samples():
    """-> (the oracle's samples 0 .. 4 of c2 at 33 x 31 (NS, H, W, 4), its five chained frames' accumulation)"""
    cfg, tris, nodes, hdr, eye, rot = config("c2")
    orc = oracle.Oracle(tris, nodes, hdr)
    samples = np.stack([rf.oracle_sample(orc, W, H, cfg.integrator, cfg.max_bounce, eye, rot, s) for s in range(NS)])
    acc = np.zeros((H, W, 4), F)
    for f in range(NS):
        acc, _ = orc.render(W, H, cfg.integrator, f, eye, rot, accum=acc, max_bounce=cfg.max_bounce)
    samples.setflags(write=False)
    acc.setflags(write=False)
    return samples, acc


def test_fold_equals_the_oracles_chained_frames():
    samples, acc = c2_samples()
    mean, _ = mr.fold(samples.reshape(NS, -1, 4), 0)
    assert np.array_equal(bits(mean), bits(acc.reshape(-1, 4)[:, 0:3]))
    assert len(np.unique(bits(mean), axis=0)) > 100  # a picture, not a constant


def test_moments_equal_the_specification():
    samples, _ = c2_samples()
    _, m = mr.fold(samples.reshape(NS, -1, 4), 0)
    want = vr.moments(list(samples))
    assert np.array_equal(bits(m), bits(want.reshape(-1, 2)))
    assert (m[:, 1] > 0).any()


def test_split_fold_equals_the_whole():
    s = c2_samples()[0].reshape(NS, -1, 4)
    mean, m = mr.fold(s, 0)
    a, ma = mr.fold(s[:3], 0)
    b, mb = mr.fold(s[3:], 3, a, ma)
    assert np.array_equal(bits(b), bits(mean)) and np.array_equal(bits(mb), bits(m))


def test_argument_checks_without_a_gpu():
    """PT_E_INVALID from both forms for a NULL context, nSamples 0, a sample range that would wrap the
    weight's s + 1u, and an unknown flag bit: none of these needs a context, so none needs a GPU."""
    lib = _native.load()
    fp, ip = _native.c_float_p, _native.c_int_p
    rays = np.zeros((4, 6), F)
    ids = np.zeros((4, 2), np.int32)
    mean = np.full((4, 4), -5.0, F)
    mom = np.full((4, 2), -5.0, F)

    def both(first, ns, flags):
        return [lib.pt_radiance_mean(None, rays.ctypes.data_as(fp), ids.ctypes.data_as(ip), 4, first, ns, flags,
                                     mean.ctypes.data_as(fp), mom.ctypes.data_as(fp)),
                lib.pt_radiance_mean_device(None, C.c_void_p(rays.ctypes.data), C.c_void_p(ids.ctypes.data), 4, first, ns,
                                            flags, C.c_void_p(mean.ctypes.data), C.c_void_p(mom.ctypes.data))]

    assert both(0, 1, 0) == [INVALID] * 2  # a NULL context
    assert both(0, 0, 0) == [INVALID] * 2
    assert both(0, -3, 0) == [INVALID] * 2
    assert both(2**32 - 1, 1, 0) == [INVALID] * 2  # s + 1u would be 0
    assert both(2**32 - 5, 5, 0) == [INVALID] * 2
    assert both(0, 1, 0x2) == [INVALID] * 2
    assert both(0, 1, 0x80000001) == [INVALID] * 2
    assert np.all(mean == F(-5.0)) and np.all(mom == F(-5.0))
