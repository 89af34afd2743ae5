"""What the many-sample radiance query is specified against (include/pt_abi.h pt_radiance_mean_device) --
TEST INFRASTRUCTURE: the fold of a ray's samples into its running mean and luminance moments in float32
numpy, built on the frames' own update (tests/variance_ref.py mix_sample, moments_update: the text of
csrc/pt_display.hip mixFrames). Helpers only, no tests.
"""
from __future__ import annotations

import numpy as np

import variance_ref as vr

F = np.float32


def fold(samples, first: int, mean=None, moments=None):
    """samples (ns, N, >= 3): sample first + j of N rays at [j]. mean (N, >= 3) and moments (N, 2): what the
    rays hold after samples 0 .. first - 1 (None: zeros, which first == 0 requires).
    -> (mean (N, 3), moments (N, 2)) after sample first + ns - 1."""
    samples = np.asarray(samples, F)
    ns, n = samples.shape[0], samples.shape[1]
    assert first == 0 or (mean is not None and moments is not None)
    a = np.zeros((1, n, 4), F)
    m = np.zeros((1, n, 2), F)
    if first:
        a[0, :, 0:3] = np.asarray(mean, F).reshape(n, -1)[:, 0:3]
        m[0] = np.asarray(moments, F).reshape(n, 2)
    with np.errstate(all="ignore"):
        for j in range(ns):
            c = samples[j][None, :, 0:3]
            a = vr.mix_sample(a, c, first + j)
            m = vr.moments_update(m, c, first + j)
    return np.ascontiguousarray(a[0, :, 0:3]), np.ascontiguousarray(m[0])
