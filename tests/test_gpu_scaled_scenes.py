"""Scaled and translated scenes on the GPU against the oracle, bit for bit. Every scene of the suite
lives at coordinates of order 1-10, while the hit search has absolute constants: insideByMargin's
"+ 1.0f", the cull margin 1e-3 max(1, t), hitTriangle's t >= 0.0005, the widening's 1e-30. c2's encoded
triangles and nodes are scaled by 2^e (exact, so the uploaded tree's boxes scale with them) or
translated by 2^p on every axis (the boxes recomputed, tests/refit_ref.py refit_nodes), the eye with
them, and the oracle gets the same floats (tests/accel_domain_ref.py scaled_scene, translated_scene).

What the inputs do is checked on the oracle alone in tests/test_accel_domain.py: the camera's hit share
stays 0.444 except at 2^-13 (0.233: hits fall under t >= 0.0005), and translated by 2^12 every hit fails
insideByMargin, so refReachable answers by its flat-leaf rule or the walk up the reference path.
On the scene scaled by 2^10 and more the oracle's MIS samples are NaN at most hit pixels; a NaN compares
equal to a NaN here. These rows found the MIS regen kernel ending such paths at 0 (`NdotL > 0`, `pdf > 0`
where the reference asks `<= 0`; csrc/pt_regen.hip): 276 of a 33 x 31 frame's pixels.
References are computed once (lru_cache) and shared: do not write to them."""
import functools

import numpy as np
import pytest

import accel_domain_ref as ad
import bvh_check
import denoise_ref
import oracle
import query_ref as qr
from opengl_ray_tracing_amd import FLAG_MEGAKERNEL, FLAG_REGEN, Renderer, scenes
from post_common import bits
from test_gpu_queries import same

pytestmark = pytest.mark.gpu

F = np.float32
CASES = [("scale", e) for e in (-13, -10, 10, 14, 20)] + [("shift", p) for p in (8, 12, 16)]
IDS = [f"{k}2^{v}" for k, v in CASES]
SIZES = [(33, 31), (70, 45)]


@functools.lru_cache(maxsize=None)
def scene(kind, v):
    """-> (tris, nodes, eye, rot) of c2 scaled by 2^v or translated by 2^v"""
    m = ad.model("c2")
    fn = ad.scaled_scene if kind == "scale" else ad.translated_scene
    tris, nodes, eye = fn(m["tris"], m["nodes"], m["eye"], v)
    for a in (tris, nodes, eye):
        a.setflags(write=False)
    return tris, nodes, eye, m["rot"]


@functools.lru_cache(maxsize=None)
def query_case(kind, v):
    """The 33 x 31 camera rays and 8 hemisphere rays from every hit point, with the oracle's answers"""
    tris, nodes, eye, rot = scene(kind, v)
    orc = oracle.Oracle(tris, nodes)
    g, cam, t, tri = denoise_ref.guides(orc, tris, 33, 31, eye, rot)
    hit = tri >= 0
    P = g["pos_t"].reshape(-1, 4)[hit, 0:3]
    N = g["nrm_tri"].reshape(-1, 4)[hit, 0:3]
    rays = np.concatenate([cam, qr.hemisphere_rays(P, N, 8, 11)])
    t, tri = ad.oracle_hits(orc, rays)
    assert hit.sum() >= 50 and len(rays) == 33 * 31 + 8 * hit.sum()
    return rays, t, tri


@functools.lru_cache(maxsize=None)
def oracle_frames(kind, v, integ, w, h, frames=2):
    tris, nodes, eye, rot = scene(kind, v)
    orc = oracle.Oracle(tris, nodes, scenes.synthetic_env())
    acc, rays = np.zeros((h, w, 4), F), 0
    for f in range(frames):
        acc, cnt = orc.render(w, h, integ, f, eye, rot, accum=acc, max_bounce=2)
        rays += cnt.rays
    acc.setflags(write=False)
    return acc, rays


@pytest.mark.parametrize("kind,v", CASES, ids=IDS)
def test_trace_closest(kind, v):
    tris, nodes, eye, rot = scene(kind, v)
    rays, t, tri = query_case(kind, v)
    with Renderer(64, 64, "lambert") as r:
        r.upload_scene(tris, nodes)
        got_t, got_tri = r.trace_closest(rays)
        same(got_t, got_tri, t, tri, f"{kind} 2^{v}")


def frames_equal(kind, v, integ, w, h, flags):
    tris, nodes, eye, rot = scene(kind, v)
    want, want_rays = oracle_frames(kind, v, integ, w, h)
    with Renderer(w, h, integ, max_bounce=2, flags=flags) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(scenes.synthetic_env())
        r.render_frames(eye, rot, 0, 2)
        r.synchronize()
        got, st = r.accum(), r.stats()
    what = f"{kind} 2^{v} {integ} {w}x{h} flags {flags:#x}"
    ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: {int((~ok).any(axis=2).sum())} pixels differ"
    print(what, "rays", st.rays, "oracle", want_rays, "regen", st.regen)
    if st.regen and integ == "mis":
        # the regen kernel does not trace a BRDF ray whose pdf is 0, which the reference traces and then
        # discards (IS:816; tests/test_gpu_parity.py states the same relation on the plain scenes): first seen
        # here as 3705 rays against the oracle's 3706 at 2^-10, 33 x 31. The megakernel traces them all.
        assert want_rays >= st.rays >= 0.95 * want_rays, what
    else:
        assert st.rays == want_rays, what


@pytest.mark.parametrize("integ", ["lambert", "mis"])
@pytest.mark.parametrize("kind,v", CASES, ids=IDS)
def test_frames_default_kernels(kind, v, integ):
    for w, h in SIZES:
        frames_equal(kind, v, integ, w, h, 0)


@pytest.mark.parametrize("kind,v", CASES, ids=IDS)
def test_frames_megakernel_and_regen(kind, v):
    frames_equal(kind, v, "mis", 33, 31, FLAG_MEGAKERNEL)
    frames_equal(kind, v, "lambert", 33, 31, FLAG_REGEN)


@pytest.mark.parametrize("kind,v", [("scale", 20), ("shift", 16)], ids=["scale2^20", "shift2^16"])
def test_device_builder(kind, v):
    """The GPU builder's own checks on these inputs: a tree over every triangle, leaves of <= 4, every
    box the exact union of its triangles', the same tree twice."""
    tris = scene(kind, v)[0]
    with Renderer(64, 64, "lambert") as r:
        nodes, order = r.build_bvh_device(tris, 4)
        nodes2, order2 = r.build_bvh_device(tris, 4)
    bvh_check.check_tree(tris, nodes, order, 4)
    assert np.array_equal(nodes, nodes2) and np.array_equal(order, order2)
