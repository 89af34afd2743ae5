"""The material paths of the frame kernels on the many-material scene (tests/material_scene.py:
400 random Disney materials on 1173 triangles, emitters and black surfaces among them) against
the oracle, bit for bit on the whole 96x64 image.

Every other scene of the GPU suite has one or two materials whose subsurface, specularTint,
anisotropic, sheen and sheenTint are 0 and, under Disney and MIS, no emitter: there a wrong term
of pt_device.h's BRDF is multiplied by 0, the camera hit's emission (pt_regen.hip camEmission,
pt_kernels.hip Le0) is 0 + Lo, and the material table (pt_scene_prep.cpp prepareScene, pt_trace.h
finishHit) has ids 0 and 1. Here every parameter, the emission terms and ids up to 399 decide the
bits of the image (tests/test_material_scene.py measures that on the oracle).

  * every frame kernel and launch form against the oracle, 3 frames, with the kernel each form
    runs (stats().regen as tests/test_gpu_parity.py test_frame_kernels_agree documents it) and
    the ray counts among the forms;
  * the reference shader text itself (tests/golden/glsl/material_frames.json), as
    tests/test_gpu_libm_pin.py does on the one-material scenes;
  * the camera hit's emission alone (max_bounce 0), a camera move within one context, the guide
    buffers' albedo and a denoise pass, and re-uploads that permute and shrink the table.

Oracle images are computed once per case in this module's cache.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as dr
import material_scene as ms
import oracle
import parity
import ref_glsl
from opengl_ray_tracing_amd import (FLAG_HOST_ACCEL, FLAG_MEGAKERNEL, FLAG_NO_BINS, FLAG_PRIMARY_PASS,
                                    FLAG_REFERENCE_TREE, FLAG_REGEN, Renderer)

pytestmark = pytest.mark.gpu

W, H = ms.W, ms.H
FRAMES = 3
CASES = ms.INTEGRATORS  # (lambert, 2), (disney, 5), (mis, 2), (mis, 8)
# launch form -> (flags, one stream of frames)
FORMS = {"sync": (0, False), "regen": (FLAG_REGEN, False), "megakernel": (FLAG_MEGAKERNEL, False),
         "regen_primary": (FLAG_REGEN | FLAG_PRIMARY_PASS, False), "no_bins": (FLAG_NO_BINS, False),
         "reference_tree": (FLAG_REFERENCE_TREE, False), "host_accel": (FLAG_HOST_ACCEL, False),
         "stream": (0, True)}
GOLD = Path(__file__).resolve().parent / "golden" / "glsl" / "material_frames.json"
TEXT_CASES = json.loads(GOLD.read_text())["cases"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def case_id(v):
    return f"{v[0]}{v[1]}" if isinstance(v, tuple) else str(v)


def expected_regen(form, integ, mb):
    """pt_plan.h planFrame: PT_FLAG_REGEN pins the regen kernel; a synchronous display() call's single
    frame runs the megakernel; streams of frames run the regen kernel for Lambert and for MIS at its
    shader's own 2 bounces."""
    if form in ("regen", "regen_primary"):
        return 1
    if form == "stream":
        return 1 if integ == "lambert" or (integ == "mis" and mb <= 2) else 0
    return 0


_oracle = {}


def oracle_images(integ, mb, frames=FRAMES, camera=ms.CAMERA, tris=None, key="scene"):
    """The oracle's running mean after each frame, once per (case, camera, material assignment `key`)."""
    k = (integ, mb, frames, camera, key)
    if k not in _oracle:
        eye, rot = ms.camera(camera)
        _oracle[k] = ms.oracle_frames(ms.build()[0] if tris is None else tris, integ, mb, frames, eye, rot)[0]
    return _oracle[k]


def renderer(integ, mb, flags=0, tris=None):
    scene, nodes, hdr, cache = ms.build()[:4]
    r = Renderer(W, H, integ, max_bounce=mb, flags=flags)
    r.upload_scene(scene if tris is None else tris, nodes)
    r.upload_env(hdr, cache)
    return r


_gpu = {}


def gpu_form(integ, mb, form):
    """-> (the accumulation after each frame it was read at, stats), once per (case, form)."""
    k = (integ, mb, form)
    if k not in _gpu:
        flags, stream = FORMS[form]
        eye, rot = ms.build()[4:6]
        with renderer(integ, mb, flags) as r:
            if stream:
                r.render_frames(eye, rot, 0, FRAMES)
                imgs = {FRAMES - 1: r.accum()}
            else:
                imgs = {f: r.render_frame(eye, rot, f, download=True) for f in range(FRAMES)}
            _gpu[k] = (imgs, r.stats())
    return _gpu[k]


def assert_image(got, want, what):
    parity.assert_parity(got.reshape(-1, 4), want.reshape(-1, 4), what, exact=True)
    assert np.array_equal(bits(got), bits(want)), what


# ------------------------------------------------------------------ every form against the oracle
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_frame_kernels_equal_oracle(case, form):
    integ, mb = case
    want = oracle_images(integ, mb)
    imgs, st = gpu_form(integ, mb, form)
    assert st.regen == expected_regen(form, integ, mb), (form, st.regen)
    assert st.frames == FRAMES
    for f, img in sorted(imgs.items()):
        assert_image(img, want[f], f"materials {integ}/{mb} {form} frame {f}")
        assert np.all(img[..., 3] == 1.0)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ray_counts_agree_among_forms(case):
    integ, mb = case
    rays = {form: gpu_form(integ, mb, form)[1] for form in FORMS}
    mk = rays["megakernel"].rays
    assert mk > FRAMES * W * H  # bounces traced
    for form, st in rays.items():
        if integ == "mis" and st.regen:
            # regeneration skips BRDF rays whose pdf is 0 (IS:816 discards them after tracing)
            assert 0.95 * mk <= st.rays <= mk, (form, st.rays, mk)
        else:
            assert st.rays == mk, (form, st.rays, mk)


# ------------------------------------------------------------------ the reference text
@pytest.mark.parametrize("case", TEXT_CASES, ids=lambda c: c["case"])
def test_gpu_material_frames_equal_reference_text(case):
    """The shaders' own main() (O, D, IS at their own bounce counts) on this scene. exact=False on
    the sampled pixels for the reason tests/test_gpu_libm_pin.py gives; the digest is the exact check."""
    tris, nodes, hdr, cache, eye, rot = ms.build()[:6]
    assert case["camera"] == list(ms.CAMERA) and (case["width"], case["height"]) == (W, H)
    idx = np.asarray(case["sample_index"])
    with Renderer(W, H, case["integrator"]) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr, cache)
        for f in range(case["frames"]):
            acc = r.render_frame(eye, rot, f, download=True)
            ref = np.asarray(case["sample_frames"][f], np.uint32).view(np.float32).reshape(-1, 4)
            got = acc.reshape(-1, 4)[idx]
            parity.assert_parity(got, ref, f"{case['case']} frame {f} vs pass1.fsh text + glibc", exact=False)
            assert ref_glsl.digest(acc) == case["digests"][f], (case["case"], f, parity.summary(got, ref))


# ------------------------------------------------------------------ emission
@pytest.mark.parametrize("flags", [FLAG_REGEN, FLAG_MEGAKERNEL], ids=["regen", "megakernel"])
@pytest.mark.parametrize("integ", ["disney", "mis"])
def test_camera_hit_emission_alone(integ, flags):
    """Every bounce cut off: a pixel whose camera ray hits an emitter carries exactly that material's
    emissive value, every other hit pixel 0 (the camera rays' hits: the oracle's closest-hit search
    of frame 0's jittered rays), and the running mean of two such frames equals the oracle's."""
    tris, nodes, _, _, eye, rot = ms.build()[:6]
    want = oracle_images(integ, 0, 2)
    _, tri, _ = oracle.Oracle(tris, nodes).trace_closest(ms.frame_rays(W, H, eye, rot, 0))
    hit = (tri >= 0).reshape(H, W)
    le = tris[np.where(tri >= 0, tri, 0), 18:21].reshape(H, W, 3)
    assert (le.any(-1) & hit).sum() >= 100
    with renderer(integ, 0, flags) as r:
        a = r.render_frame(eye, rot, 0, download=True)
        b = r.render_frame(eye, rot, 1, download=True)
        assert r.stats().regen == (1 if flags == FLAG_REGEN else 0)
    assert np.array_equal(bits(a[hit][:, :3]), bits(le[hit])), "camera-hit emission"
    assert_image(a, want[0], f"emission {integ} frame 0")
    assert_image(b, want[1], f"emission {integ} frame 1")


# ------------------------------------------------------------------ a camera move
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_camera_move_restarts_the_paths(case):
    """One context, streams of frames on the regen kernel: 3 frames here, then 3 frames from frame
    counter 0 at a second camera (the camera hit's material kept per path, pt_regen.hip mat0, must be
    the new camera's) equal the oracle at the second camera."""
    integ, mb = case
    eye, rot = ms.build()[4:6]
    eye2, rot2 = ms.camera(ms.CAMERA2)
    with renderer(integ, mb, FLAG_REGEN) as r:
        r.render_frames(eye, rot, 0, FRAMES)
        first = r.accum()
        r.render_frames(eye2, rot2, 0, FRAMES)
        second = r.accum()
        assert r.stats().regen == 1 and r.stats().frames == 2 * FRAMES
    assert_image(first, oracle_images(integ, mb)[-1], f"camera 1 {integ}/{mb}")
    assert_image(second, oracle_images(integ, mb, camera=ms.CAMERA2)[-1], f"camera 2 {integ}/{mb}")


# ------------------------------------------------------------------ guide buffers
def test_guides_and_denoise_on_many_materials():
    tris, nodes, _, _, eye, rot = ms.build()[:6]
    want, _, _, tri = dr.guides(oracle.Oracle(tris, nodes), tris, W, H, eye, rot)
    colours = np.unique(bits(want["albedo"]).reshape(-1, 4)[tri >= 0], axis=0).shape[0]
    assert colours >= 200
    with renderer("disney", 5) as r:
        for f in range(2):
            r.render_frame(eye, rot, f)
        acc = r.accum()
        r.render_guides(eye, rot)
        got = r.guides()
        den = r.denoise()
    assert np.array_equal(got["tri"].reshape(-1), tri)
    for k in ("pos_t", "nrm_tri", "albedo"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.unique(bits(got["albedo"]).reshape(-1, 4)[tri >= 0], axis=0).shape[0] == colours
    assert_image(acc, oracle_images("disney", 5)[1], "disney before the denoise pass")
    assert np.array_equal(bits(den), bits(dr.atrous(acc, want, **dr.DEFAULTS)))


# ------------------------------------------------------------------ re-uploads
@pytest.mark.parametrize("integ,mb,flags", [("mis", 2, FLAG_REGEN), ("disney", 5, FLAG_MEGAKERNEL)],
                         ids=["mis2-regen", "disney5-megakernel"])
def test_reupload_replaces_the_material_table(integ, mb, flags):
    """The same geometry with the palette assignment permuted (ids rolled by one: every triangle's
    material and the table's order change), then with one emissive material on every triangle (the
    table shrinks to one entry), then the first scene again: each image equals the oracle's for
    that assignment -- a table left over from the upload before would not -- and the guides'
    albedo follows."""
    tris, nodes, _, _, eye, rot, pal, ids = ms.build()
    rolled = ms.with_materials(tris, pal, np.roll(ids, 1))
    one = ms.with_materials(tris, pal, np.full_like(ids, ms.SLOTS["pair_emissive"] + 1))
    assert ms.table_ids(rolled).max() == ms.N_PALETTE - 1 and ms.table_ids(one).max() == 0
    assert not np.array_equal(ms.table_ids(rolled), ms.table_ids(tris))
    _, _, _, tri = dr.guides(oracle.Oracle(tris, nodes), tris, W, H, eye, rot)
    hit = (tri >= 0).reshape(H, W)
    with renderer(integ, mb, flags) as r:
        for key, scene in (("scene", None), ("rolled", rolled), ("one", one), ("scene", None)):
            src = tris if scene is None else scene
            r.upload_scene(src, nodes)
            for f in range(2):
                r.render_frame(eye, rot, f)
            want = oracle_images(integ, mb, tris=scene, key=key)[1]
            assert_image(r.accum(), want, f"upload {key} {integ}/{mb}")
            r.render_guides(eye, rot)
            alb = r.guides()["albedo"]
            assert np.array_equal(bits(alb[hit][:, :3]), bits(src[tri[tri >= 0], 21:24])), key
