"""The uniform integrators' regen kernel in its three stages (pt_regen.hip: resolve after the walk,
the hand-out, one hit-shading site for camera and bounce hits together), against the oracle bit for
bit and with equal ray counts.

  * Bounce depths 0-3 on c2's scene, Lambert and Disney. Depth 0: every path ends in the shade stage
    and the hand-out repeats. Depth 1: every bounce hit is at the last level, so only resolve's
    emission lookup runs for them. Depths 2 and 3: hits that stay pending for the shade stage and
    last-level hits in the same waves.
  * Every way to reach the kernel, per depth: streamed batches (the camera-ray pass, the live lists,
    the colour buffer); PT_FLAG_REGEN alone (Disney's narrow variant has no pass: its lanes trace
    their camera rays and reach the shade stage through resolve; Lambert's wide variant always runs
    behind the pass, pt_plan.h planFrame); PT_FLAG_REGEN | PT_FLAG_PRIMARY_PASS one frame at a time.
    Lambert with PT_FLAG_NO_CULL runs its narrow variants, with and without the pass.
  * Last-level hits on an emitter: a closed room with an emissive ceiling and the camera inside, so
    that nearly every ray hits and the last level's emission decides the image.

70 x 45 and 33 x 31 have partial 8 x 8 tiles on both edges. Oracle images are computed once per case.

Reference: O:329-364 and D:443-481 (pathTracing), IS pass1.fsh:846-871 (main).
"""
import numpy as np
import pytest

import oracle
import parity
from opengl_ray_tracing_amd import FLAG_NO_CULL, FLAG_PRIMARY_PASS, FLAG_REGEN, Renderer, orbit_camera, scenes
from opengl_ray_tracing_amd.scene import Material, Scene, get_transform_matrix

pytestmark = pytest.mark.gpu

FORCED = FLAG_REGEN | FLAG_PRIMARY_PASS
SHAPES = [(70, 45, 3), (33, 31, 4)]  # width, height, frames
DEPTHS = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def env():
    return scenes.synthetic_env(64, 32)


@pytest.fixture(scope="module")
def c2():
    cfg, tris, nodes, _ = scenes.build_config("c2")
    eye, rot = orbit_camera(*cfg.camera)
    return tris, nodes, eye, rot


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_oracle = {}


def oracle_frames(key, tris, nodes, hdr, w, h, integrator, mb, eye, rot, frames):
    """-> (the running mean after `frames` frames, rays), once per case"""
    k = (key, w, h, integrator, mb, frames)
    if k not in _oracle:
        o = oracle.Oracle(tris, nodes, hdr)
        acc = np.zeros((h, w, 4), np.float32)
        rays = 0
        for f in range(frames):
            acc, cnt = o.render(w, h, integrator, f, eye, rot, accum=acc, max_bounce=mb)
            rays += cnt.rays
        acc.setflags(write=False)
        _oracle[k] = (acc, rays)
    return _oracle[k]


def modes(integrator):
    """name -> (flags, one render_frames call); the stream runs the default kernels for Lambert (the
    regen kernel, planFrame) and is pinned for Disney, whose default is the megakernel"""
    return {"stream": (0 if integrator == "lambert" else FORCED, True),
            "regen": (FLAG_REGEN, False),
            "regen_pass": (FORCED, False)}


def gpu_frames(tris, nodes, hdr, w, h, integrator, mb, eye, rot, frames, flags, stream):
    with Renderer(w, h, integrator, max_bounce=mb, flags=flags) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        if stream:
            r.render_frames(eye, rot, 0, frames)
        else:
            for f in range(frames):
                r.render_frame(eye, rot, f)
        r.synchronize()
        st = r.stats()
        assert st.regen == 1, (flags, stream, st)
        assert st.frames == frames
        return r.accum().copy(), st.rays


def check(got, rays, want, want_rays, what):
    parity.assert_parity(got.reshape(-1, 4), want.reshape(-1, 4), what, exact=True)
    assert np.array_equal(bits(got), bits(want)), what
    assert rays == want_rays, (what, rays, want_rays)


@pytest.mark.parametrize("w,h,frames", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mb", DEPTHS)
@pytest.mark.parametrize("integrator", ["lambert", "disney"])
def test_bounce_depths(env, c2, integrator, mb, w, h, frames):
    tris, nodes, eye, rot = c2
    want, want_rays = oracle_frames("c2", tris, nodes, env, w, h, integrator, mb, eye, rot, frames)
    base, _ = oracle_frames("c2", tris, nodes, env, w, h, integrator, 0, eye, rot, frames)
    assert want_rays >= frames * w * h and (mb == 0 or want_rays > frames * w * h)
    if mb > 0:
        assert not np.array_equal(bits(want), bits(base))  # the bounces decide the image
    for name, (flags, stream) in modes(integrator).items():
        got, rays = gpu_frames(tris, nodes, env, w, h, integrator, mb, eye, rot, frames, flags, stream)
        check(got, rays, want, want_rays, f"{integrator}/{mb}/{w}x{h}/{name}")


@pytest.mark.parametrize("mb", [1, 2])
@pytest.mark.parametrize("flags", [FLAG_REGEN | FLAG_NO_CULL, FORCED | FLAG_NO_CULL], ids=["retrace", "pass"])
def test_lambert_narrow_variants(env, c2, flags, mb):
    """Without culling (the reference's own traversal) Lambert runs the narrow regen kernel: no 4-wide
    walk, and without the pass its lanes trace their own camera rays."""
    tris, nodes, eye, rot = c2
    w, h, frames = SHAPES[0]
    want, want_rays = oracle_frames("c2", tris, nodes, env, w, h, "lambert", mb, eye, rot, frames)
    for stream in (True, False):
        got, rays = gpu_frames(tris, nodes, env, w, h, "lambert", mb, eye, rot, frames, flags, stream)
        check(got, rays, want, want_rays, f"lambert narrow/{mb}/{flags:#x}/{'stream' if stream else 'call'}")


# ------------------------------------------------------------------ last-level hits on an emitter
def room(ceiling):
    """A closed room of half-size 3 around the origin (floor, four walls, a ceiling that emits
    `ceiling`) with a tilted panel inside; every mesh is a quad placed by its transform (readObj
    divides a mesh by an extent it takes from the last vertex, so the two x walls come out twice the
    size: the room is closed all the same, which the caller asserts on the oracle's ray count)."""
    s = Scene()
    R = 3.0
    quad_i = np.array([[0, 2, 1], [0, 3, 2]], np.int32)

    def quad(axis, at, material, size=2 * R, rotate=(0, 0, 0), shift=(0, 0, 0)):
        a, b = [k for k in range(3) if k != axis]
        v = np.zeros((4, 3), np.float32)  # extent 1 after readObj's division by the longest axis
        v[:, a] = [-1, 1, 1, -1]
        v[:, b] = [-1, -1, 1, 1]
        t = [0.0, 0.0, 0.0]
        t[axis] = at
        t = [t[k] + shift[k] for k in range(3)]
        s.add_mesh(v, quad_i, material, get_transform_matrix(rotate, t, (size, size, size)), False)

    quad(1, -R, Material(baseColor=(0.7, 0.7, 0.6)))
    quad(1, R, Material(baseColor=(1, 1, 1), emissive=ceiling))
    quad(0, -R, Material(baseColor=(0.8, 0.2, 0.2)))
    quad(0, R, Material(baseColor=(0.2, 0.8, 0.2)))
    quad(2, -R, Material(baseColor=(0.6, 0.6, 0.8), roughness=0.4, specular=0.5))
    quad(2, R, Material(baseColor=(0.5, 0.5, 0.5)))
    quad(1, -1.0, Material(baseColor=(0.9, 0.8, 0.3), roughness=0.3, metallic=0.5), size=2.0, rotate=(25, 10, 0),
         shift=(0.3, 0, -0.5))
    s.build_bvh("sah", 8)
    return s.encode()


@pytest.mark.parametrize("w,h,frames", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mb", [1, 2, 3])
@pytest.mark.parametrize("integrator", ["lambert", "disney"])
def test_last_level_hits_on_an_emitter(env, integrator, mb, w, h, frames):
    eye, rot = orbit_camera(30.0, 15.0, 2.0)
    tris, nodes = room((6.0, 5.0, 4.0))
    dark, nodes_dark = room((0.0, 0.0, 0.0))
    assert np.array_equal(nodes, nodes_dark)
    want, want_rays = oracle_frames("room", tris, nodes, env, w, h, integrator, mb, eye, rot, frames)
    unlit, unlit_rays = oracle_frames("dark room", dark, nodes, env, w, h, integrator, mb, eye, rot, frames)
    # the case proves something only if the emission decides the image; the room is closed, so that
    # (nearly) every ray hits: every path runs to its last level
    assert not np.array_equal(bits(want), bits(unlit))
    assert want_rays == unlit_rays and want_rays >= 0.99 * (mb + 1) * frames * w * h
    for name, (flags, stream) in modes(integrator).items():
        got, rays = gpu_frames(tris, nodes, env, w, h, integrator, mb, eye, rot, frames, flags, stream)
        check(got, rays, want, want_rays, f"room {integrator}/{mb}/{w}x{h}/{name}")
