"""The leaf step at its edges, against the oracle bit for bit and ray for ray: hand-made scenes of
1, 2, 3, 5 and 9 triangles in leaves of 1-4 (an odd leaf leaves the second half of its last pair
record unused: pt_trace.h pairTestT reads the whole record whatever the walk uses of it), and the
cases a pair test decides -- only the first or only the second triangle of a pair in view, two
coincident triangles (an exact-t tie: the retrace in the reference order), a triangle edge-on to
the rays (|dot(N, d)| < 1e-5) and one nearer than t = 0.0005 -- through the Lambert regen kernel
(culled and PT_FLAG_NO_CULL), the Disney and MIS regen kernels, the megakernels and
pt_trace_closest, at max_bounce 0-2 and at 33x31 and 70x45 pixels (neither a multiple of the 8x8
wave tile).

What a scene must show is checked on the oracle alone (test_scenes_meet_their_conditions, no
GPU): every scene's image differs from the image of a view with nothing in it, the tie scene's
camera rays meet exact ties, the edge-on and near triangles are rejected where an ordinary one is
hit, and the leaves have the sizes the scenes are there for. A GPU case cannot then pass by
hitting nothing.

Reference: IS pass1.fsh:251-301 (hitTriangle), :335-382 (hitBVH), :846-871 (the frame).
"""
import functools

import numpy as np
import pytest

import bvh_check
import oracle
from opengl_ray_tracing_amd import FLAG_MEGAKERNEL, FLAG_NO_CULL, FLAG_REGEN, Renderer, orbit_camera, scenes

SIZES = [(33, 31), (70, 45)]
BOUNCES = [0, 1, 2]
FRAMES = 2
LEAF = 4
CAMERA = (0.0, 0.0, 3.0)  # the eye at (0, 0, 3) exactly, looking down -z: image plane x, y in [-1, 1] at distance 1.5
COLOURS = [(0.8, 0.6, 0.4), (0.3, 0.7, 0.9), (0.9, 0.3, 0.3), (0.4, 0.8, 0.3), (0.7, 0.7, 0.2), (0.6, 0.4, 0.8),
           (0.9, 0.9, 0.9), (0.2, 0.5, 0.5), (0.8, 0.5, 0.7)]


def tri(p1, p2, p3, colour):
    """One Triangle_encoded (36 f32): flat shading normals, default material with this base colour."""
    p = np.array([p1, p2, p3], np.float32)
    n = np.cross(p[1] - p[0], p[2] - p[0]).astype(np.float64)
    n = (n / np.linalg.norm(n)).astype(np.float32)
    t = np.zeros(36, np.float32)
    t[0:9] = p.ravel()
    t[9:18] = np.tile(n, 3)
    t[21:24] = colour
    t[34] = 1.0  # IOR
    return t


def tree(tris):
    """BVHNode_encoded (dummy node 0, root 1) over tris in their order: leaves of LEAF triangles from
    the front, the rest to the right -- 5 triangles: leaves of 4 and 1; 9: 4, 4 and 1."""
    lo, hi = bvh_check.tri_boxes(tris)
    nodes = [np.array([255, 128, 0, 30, 0, 0, 1, 1, 0, 0, 1, 0], np.float32)]

    def build(a, b):
        k = len(nodes)
        nodes.append(np.zeros(12, np.float32))
        if b - a <= LEAF:
            nodes[k][3:5] = [b - a, a]
        else:
            nodes[k][0] = build(a, a + LEAF)
            nodes[k][1] = build(a + LEAF, b)
        nodes[k][6:9] = lo[a:b].min(axis=0)
        nodes[k][9:12] = hi[a:b].max(axis=0)
        return k

    build(0, len(tris))
    return np.stack(nodes)


def grid(n):
    """n triangles on a 3 x 3 grid facing the camera: neighbours overlap on screen at different
    depths (the closest-hit update decides), every other one wound the other way round."""
    out = []
    for k in range(n):
        cx, cy, z = 0.9 * (k % 3 - 1), 0.9 * (k // 3 - 1) if n > 3 else 0.0, 0.11 * ((5 * k) % 9) - 0.4
        a, b, c = (cx - 0.6, cy - 0.5, z), (cx + 0.6, cy - 0.5, z + 0.2), (cx, cy + 0.6, z - 0.1)
        out.append(tri(a, b, c, COLOURS[k]) if k % 2 == 0 else tri(a, c, b, COLOURS[k]))
    return np.stack(out)


FRONT = ((-1.2, -1.0, 0.0), (1.2, -1.0, 0.1), (0.0, 1.1, -0.1))    # in view
BEHIND = ((-0.1, -0.1, 50.0), (0.1, -0.1, 50.0), (0.0, 0.1, 50.0))  # behind the eye: no camera ray meets it
# in the plane y = 0, which holds the eye: a camera ray meets it at t = 0 (rejected as nearer than 0.0005;
# dot(N, d) = -d.y, below 1e-5 for rays along the plane: rejected as edge-on)
EDGE_ON = ((-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (0.0, 0.0, 1.0))
# 0.0003 in front of the eye and across the whole view: every camera ray meets its plane at
# t = 0.0003 / cos <= 0.00041 (cos >= 0.73 at the image's corner)
NEAR = ((-0.01, -0.01, 2.9997), (0.01, -0.01, 2.9997), (0.0, 0.02, 2.9997))


@functools.lru_cache(maxsize=None)
def all_scenes():
    """{name: (tris, nodes)}"""
    s = {f"n{n}": grid(n) for n in (1, 2, 3, 5, 9)}
    s["first_only"] = np.stack([tri(*FRONT, COLOURS[0]), tri(*BEHIND, COLOURS[1])])
    s["second_only"] = np.stack([tri(*BEHIND, COLOURS[1]), tri(*FRONT, COLOURS[0])])
    s["tie"] = np.stack([tri(*FRONT, COLOURS[0]), tri(*FRONT, COLOURS[1]), tri(*grid(1)[0, :9].reshape(3, 3), COLOURS[2])])
    s["edge_on"] = np.stack([tri(*EDGE_ON, COLOURS[3]), tri(*FRONT, COLOURS[0]), tri(*EDGE_ON[::-1], COLOURS[4])])
    s["near"] = np.stack([tri(*NEAR, COLOURS[5]), tri(*FRONT, COLOURS[0])])
    return {k: (t, tree(t)) for k, t in s.items()}


def nothing_in_view():
    t = np.stack([tri(*BEHIND, COLOURS[1])])
    return t, tree(t)


@functools.lru_cache(maxsize=None)
def env():
    return scenes.synthetic_env()


@functools.lru_cache(maxsize=None)
def oracle_frames(name, integrator, w, h, mb):
    """The oracle's running mean after FRAMES frames and the rays they traced (computed once per case)."""
    tris, nodes = nothing_in_view() if name == "nothing" else all_scenes()[name]
    eye, rot = orbit_camera(*CAMERA)
    o = oracle.Oracle(tris, nodes, env())
    acc = np.zeros((h, w, 4), np.float32)
    rays = 0
    for f in range(FRAMES):
        acc, c = o.render(w, h, integrator, f, eye, rot, accum=acc, max_bounce=mb)
        rays += c.rays
    acc.setflags(write=False)
    return acc, rays


def query_rays(name):
    """Rays from the eye through a 40 x 40 grid of the image plane, and each scene's own: along the
    edge-on triangle's plane at |dot(N, d)| = 0, 1e-6 (rejected) and 1e-4 (hit), and from just in front
    of FRONT (t below 0.0005: rejected) and a little further (hit)."""
    eye, _ = orbit_camera(*CAMERA)
    g = np.linspace(-0.95, 0.95, 40)
    x, y = np.meshgrid(g, g)
    d = np.stack([x.ravel(), y.ravel(), np.full(x.size, -1.5)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = [np.concatenate([np.repeat(np.asarray(eye, np.float64)[None], len(d), 0), d], 1)]
    for dy in (0.0, 1e-6, 1e-4):  # o + 3 d = (0, 0, 0.2): inside EDGE_ON
        dv = np.array([1.0, -dy, 0.0]) / np.linalg.norm([1.0, dy, 0.0])
        rays.append(np.array([[-3.0, 3.0 * dy, 0.2, *dv]]))
    p = np.array(FRONT, np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    z0 = n.dot(p[0]) / n[2]  # FRONT's plane crosses the z axis at (0, 0, z0), inside the triangle
    for dz in (0.0003, 0.002):  # straight at FRONT from dz in front of it
        rays.append(np.array([[0.0, 0.0, z0 + dz, 0.0, 0.0, -1.0]]))
    return np.concatenate(rays).astype(np.float32)


# ---------------------------------------------------------------- what the scenes must show (CPU)
def test_scenes_meet_their_conditions():
    sc = all_scenes()
    sizes = set()
    for name, (tris, nodes) in sc.items():
        bvh_check.check_tree(tris, nodes, None, LEAF)
        sizes |= {int(c) for c in nodes[1:, 3] if c > 0}
    assert sizes == {1, 2, 3, 4}
    assert [len(sc[f"n{n}"][0]) for n in (1, 2, 3, 5, 9)] == [1, 2, 3, 5, 9]
    for integrator in ("lambert", "disney", "mis"):
        for (w, h) in SIZES:
            for mb in BOUNCES:
                empty, _ = oracle_frames("nothing", integrator, w, h, mb)
                assert np.isfinite(empty).all()
                for name in sc:
                    img, rays = oracle_frames(name, integrator, w, h, mb)
                    assert np.isfinite(img).all()
                    assert not np.array_equal(img, empty), (name, integrator, w, h, mb)
                    assert rays >= FRAMES * w * h
    # the tie scene: camera rays meet the two coincident triangles at exactly the same t
    rays = query_rays("tie")
    t3 = sc["tie"][0]
    ta, ia, _ = oracle.Oracle(t3[0:1], tree(t3[0:1])).trace_closest(rays)
    tb, ib, _ = oracle.Oracle(t3[1:2], tree(t3[1:2])).trace_closest(rays)
    ties = (ia == 0) & (ib == 0) & (ta == tb)
    assert ties.sum() >= 100
    _, won, _ = oracle.Oracle(*sc["tie"]).trace_closest(rays)
    assert set(won[ties]) <= {0, 1, 2} and (won[ties] < 2).any()
    # first_only / second_only: the triangle in view is the pair's first, then its second
    for name, idx in (("first_only", 0), ("second_only", 1)):
        _, won, _ = oracle.Oracle(*sc[name]).trace_closest(rays)
        assert set(won) == {-1, idx}
    # edge_on: from the eye its plane is met at t = 0 -- never the winner; along the plane the ray that
    # crosses it inside at |dot(N, d)| = 1e-4 hits it, the rays at 0 and 1e-6 do not
    t, won, _ = oracle.Oracle(*sc["edge_on"]).trace_closest(rays)
    assert set(won[:1600]) == {-1, 1}
    assert won[1600] == -1 and won[1601] == -1 and won[1602] in (0, 2)
    # near: no camera ray sees the triangle 0.0003 ahead of it; FRONT is rejected from 0.0003 and hit from 0.002
    t, won, _ = oracle.Oracle(*sc["near"]).trace_closest(rays)
    assert set(won[:1600]) == {-1, 1}
    assert won[1603] == -1 and won[1604] == 1 and abs(t[1604] - 0.002) < 1e-5


# ---------------------------------------------------------------- the kernels (GPU)
PATHS = {  # name: (integrator, flags, the frame kernel: regen 1 / megakernel 0)
    "lambert_regen": ("lambert", 0, 1),
    "lambert_regen_nocull": ("lambert", FLAG_REGEN | FLAG_NO_CULL, 1),  # the narrow variants: the binary walk
    "disney_regen": ("disney", FLAG_REGEN, 1),
    "mis_regen": ("mis", FLAG_REGEN, 1),
    "lambert_megakernel": ("lambert", FLAG_MEGAKERNEL, 0),
    "disney_megakernel": ("disney", FLAG_MEGAKERNEL, 0),
    "mis_megakernel": ("mis", FLAG_MEGAKERNEL, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_frame_kernels_equal_oracle(path, size):
    integrator, flags, regen = PATHS[path]
    w, h = size
    eye, rot = orbit_camera(*CAMERA)
    bad = []
    for mb in BOUNCES:
        with Renderer(w, h, integrator, max_bounce=mb, flags=flags) as r:
            r.upload_env(env())
            for name, (tris, nodes) in all_scenes().items():
                r.upload_scene(tris, nodes)
                r0 = r.stats().rays
                r.render_frames(eye, rot, 0, FRAMES)
                r.synchronize()
                img, st = r.accum(), r.stats()
                assert st.regen == regen, (path, name, st.regen)
                ref, ref_rays = oracle_frames(name, integrator, w, h, mb)
                same = np.array_equal(img, ref)
                print(f"{path} {w}x{h} mb {mb} {name}: equal {same}, rays {st.rays - r0} oracle {ref_rays}")
                if not same or st.rays - r0 != ref_rays:
                    bad.append((name, mb, bool(same), int(st.rays - r0), ref_rays))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, FLAG_NO_CULL, 0x40])  # 0x40 = FLAG_REFERENCE_TREE
def test_trace_closest_equals_oracle(flags):
    with Renderer(8, 8, "lambert", flags=flags) as r:
        for name, (tris, nodes) in all_scenes().items():
            rays = query_rays(name)
            r.upload_scene(tris, nodes)
            t, won = r.trace_closest(rays)
            t_o, won_o, _ = oracle.Oracle(tris, nodes).trace_closest(rays)
            assert (won_o >= 0).sum() > 50, name
            assert np.array_equal(won, won_o), name
            assert np.array_equal(t, t_o), name
