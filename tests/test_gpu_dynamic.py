"""Geometry updated in place on the GPU (pt_update_geometry, pt_update_geometry_device,
pt_download_node_boxes; csrc/pt_refit.hip) against its specification, tests/refit_ref.py.

The contract: after update_geometry(pose k) a context is what a fresh upload of (updated_tris,
refit_nodes) would have made it, and so equals the oracle on those arrays, bit for bit: images of every
integrator through both launch forms, ray counts, query results, the boxes themselves and the fetch
counters that stale boxes would change. Scenes (refit_ref.scene_arrays): the many-material scene at 96x64
(1173 triangles, 400 materials, more than 128 internal nodes), c2 at 64x64 (a reference tree deeper than
the 32-entry LDS stack) and a hand-built chain 300 deep (the refit's one-block tail, the traversal stack's
overflow areas). tests/test_refit_ref.py shows on the oracle alone that the poses move what the camera sees.

Oracle images and posed arrays are computed once (refit_ref's caches) and shared.
"""
import numpy as np
import pytest

import material_scene as ms
import oracle
import parity
import query_ref as qr
import refit_ref as rr
from opengl_ray_tracing_amd import (FLAG_COUNT_FETCHES, FLAG_HOST_ACCEL, FLAG_MEGAKERNEL, FLAG_NO_BINS, FLAG_NO_CULL,
                                    FLAG_REFERENCE_TREE, Renderer)
from post_common import INVALID, NOSCENE, bits, rc_of

pytestmark = pytest.mark.gpu

F = np.float32
CASES = ms.INTEGRATORS  # (lambert, 2), (disney, 5), (mis, 2), (mis, 8)
FRAMES = 4


def case_id(v):
    return f"{v[0]}{v[1]}" if isinstance(v, tuple) else str(v)


def renderer(scene, integ="lambert", mb=-1, k=0, flags=0, **kw):
    """A context with pose k of the scene freshly uploaded (pose 0: the scene as built)."""
    _, _, hdr, cache, _, _, w, h = rr.scene_arrays(scene)
    tris, nodes, _ = rr.posed(scene, k)
    r = Renderer(w, h, integ, max_bounce=mb, flags=flags, **kw)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr, cache)
    return r


def verts(scene, k):
    return rr.pose(rr.scene_arrays(scene)[0], k)


def assert_image(got, want, what):
    parity.assert_parity(got.reshape(-1, 4), want.reshape(-1, 4), what, exact=True)
    assert np.array_equal(bits(got), bits(want)), what


def render(r, scene, form):
    """Frames 0 .. FRAMES-1 -> {frame: accumulation} of the frames the form materialises."""
    eye, rot = rr.scene_arrays(scene)[4:6]
    r.reset_stats()
    if form == "frames":
        r.render_frames(eye, rot, 0, FRAMES)
        return {FRAMES - 1: r.accum()}
    return {f: r.render_frame(eye, rot, f, download=True) for f in range(FRAMES)}


# ------------------------------------------------------------------ 1. a fresh upload and the oracle
def check_update(scene, integ, mb, k, form, flags=0):
    eye, rot = rr.scene_arrays(scene)[4:6]
    want = rr.oracle_frames(scene, k, integ, mb, FRAMES)[0]
    with renderer(scene, integ, mb, 0, flags) as a, renderer(scene, integ, mb, k, flags) as b:
        for f in range(2):
            a.render_frame(eye, rot, f)
        a.update_geometry(verts(scene, k))
        got_a, got_b = render(a, scene, form), render(b, scene, form)
        sa, sb = a.stats(), b.stats()
    for f in got_a:
        assert_image(got_a[f], want[f], f"{scene} {integ}/{mb} pose {k} {form} frame {f}: update vs oracle")
        assert np.array_equal(bits(got_a[f]), bits(got_b[f])), f"{scene} pose {k} {form} frame {f}: update vs fresh upload"
    assert sa.rays == sb.rays and sa.frames == sb.frames == FRAMES
    assert (sa.max_stack, sa.accel_device, sa.accel_nodes, sa.accel_depth, sa.tree4_nodes, sa.runtime_tree) == \
        (sb.max_stack, sb.accel_device, sb.accel_nodes, sb.accel_depth, sb.tree4_nodes, sb.runtime_tree)
    assert sa.upload_ms > 0


@pytest.mark.parametrize("form", ["frame", "frames"])
@pytest.mark.parametrize("k", rr.POSES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_update_equals_fresh_upload_and_oracle(case, k, form):
    check_update("material", case[0], case[1], k, form)


@pytest.mark.parametrize("form", ["frame", "frames"])
@pytest.mark.parametrize("k", rr.POSES)
def test_update_c2_deep_reference_tree(k, form):
    check_update("c2", "lambert", 2, k, form)


@pytest.mark.parametrize("scene,case", [("material", ("mis", 2)), ("c2", ("lambert", 2))], ids=["material", "c2"])
@pytest.mark.parametrize("k", rr.POSES)
def test_update_on_the_reference_tree_alone(scene, case, k):
    check_update(scene, case[0], case[1], k, "frame", FLAG_REFERENCE_TREE)


# ------------------------------------------------------------------ 2. queries
def query_rays(scene, k):
    """The camera rays, and 4 rays leaving every surface point they hit, at pose k; the oracle's answers."""
    _, _, _, _, eye, rot, w, h = rr.scene_arrays(scene)
    tris, nodes, _ = rr.posed(scene, k)
    cam = ms.frame_rays(w, h, eye, rot)
    t, tri = rr.camera_hits(scene, k)
    hit = tri >= 0
    P = (cam[hit, 0:3] + cam[hit, 3:6] * t[hit, None]).astype(F)
    p = tris[tri[hit], :9].reshape(-1, 3, 3)
    N = rr._unit(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(F))
    rays = np.concatenate([cam, qr.hemisphere_rays(P, N, 4, 100 + k)]).astype(F)
    t_o, tri_o, _ = oracle.Oracle(tris, nodes).trace_closest(rays)
    return rays, t_o, tri_o


@pytest.mark.parametrize("flags", [0, FLAG_REFERENCE_TREE, FLAG_NO_CULL], ids=["default", "reference_tree", "no_cull"])
@pytest.mark.parametrize("scene", ["material", "c2"])
def test_queries_after_an_update(scene, flags):
    import torch
    with renderer(scene, flags=flags) as r:
        for k in rr.POSES:
            rays, t_o, tri_o = query_rays(scene, k)
            assert (tri_o[len(rays) // 5:] >= 0).any() and (tri_o < 0).any()
            r.update_geometry(verts(scene, k))
            t, tri = r.trace_closest(rays)
            hit = tri_o >= 0
            assert np.array_equal(tri, tri_o) and np.array_equal(bits(t[hit]), bits(t_o[hit])), (scene, k, "host")
            d = torch.from_numpy(rays).to("cuda:0")
            torch.cuda.synchronize()
            dt, dtri = r.trace_closest_device(d)
            r.synchronize()
            dt, dtri = dt.cpu().numpy(), dtri.cpu().numpy()
            assert np.array_equal(dtri, tri_o) and np.array_equal(bits(dt[hit]), bits(t_o[hit])), (scene, k, "device")
            assert (dt[~hit] == qr.MISS_T).all()


# ------------------------------------------------------------------ 3. the boxes themselves
def assert_boxes(r, scene, k, what=""):
    _, nodes, reach = rr.posed(scene, k)
    got = r.node_boxes()
    assert got.shape == (nodes.shape[0], 6)
    assert np.array_equal(bits(got[reach]), bits(nodes[reach, 6:12])), (scene, k, what)


@pytest.mark.parametrize("scene", ["material", "c2", "chain"])
def test_node_boxes_equal_the_refit(scene):
    with renderer(scene) as r:
        assert_boxes(r, scene, 0, "as uploaded")
        for k in rr.POSES + (0,):
            r.update_geometry(verts(scene, k))
            assert_boxes(r, scene, k)


@pytest.mark.parametrize("scene", ["material", "c2", "chain"])
def test_fetch_counters_after_an_update(scene):
    """Stale boxes that still enclose the shrunken geometry (pose 3) would give the same image with more
    fetches: the reference algorithm's node and triangle fetches must be the oracle's on the refitted arrays."""
    eye, rot = rr.scene_arrays(scene)[4:6]
    for k in (3, 1):
        _, cnt = rr.oracle_frames(scene, k, "lambert", 2, 1)
        with renderer(scene, "lambert", 2, 0, FLAG_COUNT_FETCHES) as a, renderer(scene, "lambert", 2, k, FLAG_COUNT_FETCHES) as b:
            a.render_frame(eye, rot, 0)
            a.update_geometry(verts(scene, k))
            a.reset_stats()
            ia, ib = a.render_frame(eye, rot, 0, download=True), b.render_frame(eye, rot, 0, download=True)
            sa, sb = a.stats(), b.stats()
        print(f"{scene} pose {k}: update {sa.rays} rays {sa.node_fetch} nodes {sa.tri_fetch} tris; fresh {sb.node_fetch} "
              f"{sb.tri_fetch}; oracle {cnt.rays} {cnt.nodes} {cnt.tris}")
        assert np.array_equal(bits(ia), bits(ib))
        assert (sa.rays, sa.node_fetch, sa.tri_fetch) == (sb.rays, sb.node_fetch, sb.tri_fetch), (scene, k)
        assert (sa.rays, sa.node_fetch, sa.tri_fetch) == (cnt.rays, cnt.nodes, cnt.tris), (scene, k)


def test_the_chain_renders_and_overflows_the_on_chip_stack():
    eye, rot = rr.scene_arrays("chain")[4:6]
    for flags in (0, FLAG_REFERENCE_TREE):
        with renderer("chain", "mis", 2, 0, flags) as r:
            assert r.stats().max_stack > 300
            for k in (2, 1):
                r.update_geometry(verts("chain", k))
                assert r.stats().max_stack > 300
                want = rr.oracle_frames("chain", k, "mis", 2, 2)[0]
                for f in range(2):
                    assert_image(r.render_frame(eye, rot, f, download=True), want[f], f"chain pose {k} frame {f}")
                rays, t_o, tri_o = query_rays("chain", k)
                t, tri = r.trace_closest(rays)
                assert np.array_equal(tri, tri_o) and np.array_equal(bits(t[tri_o >= 0]), bits(t_o[tri_o >= 0]))


@pytest.mark.parametrize("flags", [0, FLAG_REFERENCE_TREE], ids=["runtime-tree", "uploaded-tree"])
def test_the_chain_traces_its_camera_rays_one_by_one(flags):
    """The chain is deeper than the camera-ray packets' stack (300 levels against 128), so without camera-ray
    bins the megakernel traces every camera ray on its own (primaryPacket's Tracer::trace): through the
    4-wide runtime tree, checked and retraced, and through the uploaded tree."""
    eye, rot = rr.scene_arrays("chain")[4:6]
    want = rr.oracle_frames("chain", 1, "mis", 2, 2)[0]
    with renderer("chain", "mis", 2, 1, flags | FLAG_NO_BINS | FLAG_MEGAKERNEL) as r:
        for f in range(2):
            assert_image(r.render_frame(eye, rot, f, download=True), want[f], f"chain, camera rays one by one, frame {f}")
        assert r.stats().runtime_tree == (0 if flags else 1)


# ------------------------------------------------------------------ 4. a sequence on one context
@pytest.mark.parametrize("scene,case", [("material", ("mis", 2)), ("c2", ("lambert", 2))], ids=["material", "c2"])
def test_sequence_returns_to_pose_0(scene, case):
    eye, rot = rr.scene_arrays(scene)[4:6]
    rays0, t0, tri0 = query_rays(scene, 0)
    with renderer(scene, *case) as r:
        before = render(r, scene, "frames")[FRAMES - 1]
        assert_image(before, rr.oracle_frames(scene, 0, *case, FRAMES)[0][-1], "before any update")
        qt, qtri = r.trace_closest(rays0)
        for k in (1, 2, 4, 3, 0):  # pose 4: nothing in view, no live tile; pose 3 brings the geometry back
            r.update_geometry(verts(scene, k))
            img = render(r, scene, "frames")[FRAMES - 1]
            assert_image(img, rr.oracle_frames(scene, k, *case, FRAMES)[0][-1], f"{scene} sequence pose {k}")
            assert_boxes(r, scene, k, "sequence")
        assert np.array_equal(bits(img), bits(before))
        t, tri = r.trace_closest(rays0)
        assert np.array_equal(tri, qtri) and np.array_equal(bits(t), bits(qt)) and np.array_equal(tri, tri0)


# ------------------------------------------------------------------ 5. the device form
@pytest.mark.parametrize("stride", [18, 36])
def test_device_form_in_stream_order(stride):
    import torch
    scene, case, k = "material", ("mis", 2), 1
    tris = rr.scene_arrays(scene)[0]
    v = verts(scene, k)
    want = rr.oracle_frames(scene, k, *case, FRAMES)[0][-1]
    s = torch.cuda.Stream()
    with renderer(scene, *case) as r:
        base = torch.from_numpy(v if stride == 18 else rr.updated_tris(tris, v)).to("cuda:0")
        torch.cuda.synchronize()
        r.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            # produced on the stream the update reads it on: no synchronisation in between
            d = (base * 0.5 + base * 0.5).contiguous()
            if stride == 36:
                d[:, 18:] = 7.0  # the update ignores the materials
            r.update_geometry(d)
        assert_boxes(r, scene, k, "device form")
        assert_image(render(r, scene, "frames")[FRAMES - 1], want, f"device form, stride {stride}")
        r.set_stream(None)
        for bad in (d[:, :17], d.double(), d.cpu(), d.t()):
            with pytest.raises(ValueError):
                r.update_geometry(bad)
    with pytest.raises(ValueError):
        Renderer.update_geometry(None, np.zeros((4, 17), F))


# ------------------------------------------------------------------ 6. what hangs off the scene
def test_guides_history_moments_and_bins_follow_the_update():
    scene, case, k = "material", ("mis", 2), 2
    eye, rot = rr.scene_arrays(scene)[4:6]
    with renderer(scene, *case, adaptive=True) as a, renderer(scene, *case, k=k, adaptive=True) as b:
        # a history, guides, moments, retired tiles and camera-ray bins of pose 0
        a.render_frames(eye, rot, 0, 8)
        a.render_guides(eye, rot)
        a.temporal_resolve(8, download=False)
        a.temporal_commit()
        a.adaptive_update(threshold=1e3, min_frames=2)
        assert a.moments_frames() == 8 and a.adaptive_status().retired > 0
        a.update_geometry(verts(scene, k))
        assert a.moments_frames() == 0
        st = a.adaptive_status()
        assert st.retired == 0 and st.frames == 0
        assert rc_of(a.temporal_resolve, 1) == INVALID and rc_of(a.denoise) == INVALID  # the guides are stale
        a.reset_stats()
        for r in (a, b):
            r.render_frames(eye, rot, 0, 8)  # the same camera as before the update: the bins are rebuilt
            r.render_guides(eye, rot)
        ga, gb = a.guides(), b.guides()
        for name in ("pos_t", "nrm_tri", "albedo"):
            assert np.array_equal(bits(ga[name]), bits(gb[name])), name
        acc = a.accum()
        assert_image(acc, rr.oracle_frames(scene, k, *case, 8)[0][-1], "batch launch after the update")
        assert np.array_equal(bits(acc), bits(b.accum()))
        assert a.stats().rays == b.stats().rays
        res = a.temporal_resolve(8)  # no history: the accumulation itself, as after an upload
        assert np.array_equal(bits(res[..., :3]), bits(acc[..., :3])) and np.all(res[..., 3] == 8)
        assert np.array_equal(bits(res), bits(b.temporal_resolve(8)))
        assert a.moments_frames() == 8 and np.array_equal(bits(a.moments()), bits(b.moments()))


# ------------------------------------------------------------------ 7. edges
def _one_triangle(n=1):
    tris = np.zeros((n, 36), F)
    for i in range(n):
        tris[i, 0:9] = [-1 + 0.3 * i, -1, 0.1 * i, 1, -1, 0.1 * i, 0, 1 - 0.2 * i, 0.1 * i]
        tris[i, 9:18] = [0, 0, 1] * 3
        tris[i, 21:24] = [0.7, 0.6, 0.5]
        tris[i, 28] = 0.5
    nodes = np.zeros((2, 12), F)
    nodes[1, 3], nodes[1, 4] = n, 0
    return tris, rr.refit_nodes(nodes, tris)[0]


def _quad():
    tris = np.zeros((2, 36), F)
    tris[0, 0:9] = [-1, -1, 0, 1, -1, 0, 1, 1, 0]
    tris[1, 0:9] = [-1, -1, 0, 1, 1, 0, -1, 1, 0]
    tris[:, 9:18] = [0, 0, 1] * 3
    tris[:, 21:24] = [0.7, 0.6, 0.5]
    tris[:, 28] = 0.5
    nodes = np.zeros((4, 12), F)
    nodes[1, 0], nodes[1, 1] = 2, 3
    nodes[2, 3], nodes[2, 4] = 1, 0
    nodes[3, 3], nodes[3, 4] = 1, 1
    return tris, rr.refit_nodes(nodes, tris)[0]


def check_small(tris, nodes, v, what, integ="mis"):
    """update_geometry(v) on a small hand-made scene against the oracle and a fresh upload, 40x24."""
    w, h = 40, 24
    hdr, cache = ms._env()
    eye, rot = ms.camera((15.0, 10.0, 4.0))
    t2 = rr.updated_tris(tris, v)
    n2, reach = rr.refit_nodes(nodes, t2)
    o = oracle.Oracle(t2, n2, hdr, cache)
    want = np.zeros((h, w, 4), F)
    for f in range(2):
        want, _ = o.render(w, h, integ, f, eye, rot, accum=want, max_bounce=2)
    rays = ms.frame_rays(w, h, eye, rot)
    t_o, tri_o, _ = o.trace_closest(rays)
    with Renderer(w, h, integ, max_bounce=2) as a, Renderer(w, h, integ, max_bounce=2) as b:
        a.upload_scene(tris, nodes)
        b.upload_scene(t2, n2)
        for r in (a, b):
            r.upload_env(hdr, cache)
        a.render_frame(eye, rot, 0)
        a.update_geometry(v)
        for f in range(2):
            ia, ib = a.render_frame(eye, rot, f, download=True), b.render_frame(eye, rot, f, download=True)
        assert np.array_equal(bits(ia), bits(ib)), what
        assert_image(ia, want, what)
        assert np.array_equal(bits(a.node_boxes()[reach]), bits(n2[reach, 6:12])), what
        t, tri = a.trace_closest(rays)
        assert np.array_equal(tri, tri_o) and np.array_equal(bits(t[tri_o >= 0]), bits(t_o[tri_o >= 0])), what
    return tri_o


def test_one_triangle_scene_whose_root_is_a_leaf():
    tris, nodes = _one_triangle()
    v = tris[:, :18].copy()
    v[:, 0:9] += np.tile(np.array([0.3, 0.2, -0.4], F), 3)
    assert (check_small(tris, nodes, v, "one triangle") >= 0).any()


def test_odd_count_in_one_leaf():
    tris, nodes = _one_triangle(7)
    v = tris[:, :18].copy()
    v[:, 0:9] *= F(0.8)
    assert (check_small(tris, nodes, v, "seven triangles, one leaf") >= 0).any()


def test_quad_moved_along_its_normal_has_flat_leaf_boxes():
    tris, nodes = _quad()
    v = tris[:, :18].copy()
    v[:, [2, 5, 8]] += F(0.375)
    hit = check_small(tris, nodes, v, "quad")
    assert (hit >= 0).any()
    n2 = rr.refit_nodes(nodes, rr.updated_tris(tris, v))[0]
    assert (n2[1:, 8] == n2[1:, 11]).all() and n2[1, 8] == F(0.375)


def test_odd_count_and_collapsed_triangles():
    """Triangles collapsed to a point and to a line behave exactly as after an upload (their normal is
    0 / 0; no ray hits them)."""
    scene = "material"
    tris, nodes = rr.scene_arrays(scene)[:2]
    assert tris.shape[0] % 2 == 1
    v = rr.pose(tris, 1).copy()
    _, tri = rr.camera_hits(scene, 1)
    seen = np.unique(tri[tri >= 0])
    v[seen[0], 3:6] = v[seen[0], 6:9] = v[seen[0], 0:3]          # a point
    v[seen[1], 6:9] = v[seen[1], 3:6]                            # a line
    v[seen[2], 6:9] = (v[seen[2], 0:3] + v[seen[2], 3:6]) * F(0.5)  # three points on a line
    v[tris.shape[0] - 1, 3:6] = v[tris.shape[0] - 1, 0:3]        # the last triangle: the pair record's odd end
    eye, rot = rr.scene_arrays(scene)[4:6]
    t2 = rr.updated_tris(tris, v)
    n2, reach = rr.refit_nodes(nodes, t2)
    hdr, cache = rr.scene_arrays(scene)[2:4]
    with np.errstate(all="ignore"):
        o = oracle.Oracle(t2, n2, hdr, cache)
        want = np.zeros((64, 96, 4), F)
        for f in range(2):
            want, _ = o.render(96, 64, "mis", f, eye, rot, accum=want, max_bounce=2)
    with renderer(scene, "mis", 2) as a, Renderer(96, 64, "mis", max_bounce=2) as b:
        b.upload_scene(t2, n2)
        b.upload_env(hdr, cache)
        a.update_geometry(v)
        for f in range(2):
            ia, ib = a.render_frame(eye, rot, f, download=True), b.render_frame(eye, rot, f, download=True)
        assert np.array_equal(bits(ia), bits(ib))
        assert np.array_equal(bits(ia), bits(want))
        assert np.array_equal(bits(a.node_boxes()[reach]), bits(n2[reach, 6:12]))
        rays = ms.frame_rays(96, 64, eye, rot)
        ta, tria = a.trace_closest(rays)
        tb, trib = b.trace_closest(rays)
        assert np.array_equal(tria, trib) and np.array_equal(bits(ta), bits(tb))
        assert not np.isin(tria, seen[:3]).any()


def test_tile_world_2_shares_equal_the_whole_frame():
    scene, case, k = "material", ("mis", 2), 1
    eye, rot, w, h = rr.scene_arrays(scene)[4:8]
    want = rr.oracle_frames(scene, k, *case, FRAMES)[0][-1]
    ranks = [renderer(scene, *case, tile_rank=q, tile_world=2, tile_size=16) for q in range(2)]
    try:
        owned = np.zeros((h, w), int)
        for q, r in enumerate(ranks):
            r.render_frames(eye, rot, 0, 2)
            r.update_geometry(verts(scene, k))
            r.render_frames(eye, rot, 0, FRAMES)
            img = r.accum()
            ty, tx = np.mgrid[0:h, 0:w] // 16
            mine = (ty * ((w + 15) // 16) + tx) % 2 == q
            owned += mine
            assert np.array_equal(bits(img[mine]), bits(want[mine])), q
        assert (owned == 1).all()
    finally:
        for r in ranks:
            r.close()


# ------------------------------------------------------------------ 8. errors
def last_error(r):
    return r._lib.pt_last_error(r._h).decode()


def test_error_paths():
    import ctypes as C
    import torch
    scene = "material"
    tris, nodes, hdr, cache, eye, rot, w, h = rr.scene_arrays(scene)
    v = verts(scene, 1)
    n = tris.shape[0]
    d = torch.from_numpy(v).to("cuda:0")
    torch.cuda.synchronize()
    with Renderer(w, h, "mis") as r:
        for call, arg in ((r.update_geometry, (v,)), (r.update_geometry, (d,)), (r.node_boxes, ())):
            assert rc_of(call, *arg) == NOSCENE
            assert "no scene" in last_error(r)
        r.upload_scene(tris, nodes)
        lib, hnd = r._lib, r._h
        fp = v.ctypes.data_as(C.POINTER(C.c_float))
        assert lib.pt_update_geometry(hnd, None, n, 18) == INVALID
        assert lib.pt_update_geometry(None, fp, n, 18) == INVALID
        assert lib.pt_update_geometry_device(hnd, None, n, 18) == INVALID
        assert lib.pt_download_node_boxes(hnd, None) == INVALID
        for bad_n, bad_stride in ((n - 1, 18), (n + 1, 18), (0, 18), (n, 17), (n, 0), (n, -36)):
            for form, arg in ((lib.pt_update_geometry, fp), (lib.pt_update_geometry_device, C.c_void_p(d.data_ptr()))):
                assert form(hnd, arg, bad_n, bad_stride) == INVALID, (bad_n, bad_stride)
                assert ("stride" if bad_stride != 18 else "nTriangles") in last_error(r), (bad_n, bad_stride)
        assert rc_of(r.update_geometry, v[:-1]) == INVALID
        r.update_geometry(v)  # the failed calls left the context usable
        assert_boxes(r, scene, 1, "after the failed calls")
    with Renderer(w, h, "mis", flags=FLAG_HOST_ACCEL) as r:
        r.upload_scene(tris, nodes)
        for arg in (v, d):
            assert rc_of(r.update_geometry, arg) == INVALID
            assert "PT_FLAG_HOST_ACCEL" in last_error(r)
    with Renderer(64, 64, "basic") as r:
        for call, arg in ((r.update_geometry, (v,)), (r.node_boxes, ())):
            assert rc_of(call, *arg) == NOSCENE
            assert "no scene" in last_error(r)
    with Renderer(w, h, "mis", devices=[0, 0]) as r:  # a device group: the host form serves every member
        r.upload_scene(tris, nodes)
        r.upload_env(hdr, cache)
        assert rc_of(r.update_geometry, d) == INVALID
        assert "n_devices" in last_error(r)
        r.update_geometry(v)
        for f in range(2):
            img = r.render_frame(eye, rot, f, download=True)
        assert_image(img, rr.oracle_frames(scene, 1, "mis", 2, FRAMES)[0][1], "device group after the host form")
