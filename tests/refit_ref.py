"""The specification of pt_update_geometry (include/pt_abi.h) in numpy, and the inputs its tests share
(tests/test_refit_ref.py on the oracle alone, tests/test_gpu_dynamic.py on the GPU): helpers only.

refit_nodes restates the boxes an update gives the uploaded tree: the topology stays, every reachable
node's box becomes the exact bounds of its triangles (a leaf: triangles in index order, each
min(p1, min(p2, p3))) or of its children (an internal node: the left child before the right), with the
reference's select forms min(a, b) = b < a ? b : a and max(a, b) = a < b ? b : a (scene.cpp gmin / gmax,
glm's). That is what every builder of the reference and of scene.cpp stores for the same topology
(test_refit_ref.py: bit for bit), so the contract of an update is equality with a fresh upload of
(updated_tris, refit_nodes), and with the oracle on those arrays.

A child id <= 0 or >= nNodes is absent (pt_scene_prep.cpp encodeWideTree); an internal node without
children keeps its box; unreachable nodes keep theirs.
"""
import functools

import numpy as np

F = np.float32


def gmin(a, b):
    return np.where(b < a, b, a)


def gmax(a, b):
    return np.where(a < b, b, a)


def refit_nodes(nodes, tris):
    """-> (nodes' (n, 12) f32, reachable (n,) bool). tris: (m, 36) or (m, 18) f32, floats 0..8 the positions."""
    nd = np.array(nodes, F).reshape(-1, 12)
    t = np.ascontiguousarray(tris, F)
    t = t.reshape(t.shape[0], -1)
    p1, p2, p3 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    tlo = gmin(p1, gmin(p2, p3))
    thi = gmax(p1, gmax(p2, p3))
    n = nd.shape[0]
    reach = np.zeros(n, bool)
    done = np.zeros(n, bool)

    def kids(k):
        return [c for c in (int(nd[k, 0]), int(nd[k, 1])) if 0 < c < n]

    stack = [1]
    while stack:
        k = stack[-1]
        reach[k] = True
        cnt = int(nd[k, 3])
        if cnt > 0:
            first = int(nd[k, 4])
            lo, hi = tlo[first], thi[first]
            for i in range(first + 1, first + cnt):
                lo, hi = gmin(lo, tlo[i]), gmax(hi, thi[i])
            nd[k, 6:9], nd[k, 9:12] = lo, hi
            done[k] = True
            stack.pop()
            continue
        ch = kids(k)
        todo = [c for c in ch if not done[c]]
        if todo:
            stack.extend(reversed(todo))
            continue
        if ch:
            lo, hi = nd[ch[0], 6:9].copy(), nd[ch[0], 9:12].copy()
            for c in ch[1:]:
                lo, hi = gmin(lo, nd[c, 6:9]), gmax(hi, nd[c, 9:12])
            nd[k, 6:9], nd[k, 9:12] = lo, hi
        done[k] = True
        stack.pop()
    return nd, reach


def updated_tris(tris, verts):
    """The uploaded records with floats 0..17 replaced by verts ((n, 18), or (n, 36) whose floats 18.. are ignored)."""
    out = np.array(tris, F).reshape(-1, 36)
    v = np.ascontiguousarray(verts, F).reshape(out.shape[0], -1)
    out[:, :18] = v[:, :18]
    return out


def heights(nodes):
    """Nodes per height of the reachable tree (a leaf 0, an internal node one above its higher child)."""
    nd = np.asarray(nodes, F).reshape(-1, 12)
    n = nd.shape[0]
    h = np.full(n, -1)
    stack = [1]
    while stack:
        k = stack[-1]
        ch = [] if nd[k, 3] > 0 else [c for c in (int(nd[k, 0]), int(nd[k, 1])) if 0 < c < n]
        todo = [c for c in ch if h[c] < 0]
        if todo:
            stack.extend(todo)
            continue
        h[k] = 1 + max([h[c] for c in ch], default=-1)
        stack.pop()
    return np.bincount(h[h >= 0])


# ---------------------------------------------------------------------------------------------- the poses
# Pose 0 is the scene as built. Every pose is a function of the uploaded records alone, in float32, and
# moves a vertex by a function of its position, so vertices that triangles share stay shared.
def _apply(tris, fp, fn):
    t = np.asarray(tris, F).reshape(-1, 36)
    v = np.empty((t.shape[0], 18), F)
    for k in range(3):
        p = t[:, 3 * k:3 * k + 3]
        v[:, 3 * k:3 * k + 3] = fp(p)
        v[:, 9 + 3 * k:12 + 3 * k] = fn(t[:, 9 + 3 * k:12 + 3 * k], p)
    return v


def _unit(n):
    return (n / np.maximum(np.sqrt((n * n).sum(-1, keepdims=True)), F(1e-20))).astype(F)


def _bent(n, p):
    """shading normals tilted by a function of the position: a stale hit record shows in the shading"""
    return _unit(n + F(0.35) * np.sin(F(5.0) * p[:, [1, 2, 0]] + F(0.5)).astype(F))


def _extent(tris):
    p = np.asarray(tris, F).reshape(-1, 36)[:, :9].reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    return ((lo + hi) * F(0.5)).astype(F), F((hi - lo).max())


def pose(tris, k):
    """Vertex records (n, 18) f32 of pose k of the uploaded records `tris`:
    0 as built; 1 a non-rigid displacement; 2 a rotation about y plus a translation, normals rotated too;
    3 a shrink to a quarter about the centroid of the vertices; 4 everything far behind the camera (no camera ray hits)."""
    c, ext = _extent(tris)
    if k == 0:
        return _apply(tris, lambda p: p, lambda n, p: n)
    if k == 1:
        amp, freq = F(0.12) * ext, F(7.0) / ext
        return _apply(tris, lambda p: (p + amp * np.sin(freq * p[:, [1, 2, 0]] + F(0.3)).astype(F)).astype(F), _bent)
    if k == 2:
        a = F(0.6)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F)
        shift = (np.array([0.10, 0.06, -0.08], F) * ext).astype(F)
        return _apply(tris, lambda p: ((p - c) @ R.T + c + shift).astype(F), lambda n, p: (n @ R.T).astype(F))
    if k == 3:
        g = np.asarray(tris, F).reshape(-1, 36)[:, :9].reshape(-1, 3).astype(np.float64).mean(0).astype(F)  # the centroid
        return _apply(tris, lambda p: (g + F(0.25) * (p - g)).astype(F), _bent)
    if k == 4:
        return _apply(tris, lambda p: (p + np.array([0, 0, 1000], F) * ext).astype(F), lambda n, p: n)
    raise ValueError(k)


POSES = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def posed(scene, k):
    """(tris', nodes', reachable) of pose k of a test scene ("material", "c2", "chain"): the arrays a fresh
    upload and the oracle take. Shared: do not write to them."""
    tris, nodes = scene_arrays(scene)[:2]
    t = updated_tris(tris, pose(tris, k))
    nd, reach = refit_nodes(nodes, t)
    return t, nd, reach


@functools.lru_cache(maxsize=None)
def scene_arrays(scene):
    """-> (tris, nodes, hdr, cache, eye, rot, width, height) of a test scene. Shared: do not write to them."""
    import material_scene as ms
    import oracle
    from opengl_ray_tracing_amd import scenes
    if scene == "material":
        tris, nodes, hdr, cache, eye, rot = ms.build()[:6]
        return tris, nodes, hdr, cache, eye, rot, 96, 64
    if scene == "c2":
        cfg, tris, nodes, hdr = scenes.build_config("c2")
        hdr = np.ascontiguousarray(hdr, F)
        eye, rot = ms.camera(cfg.camera)
        return (np.ascontiguousarray(tris, F), np.ascontiguousarray(nodes, F), hdr,
                np.ascontiguousarray(oracle.hdr_cache(hdr), F), eye, rot, 64, 64)
    if scene == "chain":
        tris, nodes = chain_scene(300)
        hdr, cache = ms._env()
        eye, rot = ms.camera((20.0, 15.0, 1.6))  # inside the spiral: the view clips it, a shrunken pose lies whole in front
        return tris, nodes, hdr, cache, eye, rot, 64, 64
    raise ValueError(scene)


def chain_scene(depth):
    """A tree that is one chain of `depth` internal nodes, each holding a one-triangle leaf (left) and the
    rest (right), the last one two leaves: depth + 1 small triangles strewn along a wide spiral (sparse, so the
    camera sees sky between them at every pose), the nodes hand-built in
    the reference encoding (dummy 0, root 1; internal node j is node 1 + 2 j, its leaf 2 + 2 j), the boxes
    by refit_nodes. Deeper than every on-chip traversal stack."""
    m = depth + 1
    i = np.arange(m, dtype=np.float64)
    ang = i * 0.21
    r = 0.25 + 4.0 * i / m
    ctr = np.stack([r * np.cos(ang), 4.0 * (i / m - 0.5), r * np.sin(ang)], 1)
    tris = np.zeros((m, 36), F)
    size = 0.25
    tris[:, 0:3] = ctr + np.array([-size, -size, 0.0])
    tris[:, 3:6] = ctr + np.array([size, -size, 0.02])
    tris[:, 6:9] = ctr + np.array([0.0, size, -0.02])
    e1, e2 = tris[:, 3:6] - tris[:, 0:3], tris[:, 6:9] - tris[:, 0:3]
    nrm = _unit(np.cross(e1, e2).astype(F))
    for k in range(3):
        tris[:, 9 + 3 * k:12 + 3 * k] = nrm
    tris[:, 21:24] = np.array([0.8, 0.75, 0.7], F)   # baseColor (Triangle_encoded floats 21..23)
    tris[:, 28] = 0.5                                  # roughness
    nodes = np.zeros((2 + 2 * depth, 12), F)
    for j in range(depth):
        k, leaf = 1 + 2 * j, 2 + 2 * j
        nodes[k, 0], nodes[k, 1] = leaf, k + 2
        nodes[leaf, 3], nodes[leaf, 4] = 1, j
    last = 1 + 2 * depth
    nodes[last, 3], nodes[last, 4] = 1, depth
    return tris, refit_nodes(nodes, tris)[0]


def camera_hits(scene, k):
    """The oracle's closest hit of every pixel's frame-0 camera ray at pose k -> (t, tri), (h * w,) each."""
    import material_scene as ms
    import oracle
    t, nd, _ = posed(scene, k)
    _, _, _, _, eye, rot, w, h = scene_arrays(scene)
    tt, tri, _ = oracle.Oracle(t, nd).trace_closest(ms.frame_rays(w, h, eye, rot))
    return tt, tri


@functools.lru_cache(maxsize=None)
def oracle_frames(scene, k, integrator, max_bounce, frames):
    """The oracle's running mean after each of `frames` frames at pose k -> (tuple of (h, w, 4), Counters of the last)."""
    import oracle
    t, nd, _ = posed(scene, k)
    _, _, hdr, cache, eye, rot, w, h = scene_arrays(scene)
    o = oracle.Oracle(t, nd, hdr, cache)
    acc = np.zeros((h, w, 4), F)
    outs, cnt = [], None
    for f in range(frames):
        acc, cnt = o.render(w, h, integrator, f, eye, rot, accum=acc, max_bounce=max_bounce)
        outs.append(acc.copy())
    return tuple(outs), cnt
