"""tests/refit_ref.py, the specification of pt_update_geometry, on the CPU alone.

refit_nodes must leave the boxes of every tree the builders make as they are: each builder of the
reference and of scene.cpp stores the exact bounds of a node's triangles, folded in index order with the
select forms refit_nodes uses, so a refit of the unmoved triangles reproduces them bit for bit. If this
fails for a builder, the restatement is wrong, not the builder.

The poses of tests/test_gpu_dynamic.py (refit_ref.pose) must do something. On the oracle alone, for the
three scenes that test renders (the many-material scene at 96x64, c2 at 64x64, the 300-deep chain at
64x64): at each pose the camera's hits cover between 10 % and 95 % of the image, and the pose-0 and
pose-k images differ in at least 10 % of the pixels. If a scene misses a condition, change the pose's
amplitude or, for the hand-made chain, its geometry and camera -- not the bound. (Pose 3 is the issue's
shrink to a quarter about the centroid, which divides an unclipped silhouette by 16: the chain is sparse
and wider than the view, so the shrunken pose still covers a quarter of the image; the many-material
sphere at its given camera covers 0.107 there.)
"""
import numpy as np
import pytest

import material_scene as ms
import refit_ref as rr
from opengl_ray_tracing_amd import scenes
from opengl_ray_tracing_amd.scene import Material, Scene

F = np.float32
BUILDERS = ["sah", "median", "fixed_sah", "binned"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _material_scene():
    rs = np.random.RandomState(ms.SEED)
    v, idx = scenes.uv_sphere(30, 31, lambda u, t: 1.0 + 0.12 * np.sin(5 * u) * np.sin(4 * t))
    idx = idx[rs.uniform(size=len(idx)) >= ms.HOLES]
    s = Scene()
    s.add_mesh(v, idx, Material(), None, True)
    return s


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("scene", ["c2", "c3", "c4", "material_scene"])
def test_refit_reproduces_the_builders_boxes(scene, builder):
    s = _material_scene() if scene == "material_scene" else scenes.SCENE_BUILDERS[scene]()
    for leaf in ((4, 3, 1) if scene == "material_scene" else (8,)):
        s.build_bvh(builder, leaf)
        tris, nodes = s.encode()
        out, reach = rr.refit_nodes(nodes, tris)
        assert reach[1] and not reach[0] and reach.sum() > 1
        assert np.array_equal(bits(out[reach]), bits(np.asarray(nodes, F).reshape(-1, 12)[reach])), (scene, builder)
        assert np.array_equal(bits(out[~reach]), bits(np.asarray(nodes, F).reshape(-1, 12)[~reach]))


def _tri(a, b, c):
    t = np.zeros(36, F)
    t[0:3], t[3:6], t[6:9] = a, b, c
    return t


def test_hand_made_rows():
    t0 = _tri((0, 0, 0), (1, 0, -0.5), (0, 2, 0.25))
    t1 = _tri((-3, 1, 1), (-2, 1, 1), (-2.5, 4, 1))
    t2 = _tri((5, -1, 0), (6, -1, 0), (5, -7, 9))
    # a root that is a leaf (of two triangles)
    nodes = np.zeros((2, 12), F)
    nodes[1, 3], nodes[1, 4] = 2, 0
    out, reach = rr.refit_nodes(nodes, np.stack([t0, t1]))
    assert list(reach) == [False, True]
    assert list(out[1, 6:]) == [-3, 0, -0.5, 1, 4, 1]
    # a leaf of one triangle under a root whose right child is absent (0), and one whose child id is past the end
    for absent in (0, 7, -2):
        nodes = np.zeros((4, 12), F)
        nodes[1, 0], nodes[1, 1] = 2, absent
        nodes[2, 3], nodes[2, 4] = 1, 2
        nodes[3, 6:] = 42  # unreachable: stays
        out, reach = rr.refit_nodes(nodes, np.stack([t0, t1, t2]))
        assert list(reach) == [False, True, True, False]
        assert list(out[2, 6:]) == [5, -7, 0, 6, -1, 9] and list(out[1, 6:]) == list(out[2, 6:])
        assert list(out[3, 6:]) == [42] * 6 and list(out[0]) == [0] * 12
    # the absent child on the left
    nodes = np.zeros((3, 12), F)
    nodes[1, 0], nodes[1, 1] = 0, 2
    nodes[2, 3], nodes[2, 4] = 1, 1
    out, _ = rr.refit_nodes(nodes, np.stack([t0, t1]))
    assert list(out[1, 6:]) == [-3, 1, 1, -2, 4, 1]
    # an internal node without children keeps its box
    nodes = np.zeros((2, 12), F)
    nodes[1, 6:] = [1, 2, 3, 4, 5, 6]
    assert list(rr.refit_nodes(nodes, np.stack([t0]))[0][1, 6:]) == [1, 2, 3, 4, 5, 6]
    # the select forms: the first of +0 / -0 in fold order stays
    z = _tri((0.0, 0, 0), (-0.0, 1, 0), (1, 0, 0))
    nodes = np.zeros((2, 12), F)
    nodes[1, 3] = 1
    out, _ = rr.refit_nodes(nodes, z[None])
    assert not np.signbit(out[1, 6]) and bits(out[1, 6:9]).tolist() == [0, 0, 0]


def test_chain_300_deep():
    tris, nodes = rr.chain_scene(300)
    assert tris.shape[0] == 301 and nodes.shape[0] == 602
    per_height = rr.heights(nodes)
    assert len(per_height) == 301 and per_height[0] == 301 and (per_height[1:] == 1).all()
    p = tris[:, :9].reshape(-1, 3, 3)
    for j in (0, 1, 150, 299):
        k = 1 + 2 * j
        assert np.array_equal(nodes[k, 6:9], p[j:].reshape(-1, 3).min(0)), j
        assert np.array_equal(nodes[k, 9:12], p[j:].reshape(-1, 3).max(0)), j
        assert np.array_equal(nodes[k + 1, 6:9], p[j].min(0)) and nodes[k + 1, 3] == 1 and nodes[k + 1, 4] == j
    moved = rr.updated_tris(tris, rr.pose(tris, 1))
    out, reach = rr.refit_nodes(nodes, moved)
    assert reach[1:].all()
    q = moved[:, :9].reshape(-1, 3)
    assert np.array_equal(out[1, 6:9], q.min(0)) and np.array_equal(out[1, 9:12], q.max(0))


def test_updated_tris_keeps_the_materials():
    tris = ms.build()[0]
    v18 = rr.pose(tris, 2)
    a = rr.updated_tris(tris, v18)
    wide = np.full((tris.shape[0], 36), 7.0, F)
    wide[:, :18] = v18
    b = rr.updated_tris(tris, wide)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a[:, 18:]), bits(tris[:, 18:])) and np.array_equal(bits(a[:, :18]), bits(v18))
    assert np.array_equal(bits(rr.pose(tris, 0)), bits(tris[:, :18]))


@pytest.mark.parametrize("scene", ["material", "c2", "chain"])
def test_the_poses_do_something(scene):
    w, h = rr.scene_arrays(scene)[6:8]
    base = rr.oracle_frames(scene, 0, "lambert", 2, 1)[0][0]
    for k in (0,) + rr.POSES:
        _, tri = rr.camera_hits(scene, k)
        cover = float((tri >= 0).mean())
        print(f"{scene} pose {k}: camera hits cover {cover:.3f}")
        assert 0.10 <= cover <= 0.95, (scene, k, cover)
        if k:
            img = rr.oracle_frames(scene, k, "lambert", 2, 1)[0][0]
            diff = float((bits(img) != bits(base)).any(-1).mean())
            print(f"{scene} pose {k}: {diff:.3f} of the pixels differ from pose 0")
            assert diff >= 0.10, (scene, k, diff)
    # pose 4 takes everything out of view
    assert (rr.camera_hits(scene, 4)[1] < 0).all()
    # shared vertices stay shared: equal positions before, equal positions after
    tris = rr.scene_arrays(scene)[0]
    p0 = np.asarray(tris, F)[:, :9].reshape(-1, 3)
    _, inv = np.unique(bits(p0), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for k in rr.POSES:
        pk = rr.pose(tris, k)[:, :9].reshape(-1, 3)
        first = np.zeros((inv.max() + 1, 3), np.uint32)
        first[inv] = bits(pk)
        assert np.array_equal(first[inv], bits(pk)), (scene, k)
