"""The "looks" pt_update_materials is tested with -- TEST INFRASTRUCTURE ONLY: helpers, no tests.

A look is an (n, 18) float32 array: Triangle_encoded floats 18..35 for every triangle of a scene, in
the uploaded order. The specification of an update is a fresh upload of the scene's records with those
floats replaced (tris_of), and the table a fresh upload makes (expected: distinct keys, bit for bit, in
the order of their first appearance -- material_scene.table_ids).

Looks of the many-material scene (material_scene.build(): 1173 triangles, an odd count, 96 x 64):
  0  as built (400 materials)
  1  the palette re-dealt with a new permutation: a table of the same size in another order
  2  one distinct material per triangle: specular (a shaded scalar, equal within each of the palette's
     near-identical pairs) moved by i ulps at triangle i -- the table grows from 400 to 1173. (A specular
     of exactly 0 becomes 0.5 first, so that no denormal is shaded.)
  3  one material for all triangles: the table shrinks to 1
  4  emitters off and other entries lit
  5  look 1 with an adversarial tail in the last eight triangles: two keys that differ in one bit of
     word 17 only, a +0 / -0 pair, two triangles with the same NaN bits in IOR (not shaded: the image is
     safe) and one with another NaN payload, and the key of triangle 0 again at the last triangle

The "c2x3" scene, 64 x 64: c2's meshes with its bumpy sphere three times side by side (15004 triangles)
and a distinct material for every triangle. c2 alone has 5004 triangles, fewer than one block of the
device scan covers on this GPU generation (256 threads x 21 items = 5376), so its records are repeated
until the scan runs over more than two blocks and the probe table over more than one page.

Everything is computed once and shared: do not write to what these functions return.
"""
import functools

import numpy as np

import material_scene as ms
import oracle
from opengl_ray_tracing_amd import Material, Scene, scenes
from opengl_ray_tracing_amd.scene import get_transform_matrix

F = np.float32
LOOKS = (0, 1, 2, 3, 4, 5)
SIZES = {0: ms.N_PALETTE, 1: ms.N_PALETTE, 2: 1173, 3: 1}  # the tables' sizes (looks 4 and 5: see expected)
SPECULAR, SHEEN = ms.SCALARS["specular"], ms.SCALARS["sheen"]
NAN_A, NAN_B = 0x7fc00001, 0x7fc00002
TAIL = 8


def _ulps(col, k):
    """col (f32 in [0, 1]) moved by k[i] ulps: up below 0.75, down from there; 0 becomes 0.5 first"""
    v = np.where(col == 0, F(0.5), col).astype(F)
    b = v.view(np.uint32).astype(np.int64)
    b = np.where(v < F(0.75), b + k, b - k)
    return b.astype(np.uint32).view(F)


@functools.lru_cache(maxsize=None)
def look(k):
    """Look k of the many-material scene -> (1173, 18) f32."""
    tris, _, _, _, _, _, palette, ids = ms.build()
    n = tris.shape[0]
    if k == 0:
        out = tris[:, 18:36].copy()
    elif k == 1:
        out = palette[np.random.RandomState(9001).permutation(ms.N_PALETTE)[ids]].copy()
    elif k == 2:
        out = tris[:, 18:36].copy()
        out[:, SPECULAR] = _ulps(out[:, SPECULAR], np.arange(n))
    elif k == 3:
        out = np.tile(palette[20], (n, 1))
    elif k == 4:
        p = palette.copy()
        lit = (p[:, ms.EMISSIVE] > 0).any(1)
        p[lit, ms.EMISSIVE] = 0.0
        dark = np.flatnonzero(~lit)[::9]
        p[dark, ms.EMISSIVE] = np.array([2.5, 1.5, 0.75], F)
        out = p[ids].copy()
    elif k == 5:
        out = look(1).copy()
        w = out.view(np.uint32)
        a = n - TAIL
        w[a + 1] = w[a]
        w[a + 1, 17] ^= 1                       # one bit of word 17
        w[a + 3] = w[a + 2]
        out[a + 2, SHEEN], out[a + 3, SHEEN] = 0.0, -0.0
        w[a + 5] = w[a + 6] = w[a + 4]
        w[a + 4, ms.IOR] = w[a + 5, ms.IOR] = NAN_A  # the same NaN twice
        w[a + 6, ms.IOR] = NAN_B                   # another payload
        w[n - 1] = w[0]
    else:
        raise ValueError(k)
    out = np.ascontiguousarray(out, F)
    out.setflags(write=False)
    return out


def tris_of(tris, mats):
    """The records with floats 18..35 replaced by mats ((n, 18), bits kept)."""
    out = np.array(tris, F).reshape(-1, 36)
    out.view(np.uint32)[:, 18:36] = np.ascontiguousarray(mats, F).view(np.uint32)
    return out


def expected(mats):
    """-> (table (m, 18) f32, ids (n,) i32): what materials() must return after update_materials(mats), and
    after a fresh upload of records with these materials."""
    m = np.ascontiguousarray(mats, F)
    ids = ms.table_ids(tris_of(np.zeros((m.shape[0], 36), F), m))
    first = np.unique(ids, return_index=True)[1]
    return m[first], ids.astype(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the scenes
@functools.lru_cache(maxsize=None)
def scene_arrays(scene):
    """-> (tris, nodes, hdr, cache, eye, rot, width, height) of "material" or "c2x3"."""
    if scene == "material":
        tris, nodes, hdr, cache, eye, rot = ms.build()[:6]
        return tris, nodes, hdr, cache, eye, rot, ms.W, ms.H
    if scene == "c2x3":
        s = Scene()
        v, i = scenes.bunny_standin()
        for dx in (-2.7, 0.3, 3.3):
            s.add_mesh(v, i, Material(baseColor=(0, 1, 1)), get_transform_matrix((0, 0, 0), (dx, -1.6, 0), (1.5, 1.5, 1.5)), True)
        s.read_obj_text(scenes.QUAD_OBJ, Material(baseColor=(0.725, 0.71, 0.68)),
                        get_transform_matrix((0, 0, 0), (0, -1.4, 0), (18.83, 0.01, 18.83)), False)
        s.read_obj_text(scenes.QUAD_OBJ, Material(baseColor=(1, 1, 1), emissive=(20, 20, 20)),
                        get_transform_matrix((0, 0, 0), (0.0, 1.38, -0.0), (0.7, 0.01, 0.7)), False)
        s.build_bvh("sah", 8)
        tris, nodes = s.encode()
        hdr, cache = ms._env()
        eye, rot = ms.camera(scenes.CONFIGS["c2"].camera)
        return np.ascontiguousarray(tris, F), np.ascontiguousarray(nodes, F), hdr, cache, eye, rot, 64, 64
    raise ValueError(scene)


@functools.lru_cache(maxsize=None)
def c2x3_distinct():
    """A distinct material for every triangle of "c2x3": its own, with a random base colour (the two
    triangles of the light keep theirs and differ in roughness) -> (n, 18) f32."""
    tris = scene_arrays("c2x3")[0]
    n = tris.shape[0]
    out = tris[:, 18:36].copy()
    out[:, ms.BASE] = np.random.RandomState(515).uniform(0.2, 1.0, size=(n, 3)).astype(F)
    out[:, ms.SCALARS["roughness"]] = _ulps(np.full(n, 0.5, F), np.arange(n))
    out.setflags(write=False)
    return out


def mats_of(scene, k):
    """Look k of a scene: looks 0..5 of "material"; of "c2x3" 0 (as built) and 1 (c2x3_distinct)."""
    if scene == "material":
        return look(k)
    return c2x3_distinct() if k else scene_arrays(scene)[0][:, 18:36]


@functools.lru_cache(maxsize=None)
def oracle_frames(scene, k, integrator, max_bounce, frames):
    """The oracle's running mean after each of `frames` frames of look k -> (tuple of (h, w, 4), Counters of the last)."""
    tris, nodes, hdr, cache, eye, rot, w, h = scene_arrays(scene)
    o = oracle.Oracle(tris_of(tris, mats_of(scene, k)), nodes, hdr, cache)
    acc = np.zeros((h, w, 4), F)
    outs, cnt = [], None
    for f in range(frames):
        acc, cnt = o.render(w, h, integrator, f, eye, rot, accum=acc, max_bounce=max_bounce)
        outs.append(acc.copy())
    return tuple(outs), cnt
