"""A small scene with hundreds of materials -- TEST INFRASTRUCTURE ONLY.

Every other scene of the suite has one or two materials, most of whose Disney parameters are 0.
This one is a bumpy UV sphere (30 x 31) with 35 % of its faces removed, seen from inside, so the
camera sees surfaces, paths bounce among them and still leave through the holes to the sky. After
encode(), floats 18..35 of every triangle record are overwritten from a palette of N_PALETTE
random materials, one random palette index per triangle (every entry is used at least once, ids
recur non-adjacently and neighbouring triangles differ):

  * every scalar parameter is uniform in [0, 1]; each of the ten shaded scalars (SCALARS) is
    exactly 0 or 1 in about 20 % of the entries;
  * about 8 % of the entries are emissive (0.5 .. 6 per channel), about 3 % have baseColor (0,0,0);
  * fixed slots (SLOTS): metallic 1 with clearcoat 0, roughness 0, clearcoatGloss 1, and four pairs
    that differ only in emissive, only in IOR (not shaded), by one ulp of roughness, and only in
    the sign of a zero sheen -- all distinct keys for the runtime's material table
    (pt_scene_prep.cpp prepareScene compares floats 18..35 bit for bit).

Used by tests/test_material_scene.py (the oracle alone: the inputs exercise what they claim),
tests/test_gpu_materials.py (the frame kernels against the oracle, bit for bit) and
tests/golden/make_glsl_fixtures.py (the reference shader text on this scene).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle
from opengl_ray_tracing_amd import Material, Scene, orbit_camera, scenes

SEED = 7151
W, H = 96, 64
CAMERA = (25.0, 20.0, 0.5)
CAMERA2 = (200.0, -15.0, 0.4)  # the second camera of the live comparison and of the camera move
N_PALETTE = 400
HOLES = 0.35  # share of the sphere's faces removed

# palette columns (Triangle_encoded float 18 + column)
EMISSIVE, BASE = slice(0, 3), slice(3, 6)
SCALARS = {"subsurface": 6, "metallic": 7, "specular": 8, "specularTint": 9, "roughness": 10, "anisotropic": 11,
           "sheen": 12, "sheenTint": 13, "clearcoat": 14, "clearcoatGloss": 15}
IOR, TRANSMISSION = 16, 17
# fixed palette slots: the edge entries, and the first entry of each pair (the second is slot + 1)
SLOTS = {"metal_no_coat": 0, "mirror": 1, "full_gloss": 2, "pair_emissive": 3, "pair_ior": 5, "pair_ulp": 7,
         "pair_zero_sign": 9}
INTEGRATORS = [("lambert", 2), ("disney", 5), ("mis", 2), ("mis", 8)]


def make_palette(rs: np.random.RandomState) -> np.ndarray:
    n = N_PALETTE
    p = rs.uniform(0.0, 1.0, size=(n, 18)).astype(np.float32)
    p[:, EMISSIVE] = 0.0
    for col in SCALARS.values():
        pick = rs.uniform(size=n) < 0.2
        p[pick, col] = rs.choice(np.array([0.0, 1.0], np.float32), size=int(pick.sum()))
    lit = rs.uniform(size=n) < 0.08
    p[lit, EMISSIVE] = rs.uniform(0.5, 6.0, size=(int(lit.sum()), 3)).astype(np.float32)
    black = rs.uniform(size=n) < 0.03
    p[black, BASE] = 0.0
    s = SLOTS
    p[s["metal_no_coat"], SCALARS["metallic"]] = 1.0
    p[s["metal_no_coat"], SCALARS["clearcoat"]] = 0.0
    p[s["mirror"], SCALARS["roughness"]] = 0.0
    p[s["full_gloss"], SCALARS["clearcoatGloss"]] = 1.0
    for k in ("pair_emissive", "pair_ior", "pair_ulp", "pair_zero_sign"):
        p[s[k] + 1] = p[s[k]]
    p[s["pair_emissive"], EMISSIVE] = 0.0
    p[s["pair_emissive"] + 1, EMISSIVE] = (2.0, 1.0, 0.5)
    p[s["pair_ior"] + 1, IOR] = p[s["pair_ior"], IOR] + np.float32(0.25)
    rough = np.float32(0.37)
    p[s["pair_ulp"], SCALARS["roughness"]] = rough
    p[s["pair_ulp"] + 1, SCALARS["roughness"]] = np.nextafter(rough, np.float32(1.0))
    p[s["pair_zero_sign"], SCALARS["sheen"]] = 0.0
    p[s["pair_zero_sign"] + 1, SCALARS["sheen"]] = -0.0
    return p


def with_materials(geometry: np.ndarray, palette: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """A copy of the triangle records with floats 18..35 of triangle k = palette[ids[k]]."""
    t = np.array(geometry, np.float32).reshape(-1, 36)
    t[:, 18:36] = np.asarray(palette, np.float32)[np.asarray(ids)]
    return t


def table_ids(tris: np.ndarray) -> np.ndarray:
    """The material id the runtime gives each triangle (pt_scene_prep.cpp prepareScene): distinct keys
    (floats 18..35, bit for bit) numbered by their first appearance in triangle order."""
    keys = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 36)[:, 18:36]).view(np.uint32)
    seen, out = {}, np.empty(keys.shape[0], np.int64)
    for k, row in enumerate(keys):
        out[k] = seen.setdefault(row.tobytes(), len(seen))
    return out


@functools.lru_cache(maxsize=None)
def _env():
    hdr = np.ascontiguousarray(scenes.load_hdr(scenes.HDR_FILES["peppermint"]), np.float32)
    return hdr, np.ascontiguousarray(oracle.hdr_cache(hdr), np.float32)


def camera(angles):
    eye, rot = orbit_camera(*angles)
    return np.ascontiguousarray(eye, np.float32), np.ascontiguousarray(rot, np.float32).reshape(16)


@functools.lru_cache(maxsize=None)
def build():
    """-> (tris, nodes, hdr, cache, eye, rot, palette, ids); shared between tests: do not write to them."""
    rs = np.random.RandomState(SEED)
    v, idx = scenes.uv_sphere(30, 31, lambda u, t: 1.0 + 0.12 * math.sin(5 * u) * math.sin(4 * t))
    idx = idx[rs.uniform(size=len(idx)) >= HOLES]
    s = Scene()
    s.add_mesh(v, idx, Material(), None, True)
    s.build_bvh("binned", 4)
    geometry, nodes = s.encode()
    n = geometry.shape[0]
    palette = make_palette(rs)
    ids = np.concatenate([rs.permutation(N_PALETTE), rs.randint(0, N_PALETTE, size=n - N_PALETTE)])
    ids = ids[rs.permutation(n)]
    tris = with_materials(geometry, palette, ids)
    hdr, cache = _env()
    eye, rot = camera(CAMERA)
    return tris, np.ascontiguousarray(nodes, np.float32), hdr, cache, eye, rot, palette, ids


def frame_rays(w: int, h: int, eye, rot, frame: int = 0) -> np.ndarray:
    """The jittered camera ray of every pixel in frame `frame` (IS:846-850, oracle/pt_oracle.c
    shade_gl_pixel: the pixel's first two random draws) -> (h * w, 6) origin, direction."""
    F = np.float32
    M = np.ascontiguousarray(rot, F).reshape(16)
    px = np.tile(np.arange(w, dtype=np.int64), h)
    py = np.repeat(np.arange(h, dtype=np.int64), w)
    r = np.stack([oracle.pixel_rng(int(x), int(y), frame, 2) for x, y in zip(px, py)]).astype(F)
    x = ((2 * px + 1).astype(F) / F(w) - F(1)) + (r[:, 0] - F(0.5)) / F(w)
    y = ((2 * py + 1).astype(F) / F(h) - F(1)) + (r[:, 1] - F(0.5)) / F(h)
    z = F(-1.5)
    d = [(M[0 + k] * x + M[4 + k] * y) + (M[8 + k] * z + M[12 + k] * F(0)) for k in range(3)]
    inv = F(1) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    rays = np.empty((w * h, 6), F)
    rays[:, 0:3] = np.ascontiguousarray(eye, F).reshape(3)
    for k in range(3):
        rays[:, 3 + k] = d[k] * inv
    return rays


def oracle_frames(tris, integrator, max_bounce, frames, eye, rot, w=W, h=H):
    """The oracle's running mean after each of `frames` frames -> (list of (h, w, 4), Counters of the last)."""
    _, nodes, hdr, cache = build()[:4]
    o = oracle.Oracle(tris, nodes, hdr, cache)
    acc = np.zeros((h, w, 4), np.float32)
    outs, cnt = [], None
    for f in range(frames):
        acc, cnt = o.render(w, h, integrator, f, eye, rot, accum=acc, max_bounce=max_bounce)
        outs.append(acc.copy())
    return outs, cnt
