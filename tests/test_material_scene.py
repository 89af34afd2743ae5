"""The many-material scene (tests/material_scene.py) on the oracle alone: the inputs of
tests/test_gpu_materials.py exercise what they claim, and the oracle equals the reference's own
shader text on them.

Conditions on the inputs, at 96x64 from material_scene.CAMERA (every figure from the oracle):
the camera sees surfaces, sky and emitters; hundreds of materials reach a first hit, ids above
255 among them, several per 8x8 tile (lanes of one wave hold different materials); paths bounce
on; every Disney parameter, and emission, moves the Disney and MIS images (anisotropic moves
Disney alone: IS:587-636 is the isotropic BRDF). If the geometry misses a condition, change the
geometry or the camera, not the bound.

The reference text: tests/golden/glsl/material_frames.json (tests/golden/make_glsl_fixtures.py
material_frames) holds each shader's own main() on this scene; the oracle's accumulation must
equal it bit for bit. Where the reference is present the comparison also runs live at a second
camera and size.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as dr
import material_scene as ms
import oracle
import ref_glsl

GOLD = Path(__file__).resolve().parent / "golden" / "glsl" / "material_frames.json"
CASES = json.loads(GOLD.read_text())["cases"]
W, H = ms.W, ms.H
SHADED = [("disney", 5), ("mis", 2)]  # the shaders' own bounce counts (D:502, IS:861)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def changed(a, b):
    """Pixels whose bits differ."""
    return int((bits(a) != bits(b)).any(-1).sum())


_base = {}


def base(integ, mb):
    """The oracle's 2-frame image of the scene as built, once per integrator."""
    if (integ, mb) not in _base:
        tris, _, _, _, eye, rot = ms.build()[:6]
        _base[integ, mb] = ms.oracle_frames(tris, integ, mb, 2, eye, rot)[0][-1]
    return _base[integ, mb]


def with_palette(palette):
    tris, ids = ms.build()[0], ms.build()[7]
    return ms.with_materials(tris, palette, ids)


@pytest.fixture(scope="module")
def first_hits():
    """(tri per pixel (-1: miss), material-table id per triangle) of the pixel centres."""
    tris, nodes, _, _, eye, rot = ms.build()[:6]
    _, _, _, tri = dr.guides(oracle.Oracle(tris, nodes), tris, W, H, eye, rot)
    return tri, ms.table_ids(tris)


def test_palette_is_what_the_scene_claims():
    tris, nodes, _, _, _, _, pal, ids = ms.build()
    n = tris.shape[0]
    assert 500 <= n <= 2000 and pal.shape == (ms.N_PALETTE, 18) and ms.N_PALETTE >= 300
    assert np.array_equal(bits(tris[:, 18:36]), bits(pal[ids]))
    # every entry is its own key for the table, and every entry is used
    assert np.unique(bits(pal), axis=0).shape[0] == ms.N_PALETTE
    assert np.unique(ids).size == ms.N_PALETTE and ms.table_ids(tris).max() == ms.N_PALETTE - 1
    # ids recur non-adjacently, neighbouring triangles differ
    assert (ids[1:] != ids[:-1]).mean() > 0.99
    assert np.all((pal[:, 3:] >= 0) & (pal[:, 3:] <= 1.25))
    for name, col in ms.SCALARS.items():
        edge = ((pal[:, col] == 0) | (pal[:, col] == 1)).mean()
        assert 0.12 <= edge <= 0.28, (name, edge)
    lit = pal[:, ms.EMISSIVE].any(1)
    assert 0.04 <= lit.mean() <= 0.12 and pal[lit][:, ms.EMISSIVE].min() >= 0.5 and pal[:, ms.EMISSIVE].max() <= 6
    assert 0.01 <= (~pal[:, ms.BASE].any(1)).mean() <= 0.06
    S, C = ms.SLOTS, ms.SCALARS
    assert pal[S["metal_no_coat"], C["metallic"]] == 1 and pal[S["metal_no_coat"], C["clearcoat"]] == 0
    assert pal[S["mirror"], C["roughness"]] == 0 and pal[S["full_gloss"], C["clearcoatGloss"]] == 1

    def differ(slot):
        return np.nonzero(bits(pal[slot]) != bits(pal[slot + 1]))[0].tolist()

    assert set(differ(S["pair_emissive"])) <= {0, 1, 2} and differ(S["pair_emissive"])
    assert differ(S["pair_ior"]) == [ms.IOR]
    assert differ(S["pair_ulp"]) == [C["roughness"]]
    a, b = bits(pal[S["pair_ulp"]])[C["roughness"]], bits(pal[S["pair_ulp"] + 1])[C["roughness"]]
    assert int(b) - int(a) == 1
    assert differ(S["pair_zero_sign"]) == [C["sheen"]]
    assert pal[S["pair_zero_sign"], C["sheen"]] == pal[S["pair_zero_sign"] + 1, C["sheen"]] == 0


def test_first_hits_reach_many_materials(first_hits):
    tri, tid = first_hits
    tris = ms.build()[0]
    hit = tri >= 0
    share = hit.mean()
    mats = tid[tri[hit]]
    emissive = int(tris[tri[hit], 18:21].any(1).sum())
    m = np.where(hit, tid[np.where(hit, tri, 0)], -1).reshape(H, W)
    tiles = [m[y:y + 8, x:x + 8] for y in range(0, H, 8) for x in range(0, W, 8)]
    per_tile = [np.unique(t[t >= 0]).size for t in tiles if (t >= 0).any()]
    many = sum(k >= 4 for k in per_tile)
    print(f"first-hit share {share:.4f}, distinct materials {np.unique(mats).size}, largest id {mats.max()}, "
          f"emissive first hits {emissive}, tiles with >= 4 materials {many} of {len(per_tile)}")
    assert 0.60 <= share < 0.95  # surfaces, and still sky
    assert np.unique(mats).size >= 200
    assert mats.max() > 255
    assert emissive >= 100
    assert 2 * many >= len(per_tile)


@pytest.mark.parametrize("integ,mb", ms.INTEGRATORS, ids=lambda v: str(v))
def test_oracle_frames_are_finite_and_paths_bounce(integ, mb):
    tris, _, _, _, eye, rot = ms.build()[:6]
    outs, cnt = ms.oracle_frames(tris, integ, mb, 3, eye, rot)
    for f, o in enumerate(outs):
        assert np.isfinite(o).all(), (integ, mb, f)
    rays = cnt.rays / (W * H)
    print(f"{integ} {mb} bounces: {rays:.4f} rays per pixel")
    floor = {("disney", 5): 2.4, ("mis", 8): 2.9}.get((integ, mb))
    if floor:
        assert rays >= floor


@pytest.mark.parametrize("name", list(ms.SCALARS))
def test_every_parameter_moves_the_image(name):
    """The palette column replaced by a constant changes the bits of >= 10 % of the pixels after 2
    frames, for Disney and for MIS -- except anisotropic, which MIS's isotropic BRDF never reads."""
    pal = ms.build()[6].copy()
    pal[:, ms.SCALARS[name]] = 0.5
    tris = with_palette(pal)
    eye, rot = ms.build()[4:6]
    for integ, mb in SHADED:
        n = changed(ms.oracle_frames(tris, integ, mb, 2, eye, rot)[0][-1], base(integ, mb))
        print(f"{name} constant: {integ} {n} of {W * H} pixels change")
        if name == "anisotropic" and integ == "mis":
            assert n == 0
        else:
            assert n >= 0.10 * W * H, (name, integ, n)


def test_emission_moves_the_image():
    pal = ms.build()[6].copy()
    pal[:, ms.EMISSIVE] = 0.0
    tris = with_palette(pal)
    eye, rot = ms.build()[4:6]
    for integ, mb in SHADED:
        n = changed(ms.oracle_frames(tris, integ, mb, 2, eye, rot)[0][-1], base(integ, mb))
        print(f"no emission: {integ} {n} pixels change")
        assert n >= 100, (integ, n)


def test_camera_hit_emission_alone():
    """With every bounce cut off, a pixel holds its camera ray's emissive value, 0 on any other
    surface and the sky texel on a miss (what tests/test_gpu_materials.py asserts of the GPU)."""
    tris, nodes, _, _, eye, rot = ms.build()[:6]
    _, tri, _ = oracle.Oracle(tris, nodes).trace_closest(ms.frame_rays(W, H, eye, rot, 0))
    hit = (tri >= 0).reshape(H, W)
    want = np.where(hit[..., None], tris[np.where(tri >= 0, tri, 0), 18:21].reshape(H, W, 3), 0).astype(np.float32)
    assert (want.any(-1) & hit).sum() >= 100
    for integ in ("disney", "mis"):
        img = ms.oracle_frames(tris, integ, 0, 1, eye, rot)[0][0]
        assert np.array_equal(bits(img[hit][:, :3]), bits(want[hit])), integ
        assert img[~hit][:, :3].any(-1).mean() > 0.9  # the sky


# ------------------------------------------------------------------ the reference text
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["case"])
def test_material_frames_equal_reference_main(case):
    tris, nodes, hdr, cache, eye, rot = ms.build()[:6]
    assert case["camera"] == list(ms.CAMERA) and (case["width"], case["height"]) == (W, H)
    o = oracle.Oracle(tris, nodes, hdr, cache)
    acc = np.zeros((H, W, 4), np.float32)
    for f in range(case["frames"]):
        acc, c = o.render(W, H, case["integrator"], f, eye, rot, accum=acc)
        assert ref_glsl.digest(acc) == case["digests"][f], (case["case"], f)
        got = ref_glsl.canonical(acc.reshape(-1, 4)[case["sample_index"]])
        assert np.array_equal(got, np.asarray(case["sample_frames"][f], np.uint32))
    assert case["sample_frames"][-1] == case["sample_last"]
    assert c.rays > W * H


live = pytest.mark.skipif(not ref_glsl.available(), reason="the reference is absent (the fixture covers it)")


@live
@pytest.mark.parametrize("which,integ", [(0, "lambert"), (1, "disney"), (2, "mis")])
def test_material_frames_live_second_camera(which, integ):
    tris, nodes, hdr, cache = ms.build()[:4]
    eye, rot = ms.camera(ms.CAMERA2)
    w, h = 80, 48  # another aspect and size
    refs = ref_glsl.ref_frames(which, tris, nodes, hdr, cache, eye, rot, 2, w, h)
    outs, _ = ms.oracle_frames(tris, integ, -1, 2, eye, rot, w, h)
    for f in range(2):
        assert np.array_equal(ref_glsl.canonical(outs[f]), ref_glsl.canonical(refs[f])), (integ, f)
