"""The origin domain of the runtime tree without a GPU: the conservativeness argument of the fused slab
tests (csrc/pt_scene_prep.cpp prepareAccel) checked on the product's own widened boxes, which
tests/native/scene_prep_check.cpp dumps, with tests/accel_domain_ref.py's float32 restatement of the
test. Rays are aimed at the oracle's visible points of a 160 x 120 camera of c2 and c4 from origins whose
largest coordinate is R x the scene scale; for every ray the oracle hits, every box from the root to the
winner's leaf must pass, or the walk never reaches the reference's winner.

Measured here (failing chains of ~8600 / ~8960 hits): R = 1, K/2, K, 16 K: 0 and 0; 1e4: 1 and 2; 3e4: 14
and 11; 1e5: 106 and 18; 1e6: 134 and 6 -- K = 32, PT_ORIGIN_K. The derivation is a worst case (three
roundings of half an ulp each, all one way); the rays here first lose a winner ~300 K out. Tried once on
a scratch copy with the 3e-5 widening cut to 1/16: still no failing chain out to R = 2048 on either scene
(each box keeps the 1e-5 of its own magnitude), so the chains do not notice that cut; the constants do:
test_the_figure_follows_from_the_widening reads both figures from the sources and fails for that cut
(4 x 5.8e-6 > 1.9e-6) as for PT_ORIGIN_K raised 16x (4 x 9.2e-5 > 3e-5).

Also here, on the oracle alone: the inputs of the GPU tests of far origins and of scaled and translated
scenes (test_gpu_far_origins.py, test_gpu_scaled_scenes.py) do what they are there for."""
import functools

import numpy as np
import pytest

import accel_domain_ref as ad
import denoise_ref
import oracle

F = np.float32
CONFIGS = ["c2", "c4"]


@functools.lru_cache(maxsize=None)
def tree(name):
    m = ad.model(name)
    dump = ad.prepare(m["tris"], m["nodes"])
    return dump, ad.Chains(dump)


def failing(name, reach):
    m = ad.model(name)
    _, chains = tree(name)
    rays = ad.aimed_rays(m["P"], m["d"], reach)
    t, tri = ad.oracle_hits(m["orc"], rays)
    bad = ad.failing_chains(chains, rays, tri)
    share = float((tri >= 0).mean())
    print(f"{name} reach {float(reach):.6g}: oracle hit share {share:.4f}, failing chains {int(bad.sum())} of {int((tri >= 0).sum())}")
    return int(bad.sum()), share


def test_the_figure_follows_from_the_widening():
    """PT_ORIGIN_K is the largest power of two that leaves a factor 4 between the rounding of one fused
    slab value, (3 K + 2) 2^-24 of the scene scale, and the least widening any box gets; and no more than
    the 100 the documents claimed before."""
    K, rel = ad.constants()
    print("K", K, "widening", rel, "rounding at K", (3 * K + 2) * 2.0 ** -24)
    assert K == 2.0 ** round(np.log2(K)) and K <= 100
    assert 4 * (3 * K + 2) * 2.0 ** -24 <= rel
    assert 4 * (3 * (2 * K) + 2) * 2.0 ** -24 > rel


@pytest.mark.parametrize("name", CONFIGS)
def test_the_dump_is_the_scene_model(name):
    """The scale the dumped tree was widened by is the largest vertex coordinate, the one the tests use."""
    dump, chains = tree(name)
    assert F(dump["sceneScale"][0]) == ad.model(name)["scale"]
    assert chains.n.min() >= 1 and len(chains.n) == len(ad.model(name)["tris"])


@pytest.mark.parametrize("name", CONFIGS)
def test_no_chain_fails_out_to_16K(name):
    """In the domain, and 16 times beyond it -- the safety margin this test pins: trimming the widening
    fails here."""
    K, s = F(ad.constants()[0]), ad.model(name)["scale"]
    for R in (F(1), K / F(2), K, F(16) * K):
        bad, share = failing(name, R * s)
        assert bad == 0, (name, float(R))
        assert share >= 0.9


@pytest.mark.parametrize("name", CONFIGS)
@pytest.mark.parametrize("R", [1e5, 1e6])
def test_chains_fail_far_outside(name, R):
    """... and the model is not vacuous: far enough out the fused walk does lose winners the reference
    reaches (which is why the domain is enforced, not assumed)."""
    bad, share = failing(name, F(R) * ad.model(name)["scale"])
    assert bad >= 1
    assert share >= 0.9


@pytest.mark.parametrize("name", CONFIGS)
def test_far_ray_sets_hit(name):
    """The ray sets of test_gpu_far_origins.py: at every distance the oracle hits with 0.9 of them or more,
    and the origins sit on the side of the limit their name says."""
    m = ad.model(name)
    for reach_name, reach in ad.far_reaches(name).items():
        rays, t, tri = ad.far_rays(name, reach_name)
        share = float((tri >= 0).mean())
        inside = bool((np.abs(rays[:, 0:3]).max(axis=1) <= m["limit"]).all())
        print(name, reach_name, float(reach), "hit share", round(share, 4), "in domain", inside)
        assert share >= 0.9
        assert np.array_equal(np.abs(rays[:, 0:3]).max(axis=1), np.full(len(rays), reach, F))
        assert inside == (reach_name in ("1", "K/2", "K"))


def camera_hits(tris, nodes, eye, rot, w, h):
    rays = denoise_ref.camera_rays(w, h, eye, rot)
    t, tri = ad.oracle_hits(oracle.Oracle(tris, nodes), rays)
    return rays, t, tri


def test_translation_defeats_the_margin_test():
    """refReachable's cheap answer (pt_trace.h insideByMargin on the hit's reference leaf box) against
    c2's 160 x 120 camera hits, plain and translated by 2^12 on every axis. Shares of hits that fail it:

                                                  plain    2^12
      of the hits whose leaf box has an extent    0.036    1.000   <- asserted: < 1/2, > 1/2
      of all hits                                 0.863    1.000
      leaving the cheap path (flat rule too)      0.005    0.169

    86 % of c2's hits lie in leaves whose box is flat in one axis (walls, floor), which insideByMargin can
    never pass and refReachableBox answers with its flat-leaf rule: over all hits the plain scene already
    fails the margin test for 0.863, so the comparison is made where the test can pass at all. Translated,
    the margin (2^-14 of a scale that includes the coordinates' magnitude, ~0.75 units here) exceeds every
    leaf box: every hit takes the flat rule or the walk up the reference path."""
    m = ad.model("c2")
    shares = {}
    for what, (tris, nodes, eye) in {
            "plain": (m["tris"], m["nodes"], m["eye"]),
            "2^12": ad.translated_scene(m["tris"], m["nodes"], m["eye"], 12)}.items():
        rays, t, tri = camera_hits(tris, nodes, eye, m["rot"], 160, 120)
        box = ad.prepare(tris, nodes)["leafBox"]
        ok = ad.inside_by_margin(rays, t, tri, box)
        flat_ok = ad.flat_leaf_rule(rays, tri, box)
        b = box.reshape(-1, 2, 4)[tri[tri >= 0]]
        extent = ~(b[:, 0, 0:3] == b[:, 1, 0:3]).any(axis=1)
        shares[what] = (1 - ok[extent].mean(), 1 - ok.mean(), 1 - (ok | flat_ok).mean())
        print(what, "hits", len(ok), "with an extent", int(extent.sum()), "fail shares", shares[what])
        assert extent.sum() >= 1000
    assert shares["plain"][0] < 0.5 < shares["2^12"][0]
    assert shares["2^12"][1] > 0.5
    assert shares["plain"][2] < shares["2^12"][2]


def test_translation_by_2_16_takes_the_walk_up_the_reference_path():
    """... and of the translations the GPU tests use, 2^16 is the one that sends most hits past the flat-leaf
    rule as well, into refReachable's hitAABB walk up refParent: 0.739 of c2's hits (2^12: 0.169)."""
    m = ad.model("c2")
    tris, nodes, eye = ad.translated_scene(m["tris"], m["nodes"], m["eye"], 16)
    rays, t, tri = camera_hits(tris, nodes, eye, m["rot"], 160, 120)
    box = ad.prepare(tris, nodes)["leafBox"]
    slow = 1 - (ad.inside_by_margin(rays, t, tri, box) | ad.flat_leaf_rule(rays, tri, box)).mean()
    print("2^16: share of hits on the walk up the reference path", slow)
    assert slow > 0.5


# ------------------------------------------------------------------ the scaled and translated scenes' inputs
SCALES = [-13, -10, 10, 14, 20]
SHIFTS = [8, 12, 16]


def test_scaled_and_translated_cameras_hit():
    """c2's 33 x 31 camera on the scene scaled by 2^e and translated by 2^p, on the oracle alone: the hit
    share is the plain scene's (0.444) except at 2^-13, where part of the hits fall under hitTriangle's
    t >= 0.0005 and the share lies strictly between 0.05 and 0.44 (0.233)."""
    m = ad.model("c2")
    plain = (camera_hits(m["tris"], m["nodes"], m["eye"], m["rot"], 33, 31)[2] >= 0).mean()
    assert round(float(plain), 3) == 0.444
    for e in SCALES:
        tris, nodes, eye = ad.scaled_scene(m["tris"], m["nodes"], m["eye"], e)
        share = (camera_hits(tris, nodes, eye, m["rot"], 33, 31)[2] >= 0).mean()
        print("scaled 2^%d" % e, share)
        if e >= -10:
            assert share == plain
        else:
            assert 0.05 < share < 0.44
    for p in SHIFTS:
        tris, nodes, eye = ad.translated_scene(m["tris"], m["nodes"], m["eye"], p)
        share = (camera_hits(tris, nodes, eye, m["rot"], 33, 31)[2] >= 0).mean()
        print("translated 2^%d" % p, share)
        assert share == plain


@pytest.mark.parametrize("name", CONFIGS)
def test_every_dumped_plane_is_widened(name):
    """The product's boxes, not its source text: every plane of the host-built tree's wide records
    (fastTree.bvh) lies at least 3e-5 x the scene scale outside the plane of the node it was made from (the
    dump's accelRef, the builder's nodes before the widening), which is the figure PT_ORIGIN_K is derived
    against. (The subtraction's own rounding, half an ulp of the plane, is covered by the further 1e-5 of
    the box's magnitude every plane gets.) A widening trimmed inside encodeWideTree fails here."""
    dump, _ = tree(name)
    _, rel = ad.constants()
    rec = dump["fastTree.bvh"].reshape(-1, 16)
    ids = dump["fastTree.ids"]
    ref = dump["accelRef"].reshape(-1, 12)
    s = np.float64(dump["sceneScale"][0])
    least = np.float64(F(rel) * F(s))
    refs = rec[:, 12:14].copy().view(np.int32)
    assert len(ids) == len(rec) and len(rec) > 100
    gaps = []
    for c in range(2):
        used = refs[:, c] != ad.REF_NONE
        kid = ref[ids, c].astype(np.int64)[used]
        assert (kid > 0).all()
        for a in range(3):
            gaps.append(ref[kid, 6 + a].astype(np.float64) - rec[used, 2 * a + c].astype(np.float64))
            gaps.append(rec[used, 6 + 2 * a + c].astype(np.float64) - ref[kid, 9 + a].astype(np.float64))
    gaps = np.concatenate(gaps)
    print(name, "planes", gaps.size, "least gap / (3e-5 s)", gaps.min() / least, "largest", gaps.max() / least)
    assert gaps.min() >= least
    assert gaps.max() <= 2.5 * least   # ... and no more than 1e-5 (|lo| + |hi| + extent) <= 4e-5 s beyond it: 7/3 in all
