"""The environment updated in place on the GPU (pt_update_env, pt_update_env_device, pt_download_env,
pt_env_size; csrc/pt_envupdate.hip) against its specification: after update_env(map) a context is what
upload_env of the same map would have made it -- the float texels and table, env_compact, and the
images of every integrator, which equal the oracle's for that map bit for bit. The compact forms are
checked against the float ones through the frame kernels' own decoders (download_env forms 1 and 2),
which does not depend on how the rows are numbered. PT_ENV_RGBE is checked against
tests/env_update_ref.py.

Maps: tests/env_maps.py and test_gpu_env's FORM_MAPS, callers_table and banded_map. 64 x 40 pixels,
2 frames, c2's mesh. Oracle images are computed once per (map, table, integrator) and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import env_maps
import env_update_ref as eu
from opengl_ray_tracing_amd import FLAG_MEGAKERNEL, Renderer, calculate_hdr_cache, orbit_camera, scenes
from post_common import INVALID, bits, rc_of
from test_gpu_env import (FORM_MAPS, FRAMES, H, INTEGRATORS, W, assert_equals_oracle, banded_map, callers_table, gpu_frames,
                          oracle_frames)

pytestmark = pytest.mark.gpu
F = np.float32


@functools.lru_cache(maxsize=None)
def mesh():
    cfg, tris, nodes, _ = scenes.build_config("c2")
    eye, rot = orbit_camera(*cfg.camera)
    return tris, nodes, eye, rot


def tensor(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, F)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def renderer(integrator="lambert", mb=2, w=W, h=H, flags=0, **kw):
    tris, nodes, _, _ = mesh()
    r = Renderer(w, h, integrator, max_bounce=mb, flags=flags, **kw)
    r.upload_scene(tris, nodes)
    return r


def frames_of(r, mode="stream", frames=FRAMES):
    _, _, eye, rot = mesh()
    if mode == "call":
        for f in range(frames):
            r.render_frame(eye, rot, f)
    else:
        r.render_frames(eye, rot, 0, frames)
    r.synchronize()
    return r.accum().copy()


_ORACLE = {}


def oracle_image(key, hdr, cache, integrator, mb, w=W, h=H):
    """The oracle's running mean after FRAMES frames of the map, computed once per key."""
    k = (key, integrator, mb, w, h)
    if k not in _ORACLE:
        tris, nodes, eye, rot = mesh()
        _ORACLE[k] = oracle_frames(tris, nodes, hdr, cache, w, h, integrator, mb, eye, rot, FRAMES)
    return _ORACLE[k]


def same_env(a, b, what):
    for x, y, part in zip(a, b, ("texels", "table")):
        assert env_maps.same_bits_or_nan(x, y), (what, part)


def assert_quantised(r, src, what):
    """download_env(0)'s colours are env_update_ref.quantise(src), bit for bit; the differing texels otherwise."""
    got, want = r.download_env(0)[0][..., :3].reshape(-1, 3), eu.quantise(src).reshape(-1, 3)
    bad = np.nonzero((bits(got) != bits(want)).any(-1))[0]
    assert bad.size == 0, (what, bad[:8], src.reshape(-1, 3)[bad[:8]], got[bad[:8]], want[bad[:8]])


def check_compact_forms(r, what):
    """Forms 1 and 2 of download_env, wherever env_compact allows them, equal form 0 bit for bit."""
    compact = r.stats().env_compact
    t0 = r.download_env(0)
    if compact >= 1:
        same_env(r.download_env(1), t0, f"{what}: compact forms")
    if compact >= 2:
        none, table = r.download_env(2)
        assert none is None and env_maps.same_bits_or_nan(table, t0[1]), f"{what}: row form"
    return compact


# ------------------------------------------------------------------ 1. state
@pytest.fixture(scope="module")
def state_contexts():
    with Renderer(8, 8) as a, Renderer(8, 8) as b, Renderer(8, 8) as c:
        yield a, b, c


@pytest.mark.parametrize("name", env_maps.CACHE_MAP_NAMES)
def test_state_equals_a_fresh_upload(state_contexts, name):
    """The three contexts serve every map in turn, so every update but the first replaces an environment
    of another size (and the upload replaces an update's store)."""
    up, dev, host = state_contexts
    hdr = env_maps.cache_maps()[name]
    h, w = hdr.shape[:2]
    up.update_env(env_maps.constant_map(3, 2))  # upload_env takes over from an update's store
    up.upload_env(hdr)
    dev.update_env(tensor(hdr))
    host.update_env(hdr)
    want = up.download_env(0)
    assert env_maps.same_bits_or_nan(want[0][..., :3], hdr)
    assert env_maps.same_bits_or_nan(np.dstack([want[1], want[0][..., 3:]]), calculate_hdr_cache(hdr))
    compact = check_compact_forms(up, f"{name}/upload")
    for r, form in ((dev, "device"), (host, "host")):
        assert r.env_size() == (w, h)
        same_env(r.download_env(0), want, f"{name}/{form}")
        assert r.stats().env_compact == compact, (name, form)
        check_compact_forms(r, f"{name}/{form}")


# ------------------------------------------------------------------ 2. images against the oracle
@pytest.mark.parametrize("integrator,mb", INTEGRATORS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(FORM_MAPS))
def test_images_through_the_device_form(name, integrator, mb):
    hdr = FORM_MAPS[name]()
    ref = oracle_image(name, hdr, None, integrator, mb)
    d = tensor(hdr)
    with renderer(integrator, mb) as r:
        for mode in ("stream", "call"):
            r.update_env(d)
            g = frames_of(r, mode)
            assert r.stats().env_compact == 2, (name, mode)
            assert_equals_oracle(g, ref, f"{name}/{integrator}{mb}/{mode}")


@pytest.mark.parametrize("entry,compact", [(None, 1), ((9, 20, 0, 0.3), 0), ("above one", 0)], ids=["shuffled", "0.3", "above one"])
def test_callers_table_through_the_device_form(entry, compact):
    hdr = FORM_MAPS["random 37x19"]()
    table = callers_table(hdr)
    if entry == "above one":
        table[9, 20, 0] = F(2.0)
        table[4, 30, 1] = F(3.0)
    elif entry is not None:
        table[entry[0], entry[1], entry[2]] = F(entry[3])
    ref = oracle_image(f"caller's table {entry}", hdr, table, "mis", 2)
    d, dt = tensor(hdr), tensor(table)
    with renderer("mis", 2) as r:
        for mode in ("stream", "call"):
            r.update_env(d, dt)
            g = frames_of(r, mode)
            assert r.stats().env_compact == compact, (entry, mode)
            assert_equals_oracle(g, ref, f"caller's table {entry}/{mode}")
        check_compact_forms(r, f"caller's table {entry}")
        t, tab = r.download_env(0)
        assert env_maps.same_bits_or_nan(np.dstack([tab, t[..., 3:]]), table)


def test_table_by_rows_with_ids_reused():
    hdr = banded_map()
    w, h = 48, 32
    ref = oracle_image("banded 1500x700", hdr, None, "mis", 4, w, h)
    with renderer("mis", 4, w, h, flags=FLAG_MEGAKERNEL) as r:
        r.update_env(tensor(hdr))
        g = frames_of(r)
        assert r.stats().env_compact == 2
        assert_equals_oracle(g, ref, "table by rows 1500x700")
        check_compact_forms(r, "banded 1500x700")
    tris, nodes, eye, rot = mesh()
    fresh, compact = gpu_frames(tris, nodes, hdr, None, w, h, "mis", 4, eye, rot, FRAMES, "stream", flags=FLAG_MEGAKERNEL)
    assert compact == 2 and np.array_equal(bits(g), bits(fresh))


# ------------------------------------------------------------------ 3. a sequence on one context
def test_sequence_on_one_context():
    import torch
    a, b, c = env_maps.random_map(37, 19, 21), env_maps.random_map(100, 50, 22), env_maps.random_map(100, 50, 41)
    raw = eu.unquantised_map(100, 50, 42)
    maps = {"a": a, "b": b, "c": c, "raw": raw}
    ref = {k: oracle_image(f"sequence {k}", m, None, "mis", 2) for k, m in maps.items()}
    dev = {k: tensor(m) for k, m in maps.items()}
    with renderer("mis", 2) as r:
        r.upload_env(a)
        first = frames_of(r)
        assert_equals_oracle(first, ref["a"], "1 upload 37x19")
        r.update_env(dev["b"])
        assert_equals_oracle(frames_of(r), ref["b"], "2 update 100x50")
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        r.update_env(dev["c"])
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free  # nothing allocated, nothing freed
        assert r.stats().env_compact == 2
        assert_equals_oracle(frames_of(r), ref["c"], "3 update another 100x50")
        r.update_env(dev["raw"])
        assert r.stats().env_compact == 0
        assert_equals_oracle(frames_of(r), ref["raw"], "4 update an unquantised map")
        r.update_env(dev["b"])
        assert r.stats().env_compact == 2
        assert_equals_oracle(frames_of(r), ref["b"], "5 update an RGBE map again")
        r.update_env(dev["a"])
        last = frames_of(r)
        assert_equals_oracle(last, ref["a"], "6 update the first map")
        assert np.array_equal(bits(last), bits(first))


# ------------------------------------------------------------------ 4. PT_ENV_RGBE
def test_rgbe_flag():
    raw = eu.unquantised_map(37, 19, 43)
    edged = raw.copy()
    t, _ = eu.edge_texels()
    edged.reshape(-1, 3)[5:5 + t.shape[0]] = t
    with renderer("mis", 2) as r, renderer("lambert", 2) as lam:
        for form in (tensor, np.array):
            r.update_env(form(raw), rgbe=True)
            assert_quantised(r, raw, "PT_ENV_RGBE")
            assert r.stats().env_compact == 2
            assert_equals_oracle(frames_of(r), oracle_image("rgbe", eu.quantise(raw), None, "mis", 2), "PT_ENV_RGBE")
            check_compact_forms(r, "PT_ENV_RGBE")
            # the same map without the flag: the raw floats, and the float forms
            r.update_env(form(raw))
            assert env_maps.same_bits_or_nan(r.download_env(0)[0][..., :3], raw)
            assert r.stats().env_compact == 0
            assert_equals_oracle(frames_of(r), oracle_image("raw", raw, None, "mis", 2), "without PT_ENV_RGBE")
            # the edge texels: negative, -0, NaN, inf, subnormal, around 1e-32f, 255 * 2^119 and above
            lam.update_env(form(edged), rgbe=True)
            assert_quantised(lam, edged, "PT_ENV_RGBE, edge texels")
            check_compact_forms(lam, "PT_ENV_RGBE, edge texels")
            assert_equals_oracle(frames_of(lam), oracle_image("edged", eu.quantise(edged), None, "lambert", 2), "edge texels")
        # with PT_ENV_RGBE a caller's table is used as given
        table = calculate_hdr_cache(raw)
        r.update_env(tensor(raw), tensor(table), rgbe=True)
        tex, tab = r.download_env(0)
        assert env_maps.same_bits_or_nan(tex[..., :3], eu.quantise(raw))
        assert env_maps.same_bits_or_nan(np.dstack([tab, tex[..., 3:]]), table)


# ------------------------------------------------------------------ 5. stream order
def test_stream_order():
    import torch
    hdr = env_maps.random_map(100, 50, 22)
    rolled = np.ascontiguousarray(np.roll(hdr, 7, axis=1) * F(2))  # RGBE-exact: a roll and a power of two
    assert np.array_equal(env_maps.rgbe_quantise(rolled), rolled)
    ref = oracle_image("rolled", rolled, None, "mis", 2)
    ref2 = oracle_image("sequence b", hdr, None, "mis", 2)
    base = tensor(hdr)
    x = torch.randn(2048, 2048, device="cuda:0")
    torch.cuda.synchronize()
    _, _, eye, rot = mesh()
    s = torch.cuda.Stream()
    with renderer("mis", 2) as r:
        r.upload_env(env_maps.constant_map(37, 19))
        r.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            for _ in range(20):  # a long kernel ahead of the map's producer, and no synchronisation after it
                x = (x @ x) * 1e-3
            d = (torch.roll(base, 7, 1) * 2.0).contiguous()
            r.update_env(d)
        assert r.stats().env_compact == 2
        assert_equals_oracle(frames_of(r), ref, "map produced on the context's stream")
        with torch.cuda.stream(s):
            r.render_frames(eye, rot, 0, 8)  # in flight
            r.update_env(base)  # waits for them
        assert_equals_oracle(frames_of(r), ref2, "update behind frames in flight")
        r.set_stream(None)
        for bad in (d[:, :, :2], d.double(), d.cpu(), d.permute(1, 0, 2), d.reshape(-1, 3)):
            with pytest.raises(ValueError):
                r.update_env(bad)
        with pytest.raises(ValueError):
            r.update_env(d, tensor(hdr[:10]))


# ------------------------------------------------------------------ 6. what follows the update
def test_history_moments_guides_bins_and_queries_follow_the_update():
    old, new = env_maps.random_map(37, 19, 21), env_maps.random_map(100, 50, 22)
    tris, nodes, eye, rot = mesh()
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(512, 3)).astype(F)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(np.asarray(eye, F), dirs.shape), dirs], 1).astype(F)
    with renderer("lambert", 2, moments=True) as a, renderer("lambert", 2, moments=True) as b:
        a.upload_env(old)
        b.upload_env(new)
        a.render_frames(eye, rot, 0, 4)
        a.render_guides(eye, rot)
        a.temporal_resolve(4, download=False)
        a.temporal_commit()
        assert a.moments_frames() == 4
        t0, tri0 = a.trace_closest(rays)
        miss = tri0 < 0
        assert miss.sum() > 32 and (~miss).any()
        before = a.radiance(rays[miss])
        a.update_env(tensor(new))
        assert a.moments_frames() == 0
        t1, tri1 = a.trace_closest(rays)
        assert np.array_equal(tri1, tri0) and np.array_equal(bits(t1), bits(t0))
        a.reset_stats()
        for r in (a, b):
            r.render_frames(eye, rot, 0, 4)  # the same camera: a's camera-ray bins are kept
            r.synchronize()
        acc = a.accum()
        assert np.array_equal(bits(acc), bits(b.accum()))
        assert a.stats().rays == b.stats().rays
        res = a.temporal_resolve(4)  # the guides are still accepted; no history: the accumulation's rgb
        assert np.array_equal(bits(res[..., :3]), bits(acc[..., :3]))
        a.denoise()
        got = a.radiance(rays[miss])
        assert np.array_equal(bits(got), bits(b.radiance(rays[miss])))
        texels = {tuple(t) for t in bits(np.minimum(new, F(10))).reshape(-1, 3)}  # sampleHdr clamps at 10
        assert all(tuple(c) in texels for c in bits(got[:, :3])) and not np.array_equal(bits(got), bits(before))


# ------------------------------------------------------------------ 7. clear
def test_clear():
    """(Lambert: MIS under a black sky divides by a zero pdf, and a NaN pixel of the accumulation outlives
    the restart at frame_counter 0 -- after upload_env(None) just as well.)"""
    hdr = env_maps.random_map(37, 19, 21)
    d = tensor(hdr)
    with renderer("lambert", 2) as r, renderer("lambert", 2) as fresh:
        fresh.upload_env(hdr)
        fresh.upload_env(None)
        black = frames_of(fresh)
        for clear in (lambda: r.update_env(None), lambda: r._ck(r._lib.pt_update_env_device(r._h, None, 0, 0, None, 0), "clear")):
            r.update_env(d)
            assert r.env_size() == (37, 19)
            clear()
            assert r.env_size() == (0, 0) and r.stats().env_compact == 0
            assert np.array_equal(bits(frames_of(r)), bits(black))
            assert rc_of(r.download_env, 0) == INVALID
        r.update_env(d)  # and back
        assert_equals_oracle(frames_of(r), oracle_image("random 37x19", FORM_MAPS["random 37x19"](), None, "lambert", 2), "after a clear")


# ------------------------------------------------------------------ 8. a device group
def test_device_group():
    hdr = FORM_MAPS["random 100x50"]()
    ref = oracle_image("random 100x50", hdr, None, "mis", 2)
    with renderer("mis", 2, devices=[0, 0]) as r:
        r.upload_env(env_maps.constant_map(37, 19))
        assert rc_of(r.update_env, tensor(hdr)) == INVALID
        assert "n_devices" in r._lib.pt_last_error(r._h).decode()
        r.update_env(hdr)
        assert_equals_oracle(frames_of(r, "call"), ref, "device group, host form")
        assert r.stats().env_compact == 2


# ------------------------------------------------------------------ 9. error paths
def test_error_paths():
    hdr = FORM_MAPS["random 37x19"]()
    ref = oracle_image("random 37x19", hdr, None, "mis", 2)
    raw = eu.unquantised_map(37, 19, 43)
    d = tensor(hdr)
    fp = hdr.ctypes.data_as(C.POINTER(C.c_float))
    dp = C.c_void_p(d.data_ptr())
    out = np.zeros((19, 37, 4), F)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    with renderer("mis", 2) as r:
        lib, hnd = r._lib, r._h
        r.update_env(d)
        bad = [(37, 0, 0), (0, 19, 0), (-37, 19, 0), (37, -1, 0),            # w <= 0 or h <= 0
               (65536, 65536, 0), (1 << 30, 4, 0),                             # w * h does not fit an int
               (30000, 30000, 0), (46340, 46340, 0),                           # 3 * w * h / the table scratch do not
               (37, 19, 2), (37, 19, 0x80000000), (37, 19, 3)]                 # unknown flag bits
        for w, h, flags in bad:
            for form, arg in ((lib.pt_update_env, fp), (lib.pt_update_env_device, dp)):
                assert form(hnd, arg, w, h, None, flags) == INVALID, (w, h, flags)
                assert lib.pt_last_error(hnd), (w, h, flags)
            assert r.env_size() == (37, 19)
            assert_equals_oracle(frames_of(r), ref, f"after the failed call {(w, h, flags)}")
        assert lib.pt_update_env(None, fp, 37, 19, None, 0) == INVALID
        assert lib.pt_update_env_device(None, dp, 37, 19, None, 0) == INVALID
        assert lib.pt_env_size(hnd, None, None) == INVALID
        # download_env: env_compact is 2 here, 0 after the raw map
        assert lib.pt_download_env(hnd, 0, None, None) == INVALID
        assert lib.pt_download_env(hnd, 3, op, None) == INVALID and lib.pt_download_env(hnd, -1, op, None) == INVALID
        assert lib.pt_download_env(hnd, 2, op, None) == INVALID  # the row form holds no texels
        assert lib.pt_download_env(hnd, 1, op, None) == 0 and env_maps.same_bits_or_nan(out[..., :3], hdr)
        r.update_env(tensor(raw))
        assert r.stats().env_compact == 0
        assert rc_of(r.download_env, 1) == INVALID and rc_of(r.download_env, 2) == INVALID
        r.update_env(d, tensor(callers_table(hdr)))
        assert r.stats().env_compact == 1
        r.download_env(1)
        assert rc_of(r.download_env, 2) == INVALID
        r.update_env(d)
        assert_equals_oracle(frames_of(r), ref, "after the failed calls")
    with Renderer(64, 64, "basic") as r:
        assert rc_of(r.update_env, hdr) == INVALID and rc_of(r.update_env, d) == INVALID and rc_of(r.update_env, None) == INVALID


# ------------------------------------------------------------------ 10. uploads and updates in turn: one owner of the buffers
@pytest.fixture(scope="module")
def fresh_exact():
    """An RGBE-exact 37 x 19 map and download_env forms 0, 1 and 2 of a fresh context's upload_env of it."""
    hdr = env_maps.random_map(37, 19, 21)
    with Renderer(8, 8) as r:
        r.upload_env(hdr)
        assert r.stats().env_compact == 2
        return hdr, [r.download_env(form) for form in range(3)]


def assert_state(r, want, what):
    assert r.env_size() == (37, 19) and r.stats().env_compact == 2, what
    for form in (0, 1):
        same_env(r.download_env(form), want[form], f"{what}: form {form}")
    none, table = r.download_env(2)
    assert none is None and env_maps.same_bits_or_nan(table, want[2][1]), f"{what}: row form"


def test_update_after_an_upload_of_the_same_size(fresh_exact):
    """An upload's store holds only the forms that serve its map: the update that follows gets a complete
    store though the size is the same, and the update after that one allocates nothing."""
    import torch
    hdr, want = fresh_exact
    d, other = tensor(hdr), tensor(env_maps.random_map(37, 19, 22))
    with Renderer(8, 8) as r:
        r.upload_env(eu.unquantised_map(37, 19, 43))
        assert r.env_size() == (37, 19) and r.stats().env_compact == 0
        r.update_env(d)
        assert_state(r, want, "upload, update")
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        r.update_env(other)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free  # nothing allocated, nothing freed
        assert r.stats().env_compact == 2


def test_upload_between_updates_of_the_same_size(fresh_exact):
    hdr, want = fresh_exact
    d = tensor(hdr)
    with Renderer(8, 8) as r:
        r.update_env(d)
        assert r.stats().env_compact == 2
        r.upload_env(eu.unquantised_map(37, 19, 43))
        assert r.env_size() == (37, 19) and r.stats().env_compact == 0
        r.update_env(d)
        assert_state(r, want, "update, upload, update")


def test_a_rejected_upload_leaves_no_environment():
    """pt_upload_env releases the old environment before it looks at the new one's size."""
    hdr = env_maps.random_map(37, 19, 21)
    fp = hdr.ctypes.data_as(C.POINTER(C.c_float))
    with renderer("lambert", 2, 8, 8) as r, renderer("lambert", 2, 8, 8) as never:
        r.upload_env(hdr)
        assert r.env_size() == (37, 19)
        assert r._lib.pt_upload_env(r._h, fp, 0, 19, None) == INVALID
        assert r.env_size() == (0, 0) and r.stats().env_compact == 0
        assert np.array_equal(bits(frames_of(r)), bits(frames_of(never)))
