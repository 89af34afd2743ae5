"""The environment-map path at its edges: the shared transcendentals on structured inputs, the sky
texel decision (pt_device.h sphTexel) at directions aimed at texel edges, poles and the seam, the
texel a frame reads, calculateHdrCache on degenerate maps and every form pt_upload_env stores
(float texels, compact texels + 16-bit table + Env::trig / Env::light, and the table by rows).

The maps come from seeds (tests/env_maps.py), the inputs from tests/fmath_sets.py and
tests/sph_texel_ref.py; every image is compared with the oracle bit for bit (tests/parity.py).

Reference: IS pass1.fsh:175-189 (SampleSphericalMap, sampleHdr), :573-585 (SampleHdr), :638-666
(toSphericalCoord, hdrColor, hdrPdf); IS main.cpp:555-652 (calculateHdrCache).
"""
import numpy as np
import pytest

import env_maps
import fmath_sets as fs
import oracle
import parity
import sph_texel_ref as sph
from opengl_ray_tracing_amd import FLAG_MEGAKERNEL, Renderer, calculate_hdr_cache, orbit_camera, scenes
from test_gpu_live_tiles import behind_camera

pytestmark = pytest.mark.gpu
host = fs.host


@pytest.fixture(scope="module")
def ctx():
    with Renderer(8, 8) as r:
        yield r


# ---- a. device equals host
@pytest.mark.parametrize("fn", range(11), ids=lambda f: fs.NAMES[f])
def test_fmath_device_equals_host_on_structured_sets(ctx, fn):
    """Every pt_fmath.h function, the approximations and ptm_sincosf included, gives the host's bits
    on the structured sets and on the zero, infinite and NaN arguments (a NaN equal to any NaN)."""
    args = fs.with_specials(fn)
    d = ctx.fmath_device(fn, *args)
    h = host(fn, *args)
    bad = np.nonzero(~fs.same_bits_or_nan(d, h))[0]
    assert bad.size == 0, (fs.NAMES[fn], bad.size, [a[bad[:3]] for a in args], d[bad[:3]], h[bad[:3]])


# ---- b. the texel decision
@pytest.mark.parametrize("W,H", sph.SIZES, ids=lambda v: str(v))
def test_sph_texel_at_edges_poles_and_seam(ctx, W, H):
    """sphTexel and sphTexelExact, as the frame kernels inline and call them, give the reference's
    texel -- toSpherical + texIndex in float32 numpy with atan2 / asin from float64 -- for 2e5
    directions aimed within 1e-9 .. 1e-5 of texel edges and for the poles, the seam, zero components
    of both signs, vectors off unit length and |y| > 1. The split between the approximations and the
    fallback is restated from pt_fmath_host (the device gives the same bits, test a): both branches
    take their share of the aimed directions, and the approximate coordinate stays closer to the
    exact one than the fallback zone is wide (sph_texel_ref.check_restated_decision; 1 x 1 is
    exempt from the fast share by name there)."""
    dirs, r, ref = sph.check_restated_decision(W, H, host, sph.kernel_margin())
    for fn, a in ((7, (dirs[:, 2], dirs[:, 0])), (8, (dirs[:, 1],))):  # test a's claim on these very inputs
        a = [np.ascontiguousarray(v) for v in a]
        assert fs.same_bits_or_nan(ctx.fmath_device(fn, *a), host(fn, *a)).all()
    t, te = ctx.sph_texel(W, H, dirs)
    bad = np.nonzero((t != ref) | (te != ref))[0]
    assert bad.size == 0, (bad.size, dirs[bad[:4]], t[bad[:4]], te[bad[:4]], ref[bad[:4]], r["fast"][bad[:4]])


# ---- c. which texel a frame reads
TEX_W, TEX_H = 1024, 512


def index_map():
    """1024 x 512, RGBE-exact with one exponent: texel k = y * 1024 + x is (128 + (k >> 16), (k >> 8)
    & 255, k & 255) / 32 -- every texel its own colour, every channel below 8."""
    k = np.arange(TEX_W * TEX_H, dtype=np.int64).reshape(TEX_H, TEX_W)
    img = np.stack([128 + (k >> 16), (k >> 8) & 255, k & 255], -1).astype(np.float32) / np.float32(32.0)
    assert np.array_equal(env_maps.rgbe_quantise(img), img) and img.max() <= 10.0
    return img


def decode_index(rgb, weight=1):
    """The texel index a colour of index_map() encodes; `weight`: the colour is a sample times
    1 / weight (a frame's running-mean update of a cleared image)."""
    m = np.rint(np.asarray(rgb, np.float64)[..., :3] * (32.0 * weight)).astype(np.int64)
    return ((m[..., 0] - 128) << 16) | (m[..., 1] << 8) | m[..., 2]


def sky_frames(hdr, w, h, eye, rot, frames, mode, tris, nodes):
    """-> (running mean after `frames` Lambert frames, the image after frame 0 (mode "call") or None, env_compact)"""
    with Renderer(w, h, "lambert", flags=FLAG_MEGAKERNEL if mode == "megakernel" else 0) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        first = None
        if mode == "call":
            first = r.render_frame(eye, rot, 0, download=True)
            for f in range(1, frames):
                r.render_frame(eye, rot, f)
        else:
            r.render_frames(eye, rot, 0, frames)
        r.synchronize()
        return r.accum().copy(), first, r.stats().env_compact


def test_the_texel_a_frame_reads():
    """A sky-only Lambert frame of a map finer than a pixel whose colours are the texel indices: the
    default kernels of a batch, the megakernel and display() calls give the oracle's image and one
    another's, and frame 0 reads the oracle's texel at every pixel. With one texel moved by an ulp the
    float texels serve (env_compact 0): frame 0 changes at exactly the pixels that read that texel,
    and the mean of four frames only where one of them did."""
    w, h, frames = 192, 128, 4
    eye, rot = orbit_camera(20.0, 10.0, 4.0)
    tris, nodes = behind_camera(eye, rot, w, h)
    hdr = index_map()

    def oracle_mean(img):
        o = oracle.Oracle(tris, nodes, img)
        acc = np.zeros((h, w, 4), np.float32)
        for f in range(frames):
            acc, _ = o.render(w, h, "lambert", f, eye, rot, accum=acc)
        return acc

    o = oracle.Oracle(tris, nodes, hdr)
    texels = [decode_index(o.render(w, h, "lambert", f, eye, rot)[0], f + 1) for f in range(frames)]
    ref = oracle_mean(hdr)
    imgs = {}
    for mode in ("stream", "megakernel", "call"):
        g, first, compact = sky_frames(hdr, w, h, eye, rot, frames, mode, tris, nodes)
        assert compact == 2, (mode, compact)
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), f"texel index map/{mode}")
        imgs[mode] = g
        if mode == "call":
            first0 = first
    assert np.array_equal(imgs["stream"], imgs["megakernel"]) and np.array_equal(imgs["stream"], imgs["call"])
    assert np.array_equal(index_map().reshape(-1, 3)[texels[0]], first0[..., :3])  # (the decoding is exact)
    assert (texels[0][:, 1:] != texels[0][:, :-1]).mean() > 0.5  # the map is finer than a pixel
    # one texel (the one the centre pixel reads in frame 0) one ulp up: no longer an RGBE value
    k = int(texels[0][h // 2, w // 2])
    moved = hdr.copy()
    moved[k // TEX_W, k % TEX_W, 0] = np.nextafter(moved[k // TEX_W, k % TEX_W, 0], np.float32(np.inf))
    ref_moved = oracle_mean(moved)
    touched = np.any([t == k for t in texels], axis=0)
    assert touched[h // 2, w // 2]
    for mode in ("stream", "call"):
        g, first, compact = sky_frames(moved, w, h, eye, rot, frames, mode, tris, nodes)
        assert compact == 0, (mode, compact)
        parity.assert_parity(g.reshape(-1, 4), ref_moved.reshape(-1, 4), f"texel index map, float texels/{mode}")
        assert np.array_equal(g[~touched], imgs[mode][~touched])
        if mode == "call":
            assert np.array_equal(np.any(first != first0, axis=-1), texels[0] == k)


# ---- d. calculateHdrCache on the GPU
@pytest.mark.parametrize("name", env_maps.CACHE_MAP_NAMES)
def test_hdr_cache_device_on_degenerate_maps(ctx, name):
    """pt_hdr_cache_device equals the host's table bit for bit, NaN as NaN: one texel; exactly one
    chunk of the serial luminance sum (64 x 64), a chunk and a 64-value tail (64 x 65), a chunk and
    one value (241 x 17, 4097 x 1: a tail that is no multiple of 4); black rows, black columns (NaN
    conditional CDFs) and an all-black map (every pdf NaN)."""
    hdr = env_maps.cache_maps()[name]
    assert env_maps.same_bits_or_nan(ctx.hdr_cache_device(hdr), calculate_hdr_cache(hdr))


# ---- e. the upload forms
@pytest.fixture(scope="module")
def c2_mesh():
    cfg, tris, nodes, _ = scenes.build_config("c2")
    eye, rot = orbit_camera(*cfg.camera)
    return tris, nodes, eye, rot


def oracle_frames(tris, nodes, hdr, cache, w, h, integrator, mb, eye, rot, frames):
    o = oracle.Oracle(tris, nodes, hdr, cache=cache)
    acc = np.zeros((h, w, 4), np.float32)
    for f in range(frames):
        acc, _ = o.render(w, h, integrator, f, eye, rot, accum=acc, max_bounce=mb)
    return acc


def assert_equals_oracle(g, ref, what):
    """parity.assert_parity (bit for bit) -- or, where the oracle's own image is not finite (MIS divides
    by the pdf of a black texel, as the shader does), equal bit for bit with NaN equal to NaN."""
    if np.isfinite(ref).all():
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), what)
    else:
        assert np.array_equal(g, ref, equal_nan=True), (what, float(np.mean(np.isfinite(g) != np.isfinite(ref))))


def gpu_frames(tris, nodes, hdr, cache, w, h, integrator, mb, eye, rot, frames, mode, flags=0):
    """mode "stream": one render_frames call; "call": display() calls. -> (running mean, env_compact)"""
    with Renderer(w, h, integrator, max_bounce=mb, flags=flags) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr, cache)
        if mode == "call":
            for f in range(frames):
                r.render_frame(eye, rot, f)
        else:
            r.render_frames(eye, rot, 0, frames)
        r.synchronize()
        return r.accum().copy(), r.stats().env_compact


FORM_MAPS = {
    "random 37x19": lambda: env_maps.random_map(37, 19, 21),
    "random 100x50": lambda: env_maps.random_map(100, 50, 22),
    "constant 37x19": lambda: env_maps.constant_map(37, 19),
    "hot texel 37x19": lambda: env_maps.hot_texel_map(37, 19),
    "black rows 40x20": lambda: env_maps.black_rows_map(40, 20, 23),
    "black columns 40x20": lambda: env_maps.black_columns_map(40, 20, 24),
}
INTEGRATORS = [("lambert", 2), ("mis", 2), ("mis", 4)]
W, H, FRAMES = 64, 40, 2


@pytest.mark.parametrize("integrator,mb", INTEGRATORS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(FORM_MAPS))
def test_library_table_is_kept_compact_by_rows(c2_mesh, name, integrator, mb):
    """RGBE maps whose size is no power of two, with constant areas, one lit texel, black rows and
    black columns: the library's own table is stored compact and by rows (env_compact 2), and a
    batch of frames and display() calls give the oracle's image for the same map (with black texels
    MIS's image has NaN pixels, in both)."""
    tris, nodes, eye, rot = c2_mesh
    hdr = FORM_MAPS[name]()
    ref = oracle_frames(tris, nodes, hdr, None, W, H, integrator, mb, eye, rot, FRAMES)
    for mode in ("stream", "call"):
        g, compact = gpu_frames(tris, nodes, hdr, None, W, H, integrator, mb, eye, rot, FRAMES, mode)
        assert compact == 2, (name, mode, compact)
        assert_equals_oracle(g, ref, f"{name}/{integrator}{mb}/{mode}")


def callers_table(hdr):
    """The library's table with its pdf column unchanged and its (x, y) pairs shuffled among the
    texels -- so a row no longer holds one x and the table cannot be stored by rows -- and four
    entries at the corners (0, 0), (1, 0), (0, 1), (1, 1): the integers 0 and w, h, whose sines and
    cosines are the last entries of Env::trig and whose light samples the last row and column of
    Env::light."""
    t = calculate_hdr_cache(hdr).copy()
    h, w = hdr.shape[:2]
    xy = t[..., :2].reshape(-1, 2)
    xy[:] = xy[np.random.default_rng(5).permutation(w * h)]
    xy[[3, w + 7, 5 * w + 11, w * h - 2]] = np.float32([[0, 0], [1, 0], [0, 1], [1, 1]])
    return t


@pytest.mark.parametrize("mb", [2, 4])
def test_callers_table_is_kept_compact_but_not_by_rows(c2_mesh, mb):
    tris, nodes, eye, rot = c2_mesh
    hdr = FORM_MAPS["random 37x19"]()
    table = callers_table(hdr)
    ref = oracle_frames(tris, nodes, hdr, table, W, H, "mis", mb, eye, rot, FRAMES)
    assert not np.array_equal(ref, oracle_frames(tris, nodes, hdr, None, W, H, "mis", mb, eye, rot, FRAMES))
    for mode in ("stream", "call"):
        g, compact = gpu_frames(tris, nodes, hdr, table, W, H, "mis", mb, eye, rot, FRAMES, mode)
        assert compact == 1, (mode, compact)
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), f"caller's table/mis{mb}/{mode}")


@pytest.mark.parametrize("mb", [2, 4])
def test_table_entry_that_is_no_integer_keeps_the_float_table(c2_mesh, mb):
    """The same map and table with one entry 0.3f, which is no x / 37: the float texels and the float
    table serve (env_compact 0)."""
    tris, nodes, eye, rot = c2_mesh
    hdr = FORM_MAPS["random 37x19"]()
    table = callers_table(hdr)
    table[9, 20, 0] = np.float32(0.3)
    ref = oracle_frames(tris, nodes, hdr, table, W, H, "mis", mb, eye, rot, FRAMES)
    for mode in ("stream", "call"):
        g, compact = gpu_frames(tris, nodes, hdr, table, W, H, "mis", mb, eye, rot, FRAMES, mode)
        assert compact == 0, (mode, compact)
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), f"float table/mis{mb}/{mode}")


def test_table_entry_above_one_keeps_the_float_table(c2_mesh):
    """Entries 2.0 = 74 / 37 and 3.0 = 57 / 19 are integers over the map's size but lie past the last
    angle of Env::trig and the last entry of Env::light: such a table is not stored compact
    (pt_envcache.hip envCompactKernel), and the float table gives the oracle's image."""
    tris, nodes, eye, rot = c2_mesh
    hdr = FORM_MAPS["random 37x19"]()
    table = callers_table(hdr)
    table[9, 20, 0] = np.float32(2.0)
    table[4, 30, 1] = np.float32(3.0)
    ref = oracle_frames(tris, nodes, hdr, table, W, H, "mis", 2, eye, rot, FRAMES)
    for mode in ("stream", "call"):
        g, compact = gpu_frames(tris, nodes, hdr, table, W, H, "mis", 2, eye, rot, FRAMES, mode)
        assert compact == 0, (mode, compact)
        parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), f"table entries above 1/{mode}")


def banded_map(w=1500, h=700, seed=31):
    """RGBE, mostly constant: a dim ground, a few bright columns' worth of blocks and a noisy band.
    The bright blocks take most of the marginal, so many rows of the table share their x and the
    rows of one x share one row of y's (Env::cacheRow's ids are reused)."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 2.0 ** -6, np.float32)
    for x0, x1, y0, y1, c in [(100, 130, 50, 300, 8.0), (701, 703, 0, 700, 30.0), (1200, 1400, 600, 650, 2.0)]:
        img[y0:y1, x0:x1] = c
    img[320:340] = np.exp2(rng.uniform(-6, 2, (20, w, 3)))
    return env_maps.rgbe_quantise(img)


def test_table_by_rows_is_read_at_a_width_that_is_no_power_of_two(c2_mesh):
    """1500 x 700 x 4 bytes is above the 4 MB at which the megakernel reads the table by rows
    (Env::cacheRow / cacheY): MIS at 4 bounces gives the oracle's image."""
    tris, nodes, eye, rot = c2_mesh
    hdr = banded_map()
    w, h = 48, 32
    assert hdr.shape[0] * hdr.shape[1] * 4 > 4 << 20
    x = np.rint(calculate_hdr_cache(hdr)[:, 0, 0] * hdr.shape[1]).astype(int)
    assert len(np.unique(x)) < hdr.shape[0] // 2  # rows share their x: ids are reused
    ref = oracle_frames(tris, nodes, hdr, None, w, h, "mis", 4, eye, rot, FRAMES)
    g, compact = gpu_frames(tris, nodes, hdr, None, w, h, "mis", 4, eye, rot, FRAMES, "stream", flags=FLAG_MEGAKERNEL)
    assert compact == 2
    parity.assert_parity(g.reshape(-1, 4), ref.reshape(-1, 4), "table by rows 1500x700")


@pytest.mark.parametrize("integrator,mb", INTEGRATORS, ids=lambda v: str(v))
def test_all_black_map(c2_mesh, integrator, mb):
    """No light at all: every pdf of the table is a NaN, and MIS divides by it as the shader would;
    the image equals the oracle's, NaN pixels included."""
    tris, nodes, eye, rot = c2_mesh
    hdr = env_maps.black_map(8, 4)
    ref = oracle_frames(tris, nodes, hdr, None, W, H, integrator, mb, eye, rot, FRAMES)
    for mode in ("stream", "call"):
        g, _ = gpu_frames(tris, nodes, hdr, None, W, H, integrator, mb, eye, rot, FRAMES, mode)
        assert np.array_equal(g, ref, equal_nan=True), (integrator, mb, mode)
