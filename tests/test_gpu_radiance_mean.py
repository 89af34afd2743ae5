"""Many samples per radiance call, folded on the GPU (pt_radiance_mean_device, pt_radiance_mean;
csrc/pt_radiance_mean.hip) against its contract: sample j of ray k is pt_radiance_device's for sample index
firstSample + j, and the fold is the frames' running-mean update, so per-sample camera rays give the
accumulation of pt_render_frames_async and a PT_FLAG_MOMENTS context's plane, bit for bit. References: the
oracle's frames one sample at a time folded by tests/radiance_mean_ref.py, the frame kernels themselves, and
pt_radiance_device (pinned to the oracle by tests/test_gpu_radiance.py, whose cases and helpers are used
here). 33 x 31 = 1023 rays on a 64 x 64 context, 5 samples. Every comparison is on bits.

References are computed once (functools caches) and shared: do not write to them."""
import ctypes as C
import functools

import numpy as np
import pytest

import env_maps
import material_looks as ml
import oracle
import radiance_mean_ref as mr
import radiance_ref as rf
import refit_ref as rr
import test_gpu_radiance as tg
from opengl_ray_tracing_amd import FLAG_NO_CULL, FLAG_REFERENCE_TREE, Renderer, _native
from post_common import INVALID, NOSCENE, bits
from test_gpu_radiance import CASES, CH, CW, IDS, N, PREFIXES, context, dev, frame_case, host, scene

pytestmark = pytest.mark.gpu

F = np.float32
NS = 5
STARTS = (0, 7)
PER_SAMPLE = 0x1


@functools.lru_cache(maxsize=None)
def sample_stack(case, s0, ns=NS, cam=0):
    """The camera rays of samples s0 .. s0 + ns - 1 of a case and the oracle's samples along them
    -> (rays (ns, N, 6), samples (ns, N, 3), t of the last sample's rays (N,))"""
    parts = [frame_case(case, s, cam) for s in range(s0, s0 + ns)]
    rays = np.stack([p[0] for p in parts])
    samples = np.stack([p[1][:, 0:3] for p in parts])
    t = parts[-1][1][:, 3].copy()
    for a in (rays, samples, t):
        a.setflags(write=False)
    return rays, samples, t


@functools.lru_cache(maxsize=None)
def folded(case, s0):
    """-> (start (mean (N, 3), moments (N, 2)) or None: the reference fold of samples 0 .. s0 - 1,
    want (mean, moments): the fold after samples s0 .. s0 + NS - 1)"""
    start = mr.fold(sample_stack(case, 0, s0)[1], 0) if s0 else None
    want = mr.fold(sample_stack(case, s0)[1], s0, *(start or ()))
    return start, want


def buffers(n, start=None, fill=np.nan):
    """Device mean (n, 4) and moments (n, 2): the start of a continued picture, or `fill` everywhere"""
    mean = np.full((n, 4), fill, F)
    mom = np.full((n, 2), fill, F)
    if start is not None:
        mean[:, 0:3], mean[:, 3] = start[0], F(-1)
        mom[:] = start[1]
    return dev(mean), dev(mom)


def same(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rays differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def check(mean, moments, want, t, what):
    mean = host(mean) if hasattr(mean, "is_cuda") else mean
    same(mean[:, 0:3], want[0], f"{what}: mean")
    same(mean[:, 3], t, f"{what}: t")
    if moments is not None:
        same(host(moments) if hasattr(moments, "is_cuda") else moments, want[1], f"{what}: moments")


# ------------------------------------------------------------------ 1. per-sample rays: the frames' accumulation
def frames_of(case, flags, moments):
    name, integ, mb = CASES[case]
    tris, nodes, hdr, cache, eye, rot = scene(name)
    with Renderer(CW, CH, integ, max_bounce=mb, flags=flags, moments=moments) as r:
        r.upload_scene(tris, nodes)
        if hdr is not None:
            r.upload_env(hdr, cache)
        r.render_frames(eye, rot, 0, NS)
        r.synchronize()
        return r.accum().reshape(-1, 4), (r.moments().reshape(-1, 2) if moments else None)


PER_SAMPLE_CASES = [(c, 0) for c in CASES] + [("c2-lambert", FLAG_REFERENCE_TREE), ("c2-lambert", FLAG_NO_CULL)]


@pytest.mark.parametrize("case,flags", PER_SAMPLE_CASES,
                         ids=[c if not f else f"{c}-flags{f:#x}" for c, f in PER_SAMPLE_CASES])
def test_per_sample_rays(case, flags):
    with context(case, flags=flags) as r:
        for s0 in STARTS:
            rays, _, t = sample_stack(case, s0)
            start, want = folded(case, s0)
            mean, mom = buffers(N, start)
            got = r.radiance_mean_device(dev(rays), dev(IDS), s0, NS, per_sample_rays=True, mean=mean, moments=mom)
            assert got[0] is mean and got[1] is mom
            r.synchronize()
            check(mean, mom, want, t, f"{case} flags {flags:#x} samples {s0}..{s0 + NS - 1}")
        first = host(r.radiance_mean_device(dev(sample_stack(case, 0)[0]), dev(IDS), 0, NS, per_sample_rays=True,
                                            moments=True)[0])
    # ... and so the frame kernels' own accumulation, and a PT_FLAG_MOMENTS context's plane
    want = folded(case, 0)[1]
    acc, _ = frames_of(case, flags, False)
    same(acc[:, 0:3], want[0], f"{case}: render_frames(0, {NS})")
    same(first[:, 0:3], acc[:, 0:3], f"{case}: against render_frames")
    acc_m, plane = frames_of(case, flags, True)
    same(plane, want[1], f"{case}: a moments context's plane")
    same(acc_m[:, 0:3], want[0], f"{case}: a moments context's accumulation")


# ------------------------------------------------------------------ 2. fixed rays
@pytest.mark.parametrize("case", ["c2-lambert", "c3-disney5", "c3-mis2", "c4-mis8", "c2-noenv"])
def test_fixed_rays(case):
    rays, first = frame_case(case, 0)
    rng = np.random.RandomState(77)
    start = (rng.rand(N, 3).astype(F) * F(3), rng.rand(N, 2).astype(F) * F(2))
    with context(case) as r:
        d_rays, d_ids = dev(rays), dev(IDS)
        for s0 in STARTS:
            singles = np.stack([host(r.radiance_device(d_rays, d_ids, s0 + j)) for j in range(NS)])
            assert all(np.array_equal(bits(singles[j, :, 3]), bits(first[:, 3])) for j in range(NS))
            assert case == "c2-noenv" or not np.array_equal(bits(singles[0]), bits(singles[1]))  # the samples differ
            want = mr.fold(singles[:, :, 0:3], s0, *(start if s0 else ()))
            mean, mom = buffers(N, start if s0 else None)
            r.radiance_mean_device(d_rays, d_ids, s0, NS, mean=mean, moments=mom)
            r.synchronize()
            check(mean, mom, want, first[:, 3], f"{case} fixed rays, samples {s0}..{s0 + NS - 1}")
        # one sample: the oracle's sample of the rays' own frame, folded once
        for s in STARTS:
            rays_s, want_s = frame_case(case, s)
            mean, mom = buffers(N, start if s else None)
            r.radiance_mean_device(dev(rays_s), d_ids, s, 1, mean=mean, moments=mom)
            r.synchronize()
            check(mean, mom, mr.fold(want_s[None, :, 0:3], s, *(start if s else ())), want_s[:, 3],
                  f"{case} one sample {s}")


# ------------------------------------------------------------------ 3. continuation
@pytest.mark.parametrize("per_sample", [True, False], ids=["per_sample", "fixed"])
def test_continuation(per_sample):
    import torch
    case = "c2-lambert"
    stack = sample_stack(case, 0)[0]
    with context(case) as r:
        d_ids = dev(IDS)
        rays = dev(stack) if per_sample else dev(stack[0])
        part = (lambda a, b: rays[a:b].contiguous()) if per_sample else (lambda a, b: rays)
        torch.cuda.synchronize()
        for with_moments in (True, False):
            # firstSample 0 does not read the buffers: NaN in them does not matter
            whole, whole_m = buffers(N)
            r.radiance_mean_device(rays, d_ids, 0, NS, per_sample, whole, whole_m if with_moments else None)
            mean, mom = buffers(N)
            r.radiance_mean_device(part(0, 3), d_ids, 0, 3, per_sample, mean, mom if with_moments else None)
            r.radiance_mean_device(part(3, 5), d_ids, 3, 2, per_sample, mean, mom if with_moments else None)
            r.synchronize()
            w, m = host(whole), host(mean)
            assert not np.isnan(w).any()
            assert np.array_equal(bits(w), bits(m)), "3 + 2 samples against 5"
            if per_sample:
                same(w[:, 0:3], folded(case, 0)[1][0], "whole")
            if with_moments:
                assert np.array_equal(bits(host(whole_m)), bits(host(mom)))
                assert not np.isnan(host(mom)).any()
            else:  # no moments asked: the tensors keep their fill
                assert np.isnan(host(whole_m)).all() and np.isnan(host(mom)).all()
        # moments None: what lies behind the mean in the same allocation stays as it was
        both = torch.full((N * 6,), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.radiance_mean_device(rays, d_ids, 0, NS, per_sample, both[:N * 4].view(N, 4), None)
        r.synchronize()
        assert np.array_equal(bits(host(both[:N * 4]).reshape(N, 4)), bits(w))
        assert bool((both[N * 4:] == -7.0).all())


# ------------------------------------------------------------------ 4. shapes
@functools.lru_cache(maxsize=None)
def shuffled_stack():
    """Three cameras' per-sample rays of samples 0 .. 4 concatenated and shuffled
    -> (rays (NS, 3N, 6), ids (3N, 2), want (mean, moments), t of the last sample's rays)"""
    cams = [sample_stack("c2-lambert", 0, NS, cam) for cam in range(len(tg.cameras()))]
    perm = np.random.RandomState(4321).permutation(3 * N)
    rays = np.ascontiguousarray(np.concatenate([c[0] for c in cams], axis=1)[:, perm])
    samples = np.concatenate([c[1] for c in cams], axis=1)[:, perm]
    t = np.concatenate([c[2] for c in cams])[perm]
    ids = np.ascontiguousarray(np.concatenate([IDS] * 3)[perm])
    return rays, ids, mr.fold(samples, 0), t


def test_order_and_prefixes():
    rays, ids, want, t = shuffled_stack()
    with context("c2-lambert") as r:
        d_rays, d_ids = dev(rays), dev(ids)
        mean, mom = r.radiance_mean_device(d_rays, d_ids, 0, NS, per_sample_rays=True, moments=True)
        r.synchronize()
        check(mean, mom, want, t, "three cameras shuffled")
        for n in PREFIXES:
            cut = d_rays[:, :n].contiguous()
            import torch
            torch.cuda.synchronize()
            mean, mom = r.radiance_mean_device(cut, d_ids[:n], 0, NS, per_sample_rays=True, moments=True)
            r.synchronize()
            check(mean, mom, (want[0][:n], want[1][:n]), t[:n], f"prefix {n}")


def test_default_ids():
    """ids None is (k & 4095, k >> 12), over more than one row of ids"""
    rays3 = shuffled_stack()[0][0]
    rays = np.ascontiguousarray(np.concatenate([rays3, rays3])[:4096 + 65])
    ids = rf.default_ids(len(rays))
    assert ids[:, 1].max() == 1
    with context("c2-lambert") as r:
        d_rays = dev(rays)
        a, am = r.radiance_mean_device(d_rays, None, 0, NS, moments=True)
        b, bm = r.radiance_mean_device(d_rays, dev(ids), 0, NS, moments=True)
        h, hm = r.radiance_mean(rays, None, 0, NS, moments=True)
        r.synchronize()
        singles = np.stack([r.radiance(rays, ids, j) for j in range(NS)])
    assert np.array_equal(bits(host(a)), bits(host(b))) and np.array_equal(bits(host(am)), bits(host(bm)))
    assert np.array_equal(bits(host(a)), bits(h)) and np.array_equal(bits(host(am)), bits(hm))
    check(h, hm, mr.fold(singles[:, :, 0:3], 0), singles[0][:, 3], "default ids against radiance_device")


def test_more_rays_than_lanes():
    """More rays than the largest launch has lanes (8 blocks of 256 per compute unit): a lane takes a second ray"""
    import torch
    rays0 = frame_case("c2-lambert", 0)[0]
    n = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 777
    with context("c2-lambert") as r:
        rays = dev(rays0).repeat((n + N - 1) // N, 1)[:n].contiguous()
        torch.cuda.synchronize()
        a = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
        for s in range(2):
            c = r.radiance_device(rays, None, s)
            r.synchronize()
            w = torch.tensor(F(1) / F(s + 1), dtype=torch.float32, device="cuda:0")
            a = a * (1.0 - w) + c[:, 0:3] * w  # mixf, one rounding per operation
        mean, _ = r.radiance_mean_device(rays, None, 0, 2)
        r.synchronize()
        assert torch.equal(mean[:, 0:3].view(torch.int32), a.view(torch.int32))
        assert torch.equal(mean[:, 3].view(torch.int32), c[:, 3].view(torch.int32))
        assert len(torch.unique(mean[-777:, 0])) > 50  # the tail was written with a picture


# ------------------------------------------------------------------ 5. forms and order
def test_host_device_and_torch_stream():
    import torch
    rays, ids, want, t = shuffled_stack()
    n = len(ids)
    with context("c2-lambert") as r:
        h, hm = r.radiance_mean(rays, ids, 0, NS, per_sample_rays=True, moments=True)
        check(h, hm, want, t, "host form")
        # the host form goes on from host arrays
        a, am = r.radiance_mean(rays[:3], ids, 0, 3, per_sample_rays=True, moments=True)
        b, bm = r.radiance_mean(rays[3:], ids, 3, 2, per_sample_rays=True, mean=a, moments=am)
        assert np.array_equal(bits(b), bits(h)) and np.array_equal(bits(bm), bits(hm))
        h1, none = r.radiance_mean(rays, ids, 0, NS, per_sample_rays=True)
        assert none is None and np.array_equal(bits(h1), bits(h))
        # tensors produced and consumed on a torch stream the context was given
        base, base_ids = dev(rays), dev(ids)
        st = torch.cuda.Stream()
        r.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            d_rays = (base * 1.0).contiguous()
            d_ids = base_ids.clone()
            mean, mom = r.radiance_mean_device(d_rays, d_ids, 0, NS, per_sample_rays=True, moments=True)
            hits = (mean[:, 3] < float(rf.MISS_T)).sum()
        st.synchronize()
        assert mean.dtype == torch.float32 and mean.shape == (n, 4) and mom.shape == (n, 2)
        check(mean.cpu().numpy(), mom.cpu().numpy(), want, t, "torch stream")
        assert int(hits) == int((t < rf.MISS_T).sum())
        # raw pointers with n into tensors of the caller's
        mine = torch.full((n, 4), -1.0, dtype=torch.float32, device="cuda:0")
        mine_m = torch.full((n, 2), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.radiance_mean_device(d_rays.data_ptr(), d_ids.data_ptr(), 0, NS, True, mine.data_ptr(), mine_m.data_ptr(), n=n)
        r.synchronize()
        check(mine.cpu().numpy(), mine_m.cpu().numpy(), want, t, "raw pointers")
        for kw in (dict(rays=d_rays.double()), dict(rays=d_rays, ids=d_ids.long()), dict(rays=d_rays, ids=d_ids[:-1]),
                   dict(rays=d_rays, mean=mine[:-1]), dict(rays=d_rays, moments=mine_m[:-1]), dict(rays=d_rays.cpu()),
                   dict(rays=d_rays.data_ptr()), dict(rays=d_rays, n_samples=0), dict(rays=d_rays, first_sample=2**32 - 3),
                   dict(rays=d_rays, first_sample=3), dict(rays=d_rays, first_sample=3, mean=mine, moments=True)):
            kw.setdefault("n_samples", NS)
            with pytest.raises(ValueError):
                r.radiance_mean_device(per_sample_rays=True, **kw)
        r.set_stream(None)


def test_between_frames_in_flight():
    """Frames, a call, more frames, no synchronisation in between: neither disturbs the other."""
    case = "c2-lambert"
    rays, _, t = sample_stack(case, 0)
    want = folded(case, 0)[1]
    _, _, _, _, eye, rot = scene("c2")

    def run(query):
        with context(case, 100, 76) as r:
            d_rays, d_ids = dev(rays), dev(IDS)
            out = None
            r.render_frames(eye, rot, 0, 8)
            if query:
                out = r.radiance_mean_device(d_rays, d_ids, 0, NS, per_sample_rays=True, moments=True)
            r.render_frames(eye, rot, 8, 8)
            acc = r.accum()
            st = r.stats()
            return acc, st, None if out is None else (host(out[0]), host(out[1]))

    acc_q, st_q, out = run(True)
    acc, st, _ = run(False)
    check(out[0], out[1], want, t, "between frames")
    assert np.array_equal(bits(acc_q), bits(acc))
    assert st_q.rays == st.rays and st_q.frames == st.frames == 16  # pt_frame_stats is not touched


def _after(make_a, make_b, update, integ, mb, rays, per_sample=True):
    """A context updated in place against a fresh upload of the same content: the same means and moments."""
    with make_a() as a, make_b() as b:
        before = a.radiance_mean(rays, IDS, 0, NS, per_sample_rays=per_sample, moments=True)
        update(a)
        got = a.radiance_mean(rays, IDS, 0, NS, per_sample_rays=per_sample, moments=True)
        fresh = b.radiance_mean(rays, IDS, 0, NS, per_sample_rays=per_sample, moments=True)
    assert np.array_equal(bits(got[0]), bits(fresh[0])) and np.array_equal(bits(got[1]), bits(fresh[1]))
    assert not np.array_equal(bits(got[0]), bits(before[0]))  # the update changes what the rays see
    return got


@pytest.mark.parametrize("integ,mb", [("lambert", 2), ("mis", 2)])
def test_after_updates(integ, mb):
    sc, k = "material", 1
    tris0, nodes0, hdr, cache, eye, rot, _, _ = rr.scene_arrays(sc)
    tris_k, nodes_k, _ = rr.posed(sc, k)
    rays = np.stack([rf.camera_rays(CW, CH, eye, rot, s) for s in range(NS)])

    def ctx(tris, nodes, env=(hdr, cache)):
        def make():
            r = Renderer(64, 64, integ, max_bounce=mb)
            r.upload_scene(tris, nodes)
            r.upload_env(*env)
            return r
        return make

    # geometry: against a fresh upload, and the oracle's fold
    got = _after(ctx(tris0, nodes0), ctx(tris_k, nodes_k), lambda r: r.update_geometry(rr.pose(tris0, k)), integ, mb, rays)
    orc = oracle.Oracle(tris_k, nodes_k, hdr, cache)
    samples = np.stack([rf.oracle_sample(orc, CW, CH, integ, mb, eye, rot, s).reshape(-1, 4)[:, 0:3] for s in range(NS)])
    want = mr.fold(samples, 0)
    same(got[0][:, 0:3], want[0], "after update_geometry: the oracle's fold")
    same(got[1], want[1], "after update_geometry: the oracle's moments")
    # materials (look 4 moves the emitters: every integrator shades that)
    mats = ml.mats_of(sc, 4)
    _after(ctx(tris0, nodes0), ctx(ml.tris_of(tris0, mats), nodes0), lambda r: r.update_materials(mats), integ, mb, rays)
    # environment (fixed rays: the sky rays fold the new sky's colour)
    env = env_maps.random_map(37, 19, 5)
    _after(ctx(tris0, nodes0), ctx(tris0, nodes0, (env, None)), lambda r: r.update_env(env), integ, mb, rays[0], False)


# ------------------------------------------------------------------ 6. errors
def test_error_paths():
    import torch
    rays = frame_case("c2-lambert", 0)[0]
    tris, nodes, *_ = scene("c2")
    lib = _native.load()
    n = 64
    fp, ip = _native.c_float_p, _native.c_int_p
    h_rays, h_ids = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(IDS[:n])
    h_mean, h_mom = np.full((n, 4), -5.0, F), np.full((n, 2), -5.0, F)
    d_rays, d_ids = dev(h_rays), dev(h_ids)
    d_mean = torch.full((n, 4), -5.0, dtype=torch.float32, device="cuda:0")
    d_mom = torch.full((n, 2), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def calls(r, count, first=0, ns=2, flags=0, with_rays=True, with_mean=True, with_moments=True):
        return [
            lib.pt_radiance_mean(r._h, h_rays.ctypes.data_as(fp) if with_rays else None, h_ids.ctypes.data_as(ip), count,
                                 first, ns, flags, h_mean.ctypes.data_as(fp) if with_mean else None,
                                 h_mom.ctypes.data_as(fp) if with_moments else None),
            lib.pt_radiance_mean_device(r._h, C.c_void_p(d_rays.data_ptr()) if with_rays else None,
                                        C.c_void_p(d_ids.data_ptr()), count, first, ns, flags,
                                        C.c_void_p(d_mean.data_ptr()) if with_mean else None,
                                        C.c_void_p(d_mom.data_ptr()) if with_moments else None),
        ]

    def untouched():
        torch.cuda.synchronize()
        return bool(np.all(h_mean == F(-5.0)) and np.all(h_mom == F(-5.0))) and bool((d_mean == -5.0).all()) and \
            bool((d_mom == -5.0).all())

    with Renderer(16, 16, "lambert") as r:
        assert calls(r, n) == [NOSCENE] * 2  # before pt_upload_scene
        assert calls(r, -1) == [INVALID] * 2
        r.upload_scene(tris, nodes)
        assert calls(r, -1) == [INVALID] * 2
        assert calls(r, n, ns=0) == [INVALID] * 2
        assert calls(r, n, ns=-1) == [INVALID] * 2
        assert calls(r, n, first=2**32 - 2, ns=2) == [INVALID] * 2  # the last weight's s + 1u would wrap
        assert calls(r, n, first=2**32 - 1, ns=1) == [INVALID] * 2
        assert calls(r, n, flags=0x2) == [INVALID] * 2
        assert calls(r, n, flags=0x3) == [INVALID] * 2
        assert calls(r, n, with_rays=False) == [INVALID] * 2
        assert calls(r, n, with_mean=False) == [INVALID] * 2
        assert calls(r, 0) == [0] * 2  # n == 0: PT_OK, nothing read or written
        assert calls(r, 0, with_rays=False, with_mean=False, with_moments=False) == [0] * 2
        assert calls(r, 0, ns=0) == [INVALID] * 2
        r.synchronize()
        assert untouched()
        # the same buffers take results once the call is valid; the last sample index there is: 2^32 - 2
        assert calls(r, n, with_moments=False) == [0] * 2
        r.synchronize()
        assert np.array_equal(bits(h_mean), bits(host(d_mean))) and not np.any(h_mean == F(-5.0))
        assert np.all(h_mom == F(-5.0)) and bool((d_mom == -5.0).all())  # NULL moments: none written
        assert calls(r, n, first=2**32 - 3, ns=2) == [0] * 2
        assert calls(r, n, flags=PER_SAMPLE, ns=1) == [0] * 2
        r.synchronize()
        assert np.array_equal(bits(h_mean), bits(host(d_mean))) and np.array_equal(bits(h_mom), bits(host(d_mom)))
        with pytest.raises(ValueError):
            r.radiance_mean(rays[:4], IDS[:3])
        with pytest.raises(ValueError):
            r.radiance_mean(rays[:5], None, 0, 2, per_sample_rays=True)
        with pytest.raises(ValueError):
            r.radiance_mean(rays[:4], None, 3, 2)
    with Renderer(16, 16, "basic") as r:  # the BASIC integrator has no scene of triangles
        assert calls(r, n) == [NOSCENE] * 2
