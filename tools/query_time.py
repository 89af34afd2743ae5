#!/usr/bin/env python3
"""Throughput of the ray queries on the GPU, in Mrays/s.

    python tools/query_time.py [--camera c2 c5] [--ao c4] [--rounds 5] [--reps 20] [--out out/queries.json]

Every comparison alternates its sides round by round in one process and keeps each round's figure; a
side "wins" only when its slowest round beats the other side's fastest.
 * camera rays (each config at its own size, one ray per pixel centre), closest hit:
     host         pt_trace_closest: wall time of the call (copies in and out, the pipeline drained);
                  pt_trace_closest_range with no bound is the same path without the drain, and its
                  results are asserted equal
     device_wall  pt_trace_closest_device + a stream synchronise, host clock
     device       pt_trace_closest_device, device events around `reps` calls back to back
   (Until round 16 pt_trace_closest had a kernel and staging of its own, and this script put it beside
   the ranged call as old_host / new_host: profiles/r14/queries.json, profiles/r16/queries_parent.json.)
 * AO rays (tools/ao.py: `--ao-rays` cosine-weighted directions from every hit pixel of the config at
   `--ao-size`, tmax = `--radius`): occluded against ranged closest against unbounded closest, device events.
 * the plain loop against a loop that refills a wave's finished lanes: measured once with the refill
   loop as a build option (profiles/r14/queries.json holds those rounds, profiles/r14/refill_loop.patch
   the loop and this script's comparison); it lost everywhere and is not in the library.
One JSON line per config and kind.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def spread(xs):
    return {"min": min(xs), "max": max(xs), "rounds": [round(x, 2) for x in xs]}


def beats(a, b) -> bool:
    """rates: a's slowest round beats b's fastest"""
    return min(a) > max(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--camera", nargs="*", default=["c2", "c5"])
    ap.add_argument("--ao", nargs="*", default=["c4"])
    ap.add_argument("--ao-size", default="1920x1080")
    ap.add_argument("--ao-rays", type=int, default=8)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import ao
    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    if os.environ.get("PT_VARIANT"):  # an in-tree build variant (a parent commit's library beside this tree's)
        from opengl_ray_tracing_amd import _native
        _native.use_variant(os.environ["PT_VARIANT"])
    if not torch.cuda.is_available():
        raise RuntimeError("query_time: no GPU visible")
    stream = torch.cuda.Stream()
    lines = []

    def context(cfg, tris, nodes, w, h):
        r = Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce)
        r.upload_scene(tris, nodes)
        r.set_stream(stream.cuda_stream)
        return r

    def device_rate(fn, n):
        """Mrays/s of fn() (one query of n rays on `stream`) by device events around `reps` calls"""
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return n * a.reps / (e0.elapsed_time(e1) * 1e-3) / 1e6

    def wall_rate(fn, n, reps):
        """Mrays/s of fn() (synchronous, or ending in a synchronise) by the host clock"""
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return n * reps / (time.perf_counter() - t0) / 1e6

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    for name in a.camera:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        eye, rot = orbit_camera(*cfg.camera)
        w, h = cfg.width, cfg.height
        rays = ao.camera_rays(w, h, eye, rot)
        n = rays.shape[0]
        r = context(cfg, tris, nodes, 64, 64)
        try:
            d_rays = torch.from_numpy(rays).to("cuda")
            d_t = torch.empty(n, dtype=torch.float32, device="cuda")
            d_tri = torch.empty(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            res = {"kind": "camera", "config": name, "rays": n, "rounds": a.rounds, "reps": a.reps,
                   "triangles": int(np.asarray(tris).reshape(-1, 36).shape[0])}
            t_old, tri_old = r.trace_closest(rays)
            res["hit_share"] = float((tri_old >= 0).mean())
            # the unbounded results of every new form equal the old query's
            t_new, tri_new = r.trace_closest_range(rays)
            r.trace_closest_device(d_rays, None, d_t, d_tri)
            r.synchronize()
            assert np.array_equal(d_tri.cpu().numpy(), tri_old) and np.array_equal(d_t.cpu().numpy(), t_old)
            assert np.array_equal(tri_new, tri_old) and np.array_equal(t_new, t_old)

            def device_sync():
                r.trace_closest_device(d_rays, None, d_t, d_tri)
                stream.synchronize()

            rates = {"host": [], "device_wall": [], "device": []}
            host_reps = max(2, a.reps // 4)
            for _ in range(a.rounds):
                rates["host"].append(wall_rate(lambda: r.trace_closest(rays), n, host_reps))
                rates["device_wall"].append(wall_rate(device_sync, n, a.reps))
                rates["device"].append(device_rate(lambda: r.trace_closest_device(d_rays, None, d_t, d_tri), n))
            for key, xs in rates.items():
                res[f"{key}_Mrays"] = spread(xs)
            res["device_wall_beats_host"] = beats(rates["device_wall"], rates["host"])
            emit(res)
        finally:
            r.close()

    aw, ah = (int(x) for x in a.ao_size.lower().split("x"))
    for name in a.ao:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        eye, rot = orbit_camera(*cfg.camera)
        r = context(cfg, tris, nodes, aw, ah)
        try:
            with torch.cuda.stream(stream):
                pos_t = torch.empty((ah, aw, 4), dtype=torch.float32, device="cuda")
                nrm_tri = torch.empty((ah, aw, 4), dtype=torch.float32, device="cuda")
                r.render_guides(eye, rot)
                r.guides_into(pos_t.data_ptr(), nrm_tri.data_ptr())
                idx, rays = ao.ao_rays(pos_t, nrm_tri, a.ao_rays, 1)
                n = int(rays.shape[0])
                tmax = torch.full((n,), a.radius, dtype=torch.float32, device="cuda")
                d_t = torch.empty(n, dtype=torch.float32, device="cuda")
                d_tri = torch.empty(n, dtype=torch.int32, device="cuda")
                d_occ = torch.empty(n, dtype=torch.uint8, device="cuda")
            stream.synchronize()
            res = {"kind": "ao", "config": name, "width": aw, "height": ah, "rays_per_pixel": a.ao_rays,
                   "radius": a.radius, "rays": n, "rounds": a.rounds, "reps": a.reps}
            # occluded is ranged closest's hit flag
            r.trace_occluded_device(rays, tmax, d_occ)
            r.trace_closest_device(rays, tmax, d_t, d_tri)
            r.synchronize()
            occ = d_occ.cpu().numpy()
            assert np.array_equal(occ, (d_tri.cpu().numpy() >= 0).astype(np.uint8))
            res["occluded_share"] = float(occ.mean())
            rates = {"occluded": [], "closest_ranged": [], "closest_unbounded": []}
            for _ in range(a.rounds):
                rates["occluded"].append(device_rate(lambda: r.trace_occluded_device(rays, tmax, d_occ), n))
                rates["closest_ranged"].append(device_rate(lambda: r.trace_closest_device(rays, tmax, d_t, d_tri), n))
                rates["closest_unbounded"].append(device_rate(lambda: r.trace_closest_device(rays, None, d_t, d_tri), n))
            for key, xs in rates.items():
                res[f"{key}_Mrays"] = spread(xs)
            res["occluded_beats_closest_ranged"] = beats(rates["occluded"], rates["closest_ranged"])
            res["closest_ranged_beats_unbounded"] = beats(rates["closest_ranged"], rates["closest_unbounded"])
            emit(res)
        finally:
            r.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
