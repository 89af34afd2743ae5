#!/usr/bin/env python3
"""Paths per second of the radiance query beside the frame kernels on the same rays.

    python tools/radiance_time.py [c2 c3 c4] [--rounds 5] [--reps 20] [--calls 50] [--out out/radiance.json]

Per config, at its own size (1920 x 1080) and camera, every ray one sample of its integrator:
  radiance         pt_radiance_device on the camera rays pt_camera_rays_device wrote (sample 0) with their pixel
                   ids, device events around `reps` calls back to back on the context's stream
  radiance_wall    the same call and a stream synchronise, host clock: what a caller who waits pays per call
  frame_call       one synchronous pt_render_frame of that camera (tools/per_call.py's figure: median of
                   `calls` calls), the yardstick -- it too is one sample per ray with nothing streamed
  frame_streamed   pt_render_frames_async, `reps` frames and one synchronise, host clock per frame
  camera_rays      the device time of pt_camera_rays_device
The sides alternate round by round in one process; every round's figure is kept. Before timing, the radiance
of the camera rays is checked against the frame of the same sample, bit for bit. One JSON line per config.

    python tools/radiance_time.py [c2 c3 c4] --samples 16 [--rounds 5] [--out out/radiance_mean.json]

With --samples S the many-sample call instead (pt_radiance_mean_device, mean and moments), device events
around each side, per config and for both forms of its rays:
  singles_fixed       S pt_radiance_device calls, sample indices 0 .. S-1, on the camera rays of sample 0: the
                      yardstick (what a caller's loop costs on the device before it folds anything)
  mean_fixed          one pt_radiance_mean_device call of S samples on those rays
  singles_per_sample  S pt_radiance_device calls, call j on the camera rays of sample j
  mean_per_sample     one call with PT_RADIANCE_RAYS_PER_SAMPLE on the S x n rays
Before timing, each batched result is checked on bits against the single calls folded in torch with the
frames' expressions (one kernel per operation: nothing is fused).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PROBE_FRAMES = 90  # tools/per_call.py's: the renderer's policy probe after a restart runs before the timed calls


def spread(xs, nd=4):
    return {"min": round(min(xs), nd), "max": round(max(xs), nd), "median": round(statistics.median(xs), nd),
            "rounds": [round(x, nd) for x in xs]}


def mean_config(name, S, rounds, stream):
    """--samples: one config's result line (a dict)"""
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    cfg, tris, nodes, hdr = scenes.build_config(name)
    eye, rot = orbit_camera(*cfg.camera)
    w, h = cfg.width, cfg.height
    n = w * h
    with Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        r.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            per = torch.empty((S, n, 6), dtype=torch.float32, device="cuda:0")
            ids = torch.empty((n, 2), dtype=torch.int32, device="cuda:0")
            for j in range(S):
                r.camera_rays_device(eye, rot, j, per[j], ids)
            fixed = per[0]
            out = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
            mean = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
            mom = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")

            def singles(rays_of):
                for j in range(S):
                    r.radiance_device(rays_of(j), ids, j, out)

            sides = {"singles_fixed": lambda: singles(lambda j: fixed),
                     "mean_fixed": lambda: r.radiance_mean_device(fixed, ids, 0, S, False, mean, mom),
                     "singles_per_sample": lambda: singles(lambda j: per[j]),
                     "mean_per_sample": lambda: r.radiance_mean_device(per, ids, 0, S, True, mean, mom)}
            # the batched results against the folded single calls, on bits
            equal = {}
            for form, rays_of in (("fixed", lambda j: fixed), ("per_sample", lambda j: per[j])):
                a3 = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
                m1 = torch.zeros(n, dtype=torch.float32, device="cuda:0")
                m2 = torch.zeros(n, dtype=torch.float32, device="cuda:0")
                for j in range(S):
                    r.radiance_device(rays_of(j), ids, j, out)
                    wt = torch.tensor(1.0, dtype=torch.float32, device="cuda:0") / float(j + 1)
                    c = out[:, 0:3]
                    a3 = a3 * (1.0 - wt) + c * wt
                    lum = (c[:, 0] * 0.3 + c[:, 1] * 0.6) + c[:, 2] * 0.1
                    m1 = m1 * (1.0 - wt) + lum * wt
                    m2 = m2 * (1.0 - wt) + (lum * lum) * wt
                sides[f"mean_{form}"]()
                want = torch.cat([a3, out[:, 3:4], m1[:, None], m2[:, None]], dim=1)
                got = torch.cat([mean, mom], dim=1)
                equal[form] = bool(((got.view(torch.int32) == want.view(torch.int32)) | (got.isnan() & want.isnan())).all())
            stream.synchronize()
            if not all(equal.values()):
                raise RuntimeError(f"{name}: the batched call is not the folded single calls: {equal}")

            def events(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for fn in sides.values():  # warm
                fn()
            stream.synchronize()
            ms = {k: [] for k in sides}
            for i in range(rounds):
                order = list(sides) if i % 2 == 0 else list(sides)[::-1]
                for k in order:
                    ms[k].append(events(sides[k]))
            hit_share = round(float((mean[:, 3] < 2147483648.0).float().mean()), 4)
        r.set_stream(None)
    res = {"config": name, "width": w, "height": h, "rays": n, "integrator": cfg.integrator, "max_bounce": cfg.max_bounce,
           "samples": S, "rounds": rounds, "hit_share": hit_share, "equals_folded_singles_bits": equal}
    for k, xs in ms.items():
        res[f"{k}_ms"] = spread(xs, 3)
    for form in ("fixed", "per_sample"):
        res[f"speedup_{form}"] = round(statistics.median(ms[f"singles_{form}"]) / statistics.median(ms[f"mean_{form}"]), 3)
        res[f"mean_{form}_ms_per_sample"] = round(statistics.median(ms[f"mean_{form}"]) / S, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--samples", type=int, default=0, help="time the many-sample call of this many samples instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    if os.environ.get("PT_VARIANT"):  # an in-tree tuning build (_build.build_variant, e.g. other PT_RADIANCE_WAVES_*)
        from opengl_ray_tracing_amd import _native
        _native.use_variant(os.environ["PT_VARIANT"])
    if not torch.cuda.is_available():
        raise RuntimeError("radiance_time: no GPU visible")
    stream = torch.cuda.Stream()
    lines = []
    if a.samples > 0:
        for name in a.configs:
            line = json.dumps(mean_config(name, a.samples, a.rounds, stream))
            print(line, flush=True)
            lines.append(line)
        a.configs = []
    for name in a.configs:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        eye, rot = orbit_camera(*cfg.camera)
        w, h = cfg.width, cfg.height
        n = w * h
        with Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce) as r:
            r.upload_scene(tris, nodes)
            r.upload_env(hdr)
            # the frame of sample 0 on a zero accumulation is that sample (weight 1)
            frame0 = r.render_frame(eye, rot, 0, download=True).reshape(-1, 4)
            r.set_stream(stream.cuda_stream)
            with torch.cuda.stream(stream):
                rays, ids = r.camera_rays_device(eye, rot, 0)
                out = r.radiance_device(rays, ids, 0)
            stream.synchronize()
            got = out.cpu().numpy()
            g, f0 = np.ascontiguousarray(got[:, 0:3]), np.ascontiguousarray(frame0[:, 0:3])
            same = bool(((g.view(np.uint32) == f0.view(np.uint32)) | (np.isnan(g) & np.isnan(f0))).all())
            res = {"config": name, "width": w, "height": h, "rays": n, "integrator": cfg.integrator,
                   "max_bounce": cfg.max_bounce, "rounds": a.rounds, "reps": a.reps, "calls": a.calls,
                   "hit_share": round(float((got[:, 3] < 2147483648.0).mean()), 4), "equals_frame_bits": same}
            if not same:
                raise RuntimeError(f"{name}: the radiance of the camera rays is not the frame's sample")

            def events(fn):
                """device ms per call of fn() by events around `reps` calls on `stream`"""
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / a.reps

            def wall(fn, reps):
                """host ms per call of fn() (synchronous, or ending in a synchronise): the median call"""
                fn()
                ms = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    ms.append(1e3 * (time.perf_counter() - t0))
                return statistics.median(ms)

            def radiance_sync():
                r.radiance_device(rays, ids, 0, out)
                stream.synchronize()

            f = [1]

            def frame_call():
                r.render_frame(eye, rot, f[0])
                f[0] += 1

            def frames_streamed():
                t0 = time.perf_counter()
                r.render_frames(eye, rot, f[0], a.reps)
                r.synchronize()
                f[0] += a.reps
                return 1e3 * (time.perf_counter() - t0) / a.reps

            for _ in range(PROBE_FRAMES):
                r.render_frame(eye, rot, f[0], sync=False)
                f[0] += 1
            r.synchronize()
            ms = {"radiance": [], "radiance_wall": [], "frame_call": [], "frame_streamed": [], "camera_rays": []}
            for _ in range(a.rounds):
                ms["radiance"].append(events(lambda: r.radiance_device(rays, ids, 0, out)))
                ms["radiance_wall"].append(wall(radiance_sync, a.reps))
                ms["frame_call"].append(wall(frame_call, a.calls))
                frames_streamed()
                ms["frame_streamed"].append(frames_streamed())
                ms["camera_rays"].append(events(lambda: r.camera_rays_device(eye, rot, 0, rays, ids)))
            st = r.stats()
            r.set_stream(None)
        for key, xs in ms.items():
            res[f"{key}_ms"] = spread(xs)
        res["radiance_mpaths_per_s"] = round(n / (statistics.median(ms["radiance"]) * 1e-3) / 1e6, 1)
        res["radiance_wall_over_frame_call"] = round(statistics.median(ms["radiance_wall"]) /
                                                     statistics.median(ms["frame_call"]), 3)
        res["frame_kernel_streamed"] = "path regeneration" if st.regen else "lock-step megakernel"
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
