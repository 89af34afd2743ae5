#!/usr/bin/env python3
"""What adaptive sampling (PT_FLAG_ADAPTIVE) costs and what it buys on the GPU.

    python tools/adaptive_time.py [c2 c3 c4] [--runs 5] [--frames 200] [--reps 100] [--every 48]
                                  [--max-frames 4096] [--thresholds 0.00392 0.01569] [--out out/adaptive_time.json]

Method: each config at its own size (c2 - c4: 1080p), an adaptive context and a PT_FLAG_MOMENTS context
in one process on one torch stream, HIP events (torch.cuda.Event) around what is timed, profiler off,
both past the runtime's policy probe (32 frames) first.
 * idle: the flag's own cost with nothing retired -- `frames` frames streamed (one render_frames call),
   the two contexts alternating, each first in turn, `runs` runs each: ms per frame of every run. Which
   of two contexts of a process was created first moves its time by more than the flag does (about
   5 %, in either direction, per config), so the pair is measured twice, created in either order, and
   like is compared with like: the ranges of the two contexts that were created first, and of the
   two created second. idle_spread_ms: the range of all four. c2 and c3 run the camera-ray pass either
   way; c4's megakernel takes it only with the flag.
 * update: pt_adaptive_update, `reps` repetitions between two events, with every tile active
   (min_frames never reached) and with every tile retired (each wave returns after one load).
 * buys: per threshold, from frameCounter 0, windows of `every` frames with an update after each until
   every tile has retired or `max-frames` frames: per window the frames so far, the retired share going
   into the window (what its frames skipped), max_err2 after its update, ms per frame of the window in
   both contexts (the same frame numbers), and the rays so far against frames x pixels of the moments
   context. saved_over_retired: (1 - adaptive / moments ms) / retired share of the window -- 1 would
   be time proportional to the active tiles.
One JSON line per config.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--every", type=int, default=48)
    ap.add_argument("--max-frames", type=int, default=4096)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[1 / 255, 4 / 255])
    ap.add_argument("--idle-only", action="store_true", help="only the nothing-retired comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    if not torch.cuda.is_available():
        raise RuntimeError("adaptive_time: no GPU visible")
    lines = []
    for name in a.configs:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        eye, rot = orbit_camera(*cfg.camera)
        w, h = cfg.width, cfg.height
        stream = torch.cuda.Stream()

        def context(**kw):
            r = Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce, **kw)
            r.upload_scene(tris, nodes)
            r.upload_env(hdr)
            r.set_stream(stream.cuda_stream)
            return r

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        res = {"config": name, "width": w, "height": h, "tiles": ((w + 7) // 8) * ((h + 7) // 8)}

        def warm(ctxs):
            for r in ctxs.values():
                for f in range(32):
                    r.render_frame(eye, rot, f)
                r.synchronize()
            return {key: 32 for key in ctxs}

        def idle_runs(ctxs, fc):
            idle = {key: [] for key in ctxs}
            for k in range(a.runs):
                for key, r in (list(ctxs.items())[::-1] if k & 1 else ctxs.items()):  # each goes first in turn
                    ms = timed(lambda: r.render_frames(eye, rot, fc[key], a.frames))
                    fc[key] += a.frames
                    idle[key].append(ms / a.frames)
            return idle

        # ---- nothing retired, the pair created in either order
        with context(moments=True) as mo, context(adaptive=True) as ad:
            ctxs = {"moments": mo, "adaptive": ad}
            res["idle_ms_per_frame_moments_first"] = idle_runs(ctxs, warm(ctxs))
        with context(adaptive=True) as ad, context(moments=True) as mo:
            ctxs = {"adaptive": ad, "moments": mo}
            fc = warm(ctxs)
            res["idle_ms_per_frame_adaptive_first"] = idle_runs(ctxs, fc)
            af, mf = res["idle_ms_per_frame_adaptive_first"], res["idle_ms_per_frame_moments_first"]
            # like against like: the context created first of its pair, and the one created second
            pos = {"created_first": (af["adaptive"], mf["moments"]), "created_second": (mf["adaptive"], af["moments"])}
            med = lambda v: sorted(v)[len(v) // 2]
            res["idle_ranges_overlap"] = {k: min(x) <= max(y) and min(y) <= max(x) for k, (x, y) in pos.items()}
            res["idle_adaptive_over_moments_median"] = {k: med(x) / med(y) for k, (x, y) in pos.items()}
            every = af["adaptive"] + af["moments"] + mf["adaptive"] + mf["moments"]
            spread = max(every) - min(every)
            res["idle_spread_ms"] = spread
            if a.idle_only:
                print(json.dumps(res), flush=True)
                lines.append(json.dumps(res))
                continue
            # ---- the update
            never = dict(min_frames=1 << 30)
            ad.adaptive_update(**never)
            res["update_active_ms"] = timed(lambda: [ad.adaptive_update(**never) for _ in range(a.reps)]) / a.reps
            assert ad.adaptive_status().retired == 0
            ad.adaptive_update(threshold=1e30, min_frames=2)
            assert ad.adaptive_status().retired == res["tiles"]
            res["update_retired_ms"] = timed(lambda: [ad.adaptive_update() for _ in range(a.reps)]) / a.reps
            res["update_MB_read"] = 24.0 * w * h / 1e6
            # ---- what it buys
            res["buys"] = {}
            for thr in a.thresholds:
                rows = []
                done = 0
                rays0 = {key: r.stats().rays for key, r in ctxs.items()}
                retired = 0
                while done < a.max_frames:
                    n = min(a.every, a.max_frames - done)
                    order = list(ctxs.items())[::-1] if len(rows) & 1 else list(ctxs.items())  # each goes first in turn
                    ms = {key: timed(lambda r=r: r.render_frames(eye, rot, done, n)) / n for key, r in order}
                    done += n
                    going_in = retired / res["tiles"]
                    ad.adaptive_update(threshold=thr)
                    st = ad.adaptive_status()
                    retired = st.retired
                    rays = {key: r.stats().rays - rays0[key] for key, r in ctxs.items()}
                    saved = 1.0 - ms["adaptive"] / ms["moments"]
                    rows.append({"frames": done, "retired_share_in": going_in, "retired_share": retired / res["tiles"],
                                 "max_err2": st.max_err2, "ms_adaptive": ms["adaptive"], "ms_moments": ms["moments"],
                                 "within_idle_spread": ms["adaptive"] <= ms["moments"] + spread,
                                 "saved_over_retired": saved / going_in if going_in > 0 else None,
                                 "rays_adaptive": rays["adaptive"], "rays_moments": rays["moments"],
                                 "pixel_samples": done * w * h})
                    if retired == res["tiles"]:
                        break
                res["buys"][f"{thr:.5f}"] = rows
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
