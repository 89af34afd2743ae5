#!/usr/bin/env python3
"""Device time of the guide buffers, the a-trous passes, the denoised display and the temporal
resolve on the GPU.

    python tools/denoise_time.py [c2 c4 ...] [--reps 100] [--out out/denoise_time.json]

Method: the renderer runs on a torch stream, HIP events (torch.cuda.Event) around `reps`
repetitions after a warm-up, profiler off, each config at its own size (c2 / c4: 1080p).
 * guides: pt_render_guides.
 * denoise[k]: pt_denoise with k passes (the tone-mapped plane of the accumulation + k passes).
 * pass[s]: denoise[k] - denoise[k-1] for s = 2^(k-1) (pass[1] includes the accumulation's
   tone-mapped plane; the last pass of a call writes no tone-mapped plane), and its compulsory
   80 B/pixel (16 B colour in, 48 B guides, 16 B colour out) over that time.
 * display: pt_display_denoised.
 * frame: wall time per iteration of pt_denoise (defaults) + pt_display_denoised + one synchronous
   pt_render_frame -- what a display() pays per presented frame (60 Hz: 16.6 ms).
 * temporal: pt_temporal_resolve after a commit and a 1 degree camera move (new guides, 4 frames of
   the new camera), 10 x reps repetitions, and its compulsory 112 B/pixel (6 planes read, 1 written:
   232 MB at 1080p) over that time, against the HBM peak. Two things make that rate no HBM rate: the
   7 planes fit the 256 MiB Infinity Cache, so back-to-back repetitions find them there (the a-trous
   rows are measured the same way), and a miss pixel touches 48 B, not 112 (hit_share, and
   temporal_touched_MB = (48 + 64 hit_share) B/pixel). temporal_cold: each repetition timed by its
   own event pair after a read of a 1 GiB buffer has swept the caches (an event pair adds a few
   microseconds). temporal_nohist: the call after pt_temporal_reset (a copy of the accumulation
   with the count, 32 B/pixel).
 * atrous / var / var_spatial _pass_ms_by_stride: pt_denoise and pt_denoise_var (variance from the
   moments, and the spatial estimate) pass by pass in one more context of the same process that
   holds 32 frames of moments, and var_over_atrous_by_stride, their ratio per stride ([1] includes
   what precedes the first pass: one tone-mapped plane there, the luminance plane and step A here).
 * batch12 / single _launch_ms_plain / _moments: a 12-frame and a 1-frame launch (frame kernel and
   running-mean update, back to back on one stream) of a plain and of a PT_FLAG_MOMENTS context;
   single_call_wall_ms_*: a synchronous pt_render_frame each. The kernels' own times (mixKernel,
   mixMomentsKernel, varLumKernel, varInitKernel, atrousVarKernel) come from running this script
   under rocprofv3 --kernel-trace --stats.
One JSON line per config.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_COPY_TBS = 6.29  # measured HBM copy rate
HBM_PEAK_TBS = 8.0    # HBM3E peak of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c4"])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    if not torch.cuda.is_available():
        raise RuntimeError("denoise_time: no GPU visible")
    lines = []
    for name in a.configs:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        eye, rot = orbit_camera(*cfg.camera)
        w, h = cfg.width, cfg.height
        stream = torch.cuda.Stream()
        with Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce) as r:
            r.upload_scene(tris, nodes)
            r.upload_env(hdr)
            r.set_stream(stream.cuda_stream)
            frame = 0
            for _ in range(32):  # past the runtime's policy probe, a settled running mean
                r.render_frame(eye, rot, frame)
                frame += 1
            image = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def timed(fn):
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / a.reps

            res = {"config": name, "width": w, "height": h, "reps": a.reps}
            res["guides_ms"] = timed(lambda: r.render_guides(eye, rot))
            cum = [0.0] + [timed(lambda k=k: r.denoise(download=False, passes=k)) for k in range(1, 9)]
            res["denoise_ms_by_passes"] = {str(k): cum[k] for k in range(1, 9)}
            res["pass_ms_by_stride"] = {str(1 << (k - 1)): cum[k] - cum[k - 1] for k in range(1, 9)}
            res["pass_TBs_of_80B"] = {s: 80.0 * w * h / (ms * 1e-3) / 1e12 for s, ms in res["pass_ms_by_stride"].items()}
            res["hbm_copy_TBs"] = HBM_COPY_TBS
            res["denoise_default_ms"] = timed(lambda: r.denoise(download=False))
            res["display_ms"] = timed(lambda: r.display_denoised(image.data_ptr(), 1.5, 0.0))
            # the presented frame: filter + display + one synchronous progressive frame
            r.synchronize()
            st0 = r.stats()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                r.denoise(download=False)
                r.display_denoised(image.data_ptr(), 1.5, 0.0)
                r.render_frame(eye, rot, frame)
                frame += 1
            res["frame_wall_ms"] = (time.perf_counter() - t0) * 1e3 / a.reps
            st1 = r.stats()
            res["render_frame_kernel_ms"] = (st1.kernel_ms_total - st0.kernel_ms_total) / a.reps
            res["fits_60hz"] = res["frame_wall_ms"] <= 1000.0 / 60.0
            # the temporal resolve: the settled mean becomes the history, the camera moves 1 degree
            r.temporal_resolve(frame, download=False)
            r.temporal_commit()
            angle, up, rad = cfg.camera
            eye1, rot1 = orbit_camera(angle + 1.0, up, rad)
            r.render_guides(eye1, rot1)
            for f in range(4):
                r.render_frame(eye1, rot1, f)
            reps = a.reps
            a.reps = 10 * reps  # a 30 us kernel: a longer window
            res["temporal_ms"] = timed(lambda: r.temporal_resolve(4, download=False))
            a.reps = reps
            res["hit_share"] = float((r.guides()["tri"] >= 0).mean())
            res["temporal_touched_MB"] = (48.0 + 64.0 * res["hit_share"]) * w * h / 1e6
            res["temporal_GBs_touched"] = res["temporal_touched_MB"] / res["temporal_ms"]
            sweep = torch.ones(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB, 4 x the Infinity Cache
            torch.cuda.synchronize()
            cold = 0.0
            for _ in range(20):
                with torch.cuda.stream(stream):
                    sweep.sum()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r.temporal_resolve(4, download=False)
                e1.record(stream)
                e1.synchronize()
                cold += e0.elapsed_time(e1)
            del sweep
            res["temporal_cold_ms"] = cold / 20
            res["temporal_cold_GBs_touched"] = res["temporal_touched_MB"] / res["temporal_cold_ms"]
            res["temporal_MB_of_112B"] = 112.0 * w * h / 1e6
            res["temporal_GBs_of_112B"] = 112.0 * w * h / (res["temporal_ms"] * 1e-3) / 1e9
            res["hbm_peak_TBs"] = HBM_PEAK_TBS
            res["temporal_share_of_hbm_peak"] = res["temporal_GBs_of_112B"] / (HBM_PEAK_TBS * 1e3)
            r.temporal_reset()
            res["temporal_nohist_ms"] = timed(lambda: r.temporal_resolve(4, download=False))
        # the variance-guided filter against pt_denoise, and the running-mean update with the sample
        # moments against the plain one: two contexts in this same process
        ctxs = {}
        for key, moments in (("plain", False), ("moments", True)):
            q = Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce, frame_batch=12, moments=moments)
            q.upload_scene(tris, nodes)
            q.upload_env(hdr)
            q.set_stream(stream.cuda_stream)
            for f in range(32):  # past the policy probe; the moments hold 32 frames
                q.render_frame(eye, rot, f)
            q.render_guides(eye, rot)
            q.synchronize()
            ctxs[key] = q
        try:
            q = ctxs["moments"]
            assert q.moments_frames() == 32
            for key, fn in (("atrous", lambda k: q.denoise(download=False, passes=k)),
                            ("var", lambda k: q.denoise_var(download=False, passes=k)),
                            ("var_spatial", lambda k: q.denoise_var(download=False, passes=k, min_temporal=1000))):
                cum = [0.0] + [timed(lambda k=k: fn(k)) for k in range(1, 6)]
                res[f"{key}_ms_by_passes"] = {str(k): cum[k] for k in range(1, 6)}
                # [1] includes what precedes the first pass: pt_denoise's tone-mapped plane; pt_denoise_var's
                # luminance plane and step A
                res[f"{key}_pass_ms_by_stride"] = {str(1 << (k - 1)): cum[k] - cum[k - 1] for k in range(1, 6)}
            res["var_over_atrous_by_stride"] = {s: res["var_pass_ms_by_stride"][s] / res["atrous_pass_ms_by_stride"][s]
                                                for s in res["var_pass_ms_by_stride"]}
            res["var_default_ms"] = timed(lambda: q.denoise_var(download=False))
            # launches of 12 frames and of 1 frame, frame kernel and running-mean update together: the
            # difference between the two contexts is what the moments cost a launch (a 1-frame launch of
            # the plain context issued while nothing is in flight mixes inside its frame kernel; the
            # kernels' own times: rocprofv3 --kernel-trace --stats of this script, mixKernel / mixMomentsKernel)
            fc = {"plain": 32, "moments": 32}
            for n, label in ((12, "batch12"), (1, "single")):
                for key, c in ctxs.items():
                    def launch(c=c, key=key, n=n):
                        c.render_frames(eye, rot, fc[key], n)
                        fc[key] += n
                    res[f"{label}_launch_ms_{key}"] = timed(launch)
                res[f"{label}_moments_over_plain"] = res[f"{label}_launch_ms_moments"] / res[f"{label}_launch_ms_plain"]
            # each single frame waited for: the display() call, where the plain context mixes in its frame kernel
            for key, c in ctxs.items():
                c.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    c.render_frame(eye, rot, fc[key])
                    fc[key] += 1
                res[f"single_call_wall_ms_{key}"] = (time.perf_counter() - t0) * 1e3 / a.reps
        finally:
            for q in ctxs.values():
                q.close()
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
