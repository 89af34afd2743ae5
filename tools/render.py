#!/usr/bin/env python3
"""Headless stand-in for the reference's display loop: render a benchmark
configuration progressively and write the image.

    python tools/render.py --config c2 --frames 64 --out gpurun_out/c2.png   # pass3 tonemap + PNG
    python tools/render.py --config c4 --frames 16 --out gpurun_out/c4.pfm   # linear accumulation
    python tools/render.py --config c4 --frames 4 --denoise --out out/c4.png  # + out/c4_denoised.png
    python tools/render.py --config c4 --frames 64 --denoise var --out out/c4.png  # pt_denoise_var instead
    python tools/render.py --config c2 --drag 8 --step 2 --out out/c2.png     # a camera drag, see below
    python tools/render.py --config c2 --frames 4096 --adaptive 0.0039 --update-every 48 --out out/c2.png  # see below

PNG: pass3's tonemap (pass3.fsh:14-24, limit 1.5) then imshow's gamma 2.2
(BasicRayTracingWithC++/main.cpp:169-190); the BASIC config skips the tonemap
like the reference CPU tracer. PFM: the linear running mean.

--drag N --step DEG: N cameras DEG degrees apart on the orbit, ending at the config's camera, each
with --frames frames (default 1 with --drag) from frameCounter 0, resolved against the history of
the cameras before it (pt_temporal_resolve / pt_temporal_commit). Writes the last camera's raw
running mean to <out>, the resolved image to <out>_resolved.png and the resolved image through the
a-trous filter (pt_denoise_from; with --denoise var the variance-guided one, pt_denoise_var) to
<out>_resolved_denoised.png.

--adaptive THR [--update-every N]: adaptive sampling (PT_FLAG_ADAPTIVE). Renders windows of N frames
(default 16) with a pt_adaptive_update after each, to --frames or until every 8x8 tile has retired,
and prints frames / retired tiles / max_err2 per update and the rays against frames x pixels.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--frames", type=int, default=None, help="frames per camera (default 16; 1 with --drag)")
    ap.add_argument("--out", default="gpurun_out/render.png")
    ap.add_argument("--builder", default=None)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--denoise", nargs="?", const="atrous", default=None, choices=["atrous", "var"],
                    help="also write <out>_denoised.png: pt_denoise (default), or with `var` the variance-guided "
                         "pt_denoise_var steered by the sample moments")
    ap.add_argument("--drag", type=int, default=0, help="render a drag of N cameras with the temporal resolve")
    ap.add_argument("--step", type=float, default=2.0, help="--drag: degrees between two cameras")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THR",
                    help="adaptive sampling (PT_FLAG_ADAPTIVE): 8x8 tiles whose standard error of the tone-mapped "
                         "luminance is <= THR (e.g. 0.0039 = 1/255) retire; renders to --frames or until every tile has")
    ap.add_argument("--update-every", type=int, default=16, metavar="N", help="--adaptive: frames between two decisions")
    a = ap.parse_args()
    if a.adaptive is not None and (a.drag or a.update_every < 1):
        ap.error("--adaptive: not with --drag, and --update-every must be >= 1")
    if a.frames is None:
        a.frames = 1 if a.drag else 16
    import numpy as np

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes, write_pfm, write_png
    cfg, tris, nodes, hdr = scenes.build_config(a.config, a.builder)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    basic = cfg.integrator == "basic"
    if a.drag and basic:
        ap.error("--drag: not for the BASIC config")

    def write_tm_png(path, c):
        lum = np.float32(0.3) * c[..., 0] + np.float32(0.6) * c[..., 1] + np.float32(0.1) * c[..., 2]
        tm = c[..., :3] * (np.float32(1) / (np.float32(1) + lum / np.float32(1.5)))[..., None]
        write_png(path, np.ascontiguousarray(tm, np.float32), 2.2, flip_rows=True)

    if a.adaptive is not None and basic:
        ap.error("--adaptive: not for the BASIC config")
    kw = dict(basic_samples=a.frames) if basic else dict(moments=a.denoise == "var", adaptive=a.adaptive is not None)
    with Renderer(cfg.width, cfg.height, cfg.integrator, max_bounce=cfg.max_bounce, flags=a.flags, **kw) as r:
        if basic:
            r.upload_shapes(scenes.cornell_shapes())
            eye, rot = np.zeros(3, np.float32), np.eye(4, dtype=np.float32)
        else:
            r.upload_scene(tris, nodes)
            r.upload_env(hdr)
            eye, rot = orbit_camera(*cfg.camera)
        t0 = time.perf_counter()
        if a.drag:
            angle, up, rad = cfg.camera
            for k in range(a.drag):
                eye, rot = orbit_camera(angle - (a.drag - 1 - k) * a.step, up, rad)
                if k:
                    r.temporal_commit()
                r.render_guides(eye, rot)
                for f in range(a.frames):
                    r.render_frame(eye, rot, f, sync=False)
                r.temporal_resolve(a.frames, download=False)
        elif a.adaptive is not None:
            # windows of --update-every frames, a decision after each, until every tile has retired
            done = 0
            while done < a.frames:
                n = min(a.update_every, a.frames - done)
                r.render_frames(eye, rot, done, n)
                done += n
                r.adaptive_update(threshold=a.adaptive, min_frames=max(2, min(16, a.update_every)))
                s = r.adaptive_status()
                print(f"{a.config}: {s.frames} frames, {s.retired} of {s.tiles} tiles retired, max_err2 {s.max_err2:.3e}")
                if s.retired == s.tiles:
                    break
            pix = done * cfg.width * cfg.height
            print(f"{a.config}: {r.stats().rays} rays for {done} frames x {cfg.width * cfg.height} pixels = {pix} "
                  f"pixel samples ({r.stats().rays / pix:.3f} rays per pixel sample)")
            a.frames = done
        else:
            for f in range(a.frames):
                r.render_frame(eye, rot, f, sync=False)
        r.synchronize()
        dt = time.perf_counter() - t0
        st = r.stats()
        if a.out.endswith(".pfm"):
            write_pfm(a.out, r.accum())
        elif basic:  # imshow of the reference's double image (main.cpp:169-190)
            from PIL import Image

            from opengl_ray_tracing_amd.scene import imshow_bytes
            Image.fromarray(imshow_bytes(r.basic_image())).save(a.out)
        else:
            write_png(a.out, r.tonemap(1.5), 2.2, flip_rows=True)
        if a.drag:
            out = Path(a.out)
            resolved = r.temporal_resolve(a.frames)
            name = str(out.with_name(out.stem + "_resolved.png"))
            write_tm_png(name, resolved)
            both = (r.denoise_var if a.denoise == "var" else r.denoise)(src_dptr=r.resolved_device_ptr())
            name2 = str(out.with_name(out.stem + "_resolved_denoised.png"))
            write_tm_png(name2, both)
            print(f"{a.config}: drag of {a.drag} cameras, {a.step:g} deg apart -> {name}, {name2}")
        if a.denoise and not basic:
            # the edge-avoiding a-trous filter of the running mean (pt_denoise or pt_denoise_var, default
            # parameters), through the same tonemap and gamma, beside the plain image
            r.render_guides(eye, rot)
            c = (r.denoise_var() if a.denoise == "var" else r.denoise())[..., :3]
            lum = np.float32(0.3) * c[..., 0] + np.float32(0.6) * c[..., 1] + np.float32(0.1) * c[..., 2]
            tm = c * (np.float32(1) / (np.float32(1) + lum / np.float32(1.5)))[..., None]
            out = Path(a.out)
            dn = str(out.with_name(out.stem + "_denoised.png"))
            write_png(dn, np.ascontiguousarray(tm, np.float32), 2.2, flip_rows=True)
            print(f"{a.config}: denoised -> {dn}")
    print(f"{a.config}: {a.frames} frames in {dt * 1e3:.1f} ms, {st.rays / dt / 1e6:.1f} Mrays/s -> {a.out}")


if __name__ == "__main__":
    main()
