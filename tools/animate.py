#!/usr/bin/env python3
"""A deforming scene rendered pose by pose without a trip through the host.

    python tools/animate.py --config c2 --poses 8 --frames 16 --out DIR [--size WxH] [--amplitude A] [--materials] [--sky]

The scene is uploaded once. For every pose torch displaces the vertices on the stream the renderer was
handed (pt_set_stream) -- a travelling wave, a function of each vertex's position, so shared vertices stay
shared -- and pt_update_geometry_device reads them there in stream order; then `--frames` frames restart
the running mean and one PNG per pose (pose_000.png ..., row 0 = the top row) is written. With
--materials torch also changes the materials per pose on that stream -- the emitters pulse, the
roughness of everything else sweeps between 0.05 and 0.95 -- and pt_update_materials_device rebuilds the
material table from them in place. With --sky torch also turns and dims the environment per pose on that
stream -- the map rolled along its width and scaled by a power of two, both of which keep RGBE texels
exact, so the compact forms keep serving -- and pt_update_env_device rebuilds every form of it in place:
no pose needs a new upload. One JSON line with the wall times.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    ap.add_argument("--amplitude", type=float, default=0.04, help="of the scene's extent")
    ap.add_argument("--materials", action="store_true", help="also animate emission and roughness (update_materials)")
    ap.add_argument("--sky", action="store_true", help="also turn and dim the environment (update_env)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    from opengl_ray_tracing_amd.scene import write_png
    if not torch.cuda.is_available():
        raise RuntimeError("animate: no GPU visible")
    cfg, tris, nodes, hdr = scenes.build_config(a.config)
    w, h = (int(x) for x in a.size.split("x")) if a.size else (cfg.width, cfg.height)
    eye, rot = orbit_camera(*cfg.camera)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    stream = torch.cuda.Stream()
    update_ms, material_ms, sky_ms, sky_compact, pose_ms = [], [], [], [], []
    with Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        rest = torch.from_numpy(np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 36)[:, :18])).to("cuda:0")
        # Triangle_encoded floats 18..35: emissive 0..2, roughness 10 (include/pt_scene.h pt_material)
        look = torch.from_numpy(np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 36)[:, 18:])).to("cuda:0")
        sky = torch.from_numpy(np.ascontiguousarray(hdr, np.float32)).to("cuda:0")
        p = rest[:, :9].reshape(-1, 3)
        ext = float((p.max(0).values - p.min(0).values).max())
        n = rest.shape[0]
        torch.cuda.synchronize()
        r.set_stream(stream.cuda_stream)
        for k in range(a.poses):
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                phase = 2.0 * math.pi * k / max(a.poses, 1)
                v = rest.clone()
                q = v[:, :9].view(n, 3, 3)  # a view: the displacement lands in v
                q += (a.amplitude * ext) * torch.sin((6.0 / ext) * q[..., [1, 2, 0]] + phase)
                t1 = time.perf_counter()
                r.update_geometry(v)  # no synchronisation between the deformation and the update
                update_ms.append((time.perf_counter() - t1) * 1e3)
                if a.materials:
                    m = look.clone()
                    m[:, 0:3] *= 0.6 + 0.4 * math.cos(phase)
                    dark = (look[:, 0:3] == 0).all(1)
                    m[dark, 10] = 0.5 + 0.45 * math.sin(phase)
                    t2 = time.perf_counter()
                    r.update_materials(m)  # in stream order too
                    material_ms.append((time.perf_counter() - t2) * 1e3)
                if a.sky:
                    turned = (torch.roll(sky, (k * sky.shape[1]) // max(a.poses, 1), 1) * 2.0 ** -(k % 3)).contiguous()
                    t3 = time.perf_counter()
                    r.update_env(turned)  # in stream order too; the same size every pose: nothing is allocated after the first
                    sky_ms.append((time.perf_counter() - t3) * 1e3)
                    sky_compact.append(r.stats().env_compact)
            r.render_frames(eye, rot, 0, a.frames)
            img = r.tonemap(1.5)
            pose_ms.append((time.perf_counter() - t0) * 1e3)
            write_png(str(out / f"pose_{k:03d}.png"), img)
        r.set_stream(None)
    print(json.dumps({"config": a.config, "size": [w, h], "poses": a.poses, "frames_per_pose": a.frames,
                      "update_ms": [round(x, 3) for x in update_ms],
                      "material_update_ms": [round(x, 3) for x in material_ms],
                      "env_update_ms": [round(x, 3) for x in sky_ms], "env_compact": sky_compact, "pose_ms": [round(x, 3) for x in pose_ms],
                      "out": str(out)}))


if __name__ == "__main__":
    main()
