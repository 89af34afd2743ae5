#!/usr/bin/env python3
"""An equirectangular panorama of a config from a point, path-traced through the radiance query.

    python tools/panorama.py --config c2 --frames N --out pano.png [--size 1024x512] [--eye X Y Z] [--gamma 2.2] [--batch B]

A camera the frame kernels do not have: torch builds one ray per pixel of a W x H equirectangular image
from the eye (default: the config's camera position), column = azimuth over 360 degrees, row = elevation
from straight up to straight down; every sample jitters the rays inside their pixels (seeded per sample).
pt_radiance_device gives one sample of the config's integrator along them per call (ids None: ray k is
seeded as (k & 4095, k >> 12), distinct for W * H < 2^23), and the N samples are folded into a running
mean with the frames' weights 1 / (i + 1) in torch. The mean is tone-mapped as pass3 does (limit 1.5)
and written as an 8-bit PNG. Rays, samples and mean stay on the GPU, on the stream the renderer was
handed (pt_set_stream); one image leaves it at the end.
With --batch B the jittered rays of B samples are built at once and pt_radiance_mean_device folds them on
the GPU, one call per B samples and no fold in torch: the mean goes on from call to call in the call's own
buffer, with the frames' weights and floats.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def panorama_rays(w: int, h: int, eye, sample: int, device="cuda"):
    """(h * w, 6) float32 rays on the GPU: row 0 looks up, the centre column along -z (the configs' view
    direction), columns turning towards +x; pixel
    (col, row) at ray row * w + col, jittered inside its pixel by sample's seeded offsets."""
    import torch
    gen = torch.Generator(device=device)
    gen.manual_seed(1000003 * sample + 17)
    j = torch.rand((h, w, 2), generator=gen, device=device, dtype=torch.float32)
    col = torch.arange(w, device=device, dtype=torch.float32)[None, :]
    row = torch.arange(h, device=device, dtype=torch.float32)[:, None]
    phi = (col + j[..., 0]) * (2.0 * math.pi / w) - math.pi
    theta = (row + j[..., 1]) * (math.pi / h)
    st = torch.sin(theta)
    d = torch.stack([st * torch.sin(phi), torch.cos(theta), -st * torch.cos(phi)], dim=2)
    d = torch.nn.functional.normalize(d, dim=2)
    o = torch.tensor([float(x) for x in eye], device=device, dtype=torch.float32).expand(h, w, 3)
    return torch.cat([o, d], dim=2).reshape(-1, 6).contiguous()


def render(r, w: int, h: int, eye, frames: int, stream, batch: int = 0):
    """-> the running mean of `frames` samples, (h, w, 3) float32 tensor, row 0 = up. r renders on `stream`.
    batch > 0: that many samples per pt_radiance_mean_device call."""
    import torch
    with torch.cuda.stream(stream):
        if batch > 0:
            mean4 = torch.empty((h * w, 4), dtype=torch.float32, device="cuda")
            for i in range(0, frames, batch):
                b = min(batch, frames - i)
                rays = torch.stack([panorama_rays(w, h, eye, i + j) for j in range(b)])
                r.radiance_mean_device(rays, None, i, b, per_sample_rays=True, mean=mean4)
            return mean4[:, 0:3].reshape(h, w, 3)
        mean = torch.zeros((h * w, 3), dtype=torch.float32, device="cuda")
        out = torch.empty((h * w, 4), dtype=torch.float32, device="cuda")
        for i in range(frames):
            rays = panorama_rays(w, h, eye, i)
            r.radiance_device(rays, None, i, out)  # in stream order behind the rays' producer
            mean = torch.lerp(mean, out[:, 0:3], 1.0 / (i + 1))
    return mean.view(h, w, 3)


def tonemap(img, limit: float = 1.5):
    """pass3.fsh's tone mapping (pt_device.h tonemapPixel), on a torch tensor"""
    lum = 0.3 * img[..., 0] + 0.6 * img[..., 1] + 0.1 * img[..., 2]
    return img * (1.0 / (1.0 + lum / limit))[..., None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "c4", "c5"])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", default="1024x512")
    ap.add_argument("--eye", type=float, nargs=3, default=None)
    ap.add_argument("--gamma", type=float, default=2.2)
    ap.add_argument("--out", default="pano.png")
    ap.add_argument("--batch", type=int, default=0, help="samples per pt_radiance_mean_device call (0: one pt_radiance_device call per sample, folded in torch)")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.lower().split("x"))
    if w * h >= 1 << 23:
        raise SystemExit("panorama: the default ray ids are distinct below 2^23 rays")
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    from opengl_ray_tracing_amd.scene import write_png
    if not torch.cuda.is_available():
        raise RuntimeError("panorama: no GPU visible")
    cfg, tris, nodes, hdr = scenes.build_config(a.config)
    eye = a.eye if a.eye is not None else orbit_camera(*cfg.camera)[0]
    stream = torch.cuda.Stream()
    with Renderer(64, 64, cfg.integrator, max_bounce=cfg.max_bounce) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        r.set_stream(stream.cuda_stream)
        render(r, w, h, eye, 1, stream, a.batch)  # first use: the query's own resources, torch's kernels
        stream.synchronize()
        t0 = time.perf_counter()
        mean = render(r, w, h, eye, a.frames, stream, a.batch)
        with torch.cuda.stream(stream):  # behind the last sample's fold, not on torch's default stream
            img = tonemap(mean)
        stream.synchronize()
        seconds = time.perf_counter() - t0
        img = img.cpu().numpy()
        r.set_stream(None)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    write_png(a.out, img, gamma=a.gamma, flip_rows=False)
    print(json.dumps({"config": a.config, "width": w, "height": h, "frames": a.frames, "batch": a.batch, "seconds": round(seconds, 4),
                      "ms_per_frame": round(1e3 * seconds / a.frames, 4),
                      "mpaths_per_s": round(w * h * a.frames / seconds / 1e6, 1), "mean": float(img.mean()),
                      "finite": bool((img == img).all()), "out": a.out}))


if __name__ == "__main__":
    main()
