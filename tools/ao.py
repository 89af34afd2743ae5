#!/usr/bin/env python3
"""Ambient occlusion of a config's camera view through the ray queries, built and consumed on the GPU.

    python tools/ao.py --config c2|c4 --size WxH --rays K --radius R --out ao.png [--bias B] [--seed S]

The pipeline never leaves the device: pt_render_guides gives every pixel's first hit (P, N); for every
hit pixel torch builds K cosine-weighted directions about N (seeded) on the stream the renderer was
handed (pt_set_stream); pt_trace_occluded_device tests them against the uploaded scene with tmax = R;
the mean visibility per pixel is the picture (a sky pixel is 1). One PNG, row 0 = the top row.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def camera_rays(w: int, h: int, eye, rot):
    """The camera ray through every pixel centre (pass1.fsh:846-850 with the jitter terms 0), (h * w, 6)
    float32 numpy, row 0 = the bottom row."""
    import numpy as np
    F = np.float32
    M = np.ascontiguousarray(rot, F).reshape(16)
    px = np.tile(np.arange(w, dtype=np.int64), h)
    py = np.repeat(np.arange(h, dtype=np.int64), w)
    x = (2 * px + 1).astype(F) / F(w) - F(1)
    y = (2 * py + 1).astype(F) / F(h) - F(1)
    d = np.stack([M[0 + k] * x + M[4 + k] * y + M[8 + k] * F(-1.5) for k in range(3)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.empty((w * h, 6), F)
    rays[:, 0:3] = np.ascontiguousarray(eye, F).reshape(3)
    rays[:, 3:6] = d
    return rays


def ao_rays(pos_t, nrm_tri, k: int, seed: int, bias: float = 0.0):
    """From the guide planes (H x W x 4 float32 tensors on the GPU): the flat indices of the hit pixels
    and, for each, k cosine-weighted directions about its normal leaving its hit point -- (m,) int64
    and (m * k, 6) float32, pixel-major; the origins are lifted by `bias` along the normal (the shading
    normal of a tessellated surface tilts rays into the neighbouring facets). On the current torch stream."""
    import torch
    dev = pos_t.device
    tri = nrm_tri.reshape(-1, 4)[:, 3].view(torch.int32)
    idx = torch.nonzero(tri >= 0).reshape(-1)
    P = pos_t.reshape(-1, 4)[idx, 0:3]
    N = nrm_tri.reshape(-1, 4)[idx, 0:3]
    m = idx.numel()
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    u = torch.rand((m, k, 2), generator=gen, device=dev, dtype=torch.float32)
    r, phi = torch.sqrt(u[..., 0]), (2.0 * math.pi) * u[..., 1]
    lx, ly, lz = r * torch.cos(phi), r * torch.sin(phi), torch.sqrt(torch.clamp(1.0 - u[..., 0], min=0.0))
    # a tangent frame about N (Frisvad's choice of helper axis)
    helper = torch.where((N[:, 0:1].abs() > 0.9).expand(-1, 3), torch.tensor([0.0, 1.0, 0.0], device=dev),
                         torch.tensor([1.0, 0.0, 0.0], device=dev))
    T = torch.nn.functional.normalize(torch.cross(helper, N, dim=1), dim=1)
    B = torch.cross(N, T, dim=1)
    d = lx[..., None] * T[:, None, :] + ly[..., None] * B[:, None, :] + lz[..., None] * N[:, None, :]
    d = torch.nn.functional.normalize(d, dim=2)
    rays = torch.cat([(P + bias * N)[:, None, :].expand(-1, k, -1), d], dim=2).reshape(-1, 6).contiguous()
    return idx, rays


def ambient_occlusion(r, w: int, h: int, eye, rot, k: int, radius: float, seed: int, stream, bias: float = 0.0):
    """-> (visibility (h, w) float32 tensor, row 0 = bottom; rays cast). r renders on `stream`."""
    import torch
    with torch.cuda.stream(stream):
        pos_t = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        nrm_tri = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        r.render_guides(eye, rot)
        r.guides_into(pos_t.data_ptr(), nrm_tri.data_ptr())
        idx, rays = ao_rays(pos_t, nrm_tri, k, seed, bias)
        vis = torch.ones(h * w, dtype=torch.float32, device="cuda")
        if idx.numel():
            tmax = torch.full((rays.shape[0],), float(radius), dtype=torch.float32, device="cuda")
            occ = r.trace_occluded_device(rays, tmax)  # in stream order behind the rays' producers
            vis[idx] = 1.0 - occ.view(-1, k).to(torch.float32).mean(dim=1)
    return vis.view(h, w), int(rays.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c2", "c3", "c4", "c5"])
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--rays", type=int, default=16)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--bias", type=float, default=1e-3, help="origin offset along the normal")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="ao.png")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.lower().split("x"))
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    from opengl_ray_tracing_amd.scene import write_png
    if not torch.cuda.is_available():
        raise RuntimeError("ao: no GPU visible")
    cfg, tris, nodes, hdr = scenes.build_config(a.config)
    eye, rot = orbit_camera(*cfg.camera)
    stream = torch.cuda.Stream()
    with Renderer(w, h, cfg.integrator, max_bounce=cfg.max_bounce) as r:
        r.upload_scene(tris, nodes)
        r.set_stream(stream.cuda_stream)
        vis, n = ambient_occlusion(r, w, h, eye, rot, a.rays, a.radius, a.seed, stream, a.bias)
        stream.synchronize()
        img = vis.cpu().numpy()
        r.set_stream(None)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    write_png(a.out, img[..., None].repeat(3, axis=2), gamma=1.0, flip_rows=True)
    print(json.dumps({"config": a.config, "width": w, "height": h, "rays_per_pixel": a.rays, "radius": a.radius,
                      "rays": n, "mean_visibility": float(img.mean()), "min_visibility": float(img.min()),
                      "out": a.out}))


if __name__ == "__main__":
    main()
