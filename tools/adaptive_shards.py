#!/usr/bin/env python3
"""Adaptive sampling on a screen-tile split (PT_FLAG_SHARE_MOMENTS): every rank renders its share in
windows of --update-every frames, gathers the running means with the moments to rank 0
(distributed.FrameGather(moments=True)), decides its own 8x8 tiles (pt_adaptive_update) and the ranks
combine their statuses; all stop together when the *image's* status says every tile has retired, or
at --frames. Rank 0 prints frames / retired / max_err2 per update, as render.py --adaptive does, and
writes the PNG (with --denoise var also <out>_denoised.png: pt_denoise_var on the gathered moments).

    torchrun --nproc-per-node N tools/adaptive_shards.py --config c2 --adaptive 0.0039 --update-every 48 \\
        --frames 4096 --out out/c2.png [--denoise var]
    python tools/adaptive_shards.py --proxy 8 --config c2 --adaptive 0.0039 ... [--never] [--json OUT.json]

Under torchrun each process takes GPU LOCAL_RANK when there are that many (RCCL), else all share GPU 0
and the collective is gloo. --proxy N needs no launcher: the N ranks are N contexts of this one process
on one GPU, rendered one after the other and timed each on its own, which is what each of N GPUs would
take for its share -- the split's window is the slowest rank's. It reports per update the ms per frame
of the slowest and of the mean rank and how unevenly the active tiles fall (max over mean of the active
tiles per rank). --never: the same windows and updates with nothing retiring (the baseline)."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import opengl_ray_tracing_amd  # noqa: E402,F401  (hardware queues: the package's policy, before HIP initialises)


def args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--adaptive", type=float, default=1 / 255, metavar="THR")
    ap.add_argument("--update-every", type=int, default=16, metavar="K")
    ap.add_argument("--denoise", default=None, choices=["var"])
    ap.add_argument("--out", default="out/adaptive_shards.png")
    ap.add_argument("--proxy", type=int, default=0, metavar="N", help="N ranks as contexts of this one process")
    ap.add_argument("--never", action="store_true", help="nothing retires: the same split's baseline")
    ap.add_argument("--json", default=None, help="--proxy: write the windows' figures here")
    a = ap.parse_args()
    if a.update_every < 1 or a.frames < 1:
        ap.error("--update-every and --frames must be >= 1")
    return a


def make(cfg, tris, nodes, hdr, rank, world, device=0):
    from opengl_ray_tracing_amd import Renderer
    r = Renderer(cfg.width, cfg.height, cfg.integrator, max_bounce=cfg.max_bounce, device=device, tile_rank=rank,
                 tile_world=world, adaptive=True, share_moments=world > 1)
    r.upload_scene(tris, nodes)
    r.upload_env(hdr)
    return r


def prm(a):
    return dict(threshold=a.adaptive, min_frames=a.frames + 1 if a.never else max(2, min(16, a.update_every)))


def write_images(a, r, eye, rot):
    import numpy as np

    from opengl_ray_tracing_amd import write_png
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    write_png(a.out, r.tonemap(1.5), 2.2, flip_rows=True)
    print(f"{a.config}: running mean -> {a.out}")
    if a.denoise == "var":
        r.render_guides(eye, rot)
        c = r.denoise_var()[..., :3]
        lum = np.float32(0.3) * c[..., 0] + np.float32(0.6) * c[..., 1] + np.float32(0.1) * c[..., 2]
        tm = c * (np.float32(1) / (np.float32(1) + lum / np.float32(1.5)))[..., None]
        dn = str(Path(a.out).with_name(Path(a.out).stem + "_denoised.png"))
        write_png(dn, np.ascontiguousarray(tm, np.float32), 2.2, flip_rows=True)
        print(f"{a.config}: pt_denoise_var on {r.moments_frames()} frames of gathered moments -> {dn}")


def ranks_main(a):
    import torch
    import torch.distributed as dist

    from opengl_ray_tracing_amd import orbit_camera, scenes
    from opengl_ray_tracing_amd.distributed import FrameGather, broadcast_scene
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    real = torch.cuda.device_count() >= int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    dev = local if real else 0
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if real else "gloo", rank=rank, world_size=world)
    try:
        cfg = scenes.CONFIGS[a.config]
        tris, nodes, hdr = broadcast_scene(lambda: scenes.build_config(a.config)[1:], rank, f"cuda:{dev}")
        eye, rot = orbit_camera(*cfg.camera)
        r = make(cfg, tris, nodes, hdr, rank, world, dev)
        g = FrameGather(r, rank, world, f"cuda:{dev}", mode="accum", moments=world > 1) if world > 1 else None
        done, t0 = 0, time.perf_counter()
        while done < a.frames:
            n = min(a.update_every, a.frames - done)
            r.render_frames(eye, rot, done, n)
            done += n
            if g is not None:
                g()
            r.adaptive_update(**prm(a))
            s = g.adaptive_status() if g is not None else r.adaptive_status()
            if rank == 0:
                print(f"{a.config}: {s.frames} frames, {s.retired} of {s.tiles} tiles retired, max_err2 {s.max_err2:.3e}",
                      flush=True)
            if s.retired == s.tiles:  # the image's status, the same on every rank
                break
        if g is not None:
            g.synchronize()
        r.synchronize()
        dt = time.perf_counter() - t0
        rays = torch.tensor([float(r.stats().rays)], device="cpu" if not real else f"cuda:{dev}")
        dist.all_reduce(rays)
        if rank == 0:
            pix = done * cfg.width * cfg.height
            print(f"{a.config}: {world} ranks, {done} frames in {dt:.3f} s, {int(rays.item())} rays "
                  f"({rays.item() / pix:.3f} per pixel sample)")
            write_images(a, r, eye, rot)
        r.close()
    finally:
        dist.destroy_process_group()


def proxy_main(a):
    import numpy as np
    import torch

    from opengl_ray_tracing_amd import orbit_camera, scenes
    n = a.proxy
    cfg, tris, nodes, hdr = scenes.build_config(a.config)
    eye, rot = orbit_camera(*cfg.camera)
    ranks = [make(cfg, tris, nodes, hdr, k, n) for k in range(n)]
    bufs = [torch.zeros((max(r.owned_pixel_count(), 1), 5), dtype=torch.float32, device="cuda:0") for r in ranks]
    torch.cuda.synchronize()
    for r in ranks:  # the policy probe and warm-up of every context, then from frame 0
        r.render_frames(eye, rot, 0, 40)
        r.synchronize()
    windows, done = [], 0
    while done < a.frames:
        m = min(a.update_every, a.frames - done)
        ms, sts = [], []
        for r, b in zip(ranks, bufs):
            t0 = time.perf_counter()
            r.render_frames(eye, rot, done, m)
            if n > 1:
                r.pack_owned_stats(b.data_ptr())
            r.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / m)
            r.adaptive_update(**prm(a))
            sts.append(r.adaptive_status())
        if n > 1:
            ranks[0].unpack_ranks_stats(n, [0] + [b.data_ptr() for b in bufs[1:]])
        done += m
        tiles, retired = sum(s.tiles for s in sts), sum(s.retired for s in sts)
        active = np.array([s.tiles - s.retired for s in sts], np.float64)
        w = {"frames": done, "tiles": tiles, "retired": retired, "max_err2": max(s.max_err2 for s in sts),
             "ms_per_frame_slowest_rank": round(max(ms), 4), "ms_per_frame_mean_rank": round(sum(ms) / n, 4),
             "active_tiles_max_over_mean": round(float(active.max() / active.mean()), 3) if active.mean() > 0 else None}
        windows.append(w)
        print(f"{a.config}: {done} frames, {retired} of {tiles} tiles retired, max_err2 {w['max_err2']:.3e}, "
              f"{w['ms_per_frame_slowest_rank']} ms/frame slowest rank ({w['ms_per_frame_mean_rank']} mean), "
              f"active tiles max/mean {w['active_tiles_max_over_mean']}", flush=True)
        if retired == tiles:
            break
    out = {"config": a.config, "world": n, "threshold": a.adaptive, "update_every": a.update_every, "never": a.never,
           "rays": sum(r.stats().rays for r in ranks), "windows": windows}
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    write_images(a, ranks[0], eye, rot)
    for r in ranks:
        r.close()


if __name__ == "__main__":
    a = args()
    proxy_main(a) if a.proxy else ranks_main(a)
