"""FrameGather(moments=True) between processes: two gloo ranks on the one GPU render c2 at 100x76 as a
screen-tile split with adaptive sampling, gather the running means with the moments after every
batch, decide every 8 frames and combine their statuses; rank 0's accumulation, moments and summed
tile planes must equal a one-context PT_FLAG_ADAPTIVE render bit for bit, and both ranks must see
the same status -- the image's. Three processes hold the GPU (this one only starts the two)."""
import os
import socket
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

W, H, FRAMES, EVERY = 100, 76, 16, 8
PRM = dict(threshold=4 / 255, limit=1.5, min_frames=8)
LIMIT_S = 150  # one limit for the whole run


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _one_context(cfg, tris, nodes, hdr, eye, rot):
    from opengl_ray_tracing_amd import Renderer
    statuses = []
    with Renderer(W, H, cfg.integrator, max_bounce=cfg.max_bounce, adaptive=True) as r:
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        for first in range(0, FRAMES, EVERY):
            r.render_frames(eye, rot, first, EVERY)
            r.adaptive_update(**PRM)
            st = r.adaptive_status()
            statuses.append((st.tiles, st.retired, st.frames, np.float32(st.max_err2).view(np.uint32).item()))
        return r.accum(), r.moments(), r.tile_error(), statuses


def _worker(rank, world, port, q):
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import torch
    import torch.distributed as dist

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    from opengl_ray_tracing_amd.distributed import FrameGather
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg, tris, nodes, hdr = scenes.build_config("c2")
        eye, rot = orbit_camera(*cfg.camera)
        r = Renderer(W, H, cfg.integrator, max_bounce=cfg.max_bounce, device=0, tile_rank=rank, tile_world=world,
                     adaptive=True, share_moments=True)
        r.upload_scene(tris, nodes)
        r.upload_env(hdr)
        g = FrameGather(r, rank, world, "cuda:0", mode="accum", moments=True)
        statuses = []
        for first in range(0, FRAMES, EVERY):
            r.render_frames(eye, rot, first, EVERY)
            g()
            r.adaptive_update(**PRM)
            st = g.adaptive_status()
            statuses.append((st.tiles, st.retired, st.frames, np.float32(st.max_err2).view(np.uint32).item()))
        g.synchronize()
        planes = g.tile_error()
        own = r.adaptive_status()
        result = {"rank": rank, "statuses": statuses, "own_tiles": own.tiles}
        if rank == 0:
            acc, m = r.accum(), r.moments()
            acc_ref, m_ref, (e_ref, at_ref), st_ref = _one_context(cfg, tris, nodes, hdr, eye, rot)
            result.update(accum=bool(np.array_equal(acc.view(np.uint32), acc_ref.view(np.uint32))),
                          moments=bool(np.array_equal(m.view(np.uint32), m_ref.view(np.uint32))),
                          err2=bool(np.array_equal(planes[0].view(np.uint32), e_ref.view(np.uint32))),
                          retired_at=bool(np.array_equal(planes[1], at_ref)),
                          reference=st_ref, frames=r.moments_frames(), staged=not g.overlap)
        else:
            result["planes_none"] = planes is None
        q.put(result)
        r.close()
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_gather_moments_and_agree_on_the_status():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(k, world, port, q)) for k in range(world)]
    deadline = time.monotonic() + LIMIT_S
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=max(0.0, deadline - time.monotonic()))
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    got = {r["rank"]: r for r in (q.get(timeout=5) for _ in range(world))}
    r0, r1 = got[0], got[1]
    assert r0["accum"] and r0["moments"] and r0["err2"] and r0["retired_at"], r0
    assert r0["frames"] == FRAMES and r0["staged"]
    assert r1["planes_none"]
    # both ranks see the image's status, which is the one context's
    assert r0["statuses"] == r1["statuses"] == r0["reference"], (r0["statuses"], r1["statuses"], r0["reference"])
    assert r0["statuses"][-1][0] == ((W + 7) // 8) * ((H + 7) // 8) == r0["own_tiles"] + r1["own_tiles"]
    assert 0 < r0["statuses"][0][1] <= r0["statuses"][1][1] < r0["statuses"][-1][0]  # part retires, part does not
