#!/usr/bin/env python3
"""What a geometry update costs against the upload it replaces.

    python tools/update_time.py [c2 c4 c5] [--rounds 5] [--out out/update.json]

For each config the scene is uploaded once, then `rounds` rounds alternate three ways of showing the
renderer a deformed pose of the same triangles (two poses alternate, so every call changes the scene):
 * host:    pt_update_geometry from an (n, 18) host array
 * device:  pt_update_geometry_device from an (n, 18) tensor already on the GPU
 * upload:  pt_upload_scene of (tris', nodes') -- the baseline, what a caller had to do before: the
            records with the new positions and the nodes with the refitted boxes. The caller's own cost
            of refitting or rebuilding its tree is NOT in the figure (the boxes are taken from
            pt_download_node_boxes after an update), which favours the baseline.
Each is wall time of the synchronous call, min ... max over the rounds. The claim to check, by the
project's rule: the new path's slowest round beats the old path's fastest.
 * breakdown: one more device update with PT_UPDATE_TIMES set: device time (HIP events) of the records,
   the refit and the re-encode, the wall time of the runtime tree's rebuild (pt_build.hip, as
   pt_frame_stats.accel_build_ms), the heights of the uploaded tree and the height from which the
   refit's one-block tail takes over from the launches per height.
 * first_frames_ms: wall time of each of the first synchronous frames after an update (the launch
   policies are measured again: policyKey), and steady_frame_ms, the median of frames 24..31.
One JSON line per config.
"""
from __future__ import annotations

import argparse
import re
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from update_common import emit, step_times, wall, write_lines  # noqa: E402


def deformed(tris, phase):
    """(n, 18) f32: positions displaced by a function of the position, normals kept."""
    import numpy as np
    F = np.float32
    v = np.ascontiguousarray(tris[:, :18], F).copy()
    p = v[:, :9].reshape(-1, 3, 3)  # a view: the displacement lands in v
    ext = F((p.max((0, 1)) - p.min((0, 1))).max())
    p += (F(0.01) * ext) * np.sin((F(9.0) / ext) * p[..., [1, 2, 0]] + F(phase)).astype(F)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c4", "c5"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from opengl_ray_tracing_amd import Renderer, orbit_camera, scenes
    if not torch.cuda.is_available():
        raise RuntimeError("update_time: no GPU visible")
    lines = []
    for name in a.configs:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 36)
        nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
        eye, rot = orbit_camera(*cfg.camera)
        poses = [deformed(tris, 0.0), deformed(tris, 1.5)]
        with Renderer(cfg.width, cfg.height, cfg.integrator, max_bounce=cfg.max_bounce) as r:
            first_upload = wall(lambda: r.upload_scene(tris, nodes))
            r.upload_env(hdr)
            dev = [torch.from_numpy(p).to("cuda:0") for p in poses]
            torch.cuda.synchronize()
            # the baseline's arrays: the refitted boxes of each pose, from an update
            fresh = []
            for p in poses:
                r.update_geometry(p)
                t2, n2 = tris.copy(), nodes.copy()
                t2[:, :18] = p
                n2[:, 6:12] = r.node_boxes()
                fresh.append((t2, n2))
            ms = {"host": [], "device": [], "upload": []}
            stats = {}
            for k in range(a.rounds):
                q = k % 2
                ms["host"].append(wall(lambda: r.update_geometry(poses[q])))
                ms["device"].append(wall(lambda: r.update_geometry(dev[1 - q])))
                stats["update"] = r.stats()
                ms["upload"].append(wall(lambda: r.upload_scene(*fresh[q])))
                stats["upload"] = r.stats()
            text = step_times("PT_UPDATE_TIMES", lambda: r.update_geometry(dev[0]))
            m = re.search(r"records ([\d.]+) refit ([\d.]+) reencode ([\d.]+) build ([\d.]+) ms, (\d+) heights, tail from (\d+)", text)
            first = [wall(lambda f=f: r.render_frame(eye, rot, f)) for f in range(32)]
            st = r.stats()
        line = {
            "config": name, "triangles": int(tris.shape[0]), "nodes": int(nodes.shape[0]), "rounds": a.rounds,
            "first_upload_ms": round(first_upload, 3),
            **{f"{k}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            **{f"{k}_ms_rounds": [round(x, 3) for x in v] for k, v in ms.items()},
            "device_beats_upload": max(ms["device"]) < min(ms["upload"]),
            "host_beats_upload": max(ms["host"]) < min(ms["upload"]),
            "upload_over_device_min": round(min(ms["upload"]) / max(ms["device"]), 2),
            "accel_build_ms": {k: round(s.accel_build_ms, 3) for k, s in stats.items()},
            "breakdown": None if not m else {
                "records_ms": float(m.group(1)), "refit_ms": float(m.group(2)), "reencode_ms": float(m.group(3)),
                "build_wall_ms": float(m.group(4)), "heights": int(m.group(5)), "tail_from_height": int(m.group(6))},
            "first_frames_ms": [round(x, 3) for x in first[:8]],
            "steady_frame_ms": round(statistics.median(first[24:]), 3),
            "max_stack": st.max_stack, "accel_nodes": st.accel_nodes,
        }
        emit(lines, line)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
