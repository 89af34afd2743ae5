#!/usr/bin/env python3
"""What a material update costs against the upload it replaces.

    python tools/material_time.py [c2 c5] [--rounds 5] [--out out/materials.json]

For each config the scene is uploaded once, then `rounds` rounds alternate three ways of showing the
renderer new materials for the same triangles. Two looks alternate, so every call changes the scene: the
scene's own few materials with another roughness, and a distinct material for every triangle (the largest
table an update can make, and the probe table's worst case: every insert claims a slot).
 * host:    pt_update_materials from an (n, 18) host array
 * device:  pt_update_materials_device from an (n, 18) tensor already on the GPU
 * upload:  pt_upload_scene of the records with those materials and the same nodes -- the baseline, what
            a caller had to do before (pt_frame_stats.upload_ms is reported beside the wall time)
Each is wall time of the synchronous call, min ... max over the rounds. The claim to check, by the
project's rule: the new path's slowest round beats the old path's fastest.
 * breakdown: one more device update per look with PT_MATERIAL_TIMES set: device time (HIP events) of the
   insert, of the flags and scan, and of the scatter, with the table's size and the probe table's slots.
One JSON line per config.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from update_common import emit, step_times, wall, write_lines  # noqa: E402


def looks(tris):
    """Two (n, 18) f32 looks of the records' materials: few materials, and one per triangle."""
    import numpy as np
    F = np.float32
    few = np.ascontiguousarray(tris[:, 18:36], F).copy()
    few[:, 10] = F(0.35)  # roughness
    each = few.copy()
    each[:, 3:6] = np.random.RandomState(3).uniform(0.2, 1.0, size=(few.shape[0], 3)).astype(F)  # baseColor
    each[:, 16] = np.arange(few.shape[0], dtype=F)  # IOR, not shaded: every key distinct
    return [few, each]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c5"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from opengl_ray_tracing_amd import Renderer, scenes
    if not torch.cuda.is_available():
        raise RuntimeError("material_time: no GPU visible")
    lines = []
    for name in a.configs:
        cfg, tris, nodes, hdr = scenes.build_config(name)
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 36)
        nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
        host = looks(tris)
        with Renderer(cfg.width, cfg.height, cfg.integrator, max_bounce=cfg.max_bounce) as r:
            first_upload = wall(lambda: r.upload_scene(tris, nodes))
            r.upload_env(hdr)
            dev = [torch.from_numpy(m).to("cuda:0") for m in host]
            torch.cuda.synchronize()
            fresh = []
            for m in host:
                t2 = tris.copy()
                t2[:, 18:36] = m
                fresh.append(t2)
            first_update = wall(lambda: r.update_materials(dev[1]))  # allocates the update's tables
            ms = {"host": [], "device": [], "upload": []}
            upload_stat, counts = [], {}
            for k in range(a.rounds):
                q = k % 2
                ms["host"].append(wall(lambda: r.update_materials(host[q])))
                ms["device"].append(wall(lambda: r.update_materials(dev[1 - q])))
                counts[1 - q] = r.material_count()
                ms["upload"].append(wall(lambda: r.upload_scene(fresh[q], nodes)))
                upload_stat.append(r.stats().upload_ms)
                r.update_materials(dev[q])  # untimed: the upload freed the update's tables (first_update_ms has that cost)
            breakdown = []
            for q in range(2):
                text = step_times("PT_MATERIAL_TIMES", lambda: r.update_materials(dev[q]))
                m = re.search(r"insert ([\d.]+) scan ([\d.]+) scatter ([\d.]+) ms, (\d+) materials, (\d+) slots", text)
                breakdown.append(None if not m else {
                    "insert_ms": float(m.group(1)), "scan_ms": float(m.group(2)), "scatter_ms": float(m.group(3)),
                    "materials": int(m.group(4)), "slots": int(m.group(5))})
            st = r.stats()
        line = {
            "config": name, "triangles": int(tris.shape[0]), "rounds": a.rounds,
            "first_upload_ms": round(first_upload, 3), "first_update_ms": round(first_update, 3),
            **{f"{k}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            **{f"{k}_ms_rounds": [round(x, 3) for x in v] for k, v in ms.items()},
            "upload_ms_stat_rounds": [round(x, 3) for x in upload_stat],
            "device_beats_upload": max(ms["device"]) < min(ms["upload"]),
            "host_beats_upload": max(ms["host"]) < min(ms["upload"]),
            "upload_over_device_min": round(min(ms["upload"]) / max(ms["device"]), 2),
            "materials": {("few", "each")[q]: n for q, n in sorted(counts.items())},
            "breakdown": {"few": breakdown[0], "each": breakdown[1]},
            "hw_queues_env": os.environ.get("GPU_MAX_HW_QUEUES"), "frames_in_flight": st.frames_in_flight,
            "device": torch.cuda.get_device_name(0),
        }
        emit(lines, line)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
