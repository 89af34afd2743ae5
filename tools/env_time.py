#!/usr/bin/env python3
"""What an environment update costs against the upload it replaces.

    python tools/env_time.py [peppermint san_giuseppe] [--rounds 9] [--out profiles/r19/env.json]

For each map (scenes.HDR_FILES: 1024 x 512 peppermint, 2048 x 1024 san_giuseppe) three ways of giving the
renderer a new sky of the same size are timed, each without and with a caller's table. Two maps alternate
-- the file's and the same rolled by a quarter turn, both RGBE-exact -- so every call changes the sky.
 * upload:  pt_upload_env from host arrays -- the baseline, what a caller had to do before
 * host:    pt_update_env from the same host arrays
 * device:  pt_update_env_device from tensors already on the GPU
Each is wall time of the synchronous call after a warm-up call of the same kind and size, reported as the
median and min ... max over the rounds (measure in one process, interleaved: the rounds alternate the
three ways, so drift hits all alike).
 * steps: one more device update of each kind with PT_UPDATE_TIMES set: device time (HIP events) of the
   texel pack, the library's table, the compact forms, Env::light and the rows.
On a library without pt_update_env (the parent commit) only the upload is timed: that is the figure the
update is compared with. One JSON line per map.
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from update_common import emit, step_times, wall, write_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("maps", nargs="*", default=["peppermint", "san_giuseppe"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from opengl_ray_tracing_amd import Renderer, calculate_hdr_cache, load_hdr, scenes
    if not torch.cuda.is_available():
        raise RuntimeError("env_time: no GPU visible")
    lines = []
    for name in a.maps:
        first = np.ascontiguousarray(load_hdr(scenes.HDR_FILES[name]), np.float32)
        h, w = first.shape[:2]
        host = [first, np.ascontiguousarray(np.roll(first, w // 4, axis=1))]
        table = [calculate_hdr_cache(m) for m in host]
        with Renderer(64, 64, "mis") as r:
            has_update = hasattr(r, "update_env")

            ways = {"upload": lambda q: r.upload_env(host[q]), "upload_table": lambda q: r.upload_env(host[q], table[q])}
            if has_update:
                dev = [torch.from_numpy(m).to("cuda:0") for m in host]
                dtab = [torch.from_numpy(t).to("cuda:0") for t in table]
                torch.cuda.synchronize()
                ways.update({"host": lambda q: r.update_env(host[q]), "host_table": lambda q: r.update_env(host[q], table[q]),
                             "device": lambda q: r.update_env(dev[q]), "device_table": lambda q: r.update_env(dev[q], dtab[q])})
            ms = {k: [] for k in ways}
            compact = {}
            for k in range(a.rounds):
                for way, fn in ways.items():
                    fn(k % 2)  # the warm-up of this kind and size: an upload before it freed the update's buffers
                    ms[way].append(wall(lambda: fn(1 - k % 2)))
                    compact[way] = r.stats().env_compact
            steps = {}
            if has_update:
                for way in ("device", "device_table"):
                    ways[way](0)
                    text = step_times("PT_UPDATE_TIMES", lambda: ways[way](1))
                    m = re.search(r"texels ([\d.]+) table ([\d.]+) compact ([\d.]+) light ([\d.]+) rows ([\d.]+) ms, env_compact (\d), (\d+) rows", text)
                    steps[way] = None if not m else {
                        "texels_ms": float(m.group(1)), "table_ms": float(m.group(2)), "compact_ms": float(m.group(3)),
                        "light_ms": float(m.group(4)), "rows_ms": float(m.group(5)), "distinct_rows": int(m.group(7))}
        line = {
            "map": name, "w": w, "h": h, "rounds": a.rounds, "has_update": has_update,
            **{f"{k}_ms_median": round(statistics.median(v), 3) for k, v in ms.items()},
            **{f"{k}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            **{f"{k}_ms_rounds": [round(x, 3) for x in v] for k, v in ms.items()},
            "env_compact": compact, "steps": steps,
            "hw_queues_env": os.environ.get("GPU_MAX_HW_QUEUES"), "device": torch.cuda.get_device_name(0),
        }
        if has_update:
            line["upload_over_device"] = round(statistics.median(ms["upload"]) / statistics.median(ms["device"]), 2)
            line["upload_table_over_device_table"] = round(statistics.median(ms["upload_table"]) / statistics.median(ms["device_table"]), 2)
        emit(lines, line)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
