"""bench.py's plain run (N = 1, no --full): the timed steps only -- the line carries the headline
figures and no other leg's, --steps sets the timed frames, and --dump-outputs writes the running
means the timed steps left (one progressive frame per step, OpenglRayTracing/main.cpp:558-603)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_prints_the_line_and_dumps_the_running_means(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "dump")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = the timed steps' rays over their wall time: at least one primary ray per pixel per step
    w, h = map(int, d["config"]["resolution"].split("x"))
    assert d["value"] * 1e6 * d["ms_per_step"] * 1e-3 >= 0.999 * w * h
    # no other leg ran
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["quality"] is None
    assert d["reset_ms_per_frame"] is None and "per_call" not in d
    files = sorted(p.name for p in (tmp_path / "dump").iterdir())
    assert files == ["accum.npy"]
    a = np.load(tmp_path / "dump" / "accum.npy")
    assert a.dtype == np.float32 and a.shape == (h, w, 4) and a.nbytes <= 64 * 10 ** 6
    assert np.isfinite(a).all() and (a[..., 3] == 1.0).all() and a[..., :3].max() > 0
