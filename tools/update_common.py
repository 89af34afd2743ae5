"""What tools/update_time.py, material_time.py and env_time.py share: the wall time of a synchronous
call, the library's step-time line caught off stderr, and the JSON-lines output."""
from __future__ import annotations

import json
import os
import sys
import tempfile
import time
from pathlib import Path


def wall(fn):
    """Wall time of fn() in ms."""
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def captured_stderr(fn):
    """fn() with the process's stderr (the library writes there) into a string."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def step_times(switch, fn):
    """What the library writes to stderr during fn() with the environment switch (PT_UPDATE_TIMES,
    PT_MATERIAL_TIMES) set for that call alone."""
    os.environ[switch] = "1"
    try:
        return captured_stderr(fn)
    finally:
        del os.environ[switch]


def emit(lines, line):
    """One JSON line per config or map, printed as it comes."""
    print(json.dumps(line), flush=True)
    lines.append(line)


def write_lines(out, lines):
    """... and all of them written to `out`, if any, at the end."""
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text("".join(json.dumps(x) + "\n" for x in lines))
