#!/usr/bin/env python3
"""Writes tests/golden/live_tiles/mis_rays.json: the MIS ray counts of tests/test_gpu_live_tiles.py's
cases as the regen kernel gave them when it claimed every tile (the commit before the live-item
lists). Needs a GPU.

    python tests/golden/make_live_tiles_fixture.py PACKAGE_ROOT

PACKAGE_ROOT is a built checkout of that commit (its opengl_ray_tracing_amd is imported); the cases,
the oracle and the helpers are this tree's tests. The images are checked against the oracle as in
the tests, so a count is recorded only for a run that is bit-equal to it.
"""
import json
import sys
from pathlib import Path

TESTS = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(TESTS))
sys.path.insert(0, str(Path(sys.argv[1]).resolve()))
import opengl_ray_tracing_amd  # noqa: E402

assert Path(opengl_ray_tracing_amd.__file__).resolve().parent.parent == Path(sys.argv[1]).resolve()
from opengl_ray_tracing_amd import scenes  # noqa: E402

import test_gpu_live_tiles as T  # noqa: E402

T.RECORD = {}
env = scenes.synthetic_env(64, 32)
for w, h in ((70, 45), (16, 16), (160, 32)):
    T.test_one_live_tile(env, "mis", w, h)
T.test_narrow_kernels(env, "mis", 3)
T.test_items_live_in_some_frames_only(env, "mis")
T.test_camera_move_and_scene_upload(env, "mis")
out = TESTS / "golden" / "live_tiles" / "mis_rays.json"
out.write_text(json.dumps(T.RECORD, indent=1, sort_keys=True) + "\n")
print(out, T.RECORD)
