#!/usr/bin/env python3
"""Writes tests/golden/sky_tiles/mis_rays.json: the MIS ray counts of tests/test_gpu_sky_tiles.py's cases
as the commit before the update shaded the all-sky tiles gave them (its camera-ray pass visited every
tile). Needs a GPU.

    python tests/golden/make_sky_tiles_fixture.py PACKAGE_ROOT

PACKAGE_ROOT is a built checkout of that commit (its opengl_ray_tracing_amd is imported); the cases, the
oracle and the helpers are this tree's tests. The images are checked against the oracle as in the tests,
so a count is recorded only for a run that is bit-equal to it.
"""
import json
import sys
from pathlib import Path

TESTS = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(TESTS))
sys.path.insert(0, str(Path(sys.argv[1]).resolve()))
import opengl_ray_tracing_amd  # noqa: E402

assert Path(opengl_ray_tracing_amd.__file__).resolve().parent.parent == Path(sys.argv[1]).resolve()
from opengl_ray_tracing_amd import FLAG_MEGAKERNEL, FLAG_PRIMARY_PASS, FLAG_REGEN, scenes  # noqa: E402

import test_gpu_sky_tiles as T  # noqa: E402

T.RECORD = {}
env = scenes.synthetic_env(64, 32)
for w, h in ((70, 45), (16, 16), (160, 32)):
    for off in (2.3, 0.6):
        T.test_one_pass_tile(env, "mis", off, w, h)
T.test_other_kernels_behind_a_pass(env, "mis", 8, FLAG_MEGAKERNEL | FLAG_PRIMARY_PASS)
T.test_other_kernels_behind_a_pass(env, "mis", 3, FLAG_REGEN | FLAG_PRIMARY_PASS)
out = TESTS / "golden" / "sky_tiles" / "mis_rays.json"
out.parent.mkdir(exist_ok=True)
out.write_text(json.dumps(T.RECORD, indent=1, sort_keys=True) + "\n")
print(out, T.RECORD)
