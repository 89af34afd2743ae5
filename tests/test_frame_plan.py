"""The frame path's launch policy (opengl_ray_tracing_amd/csrc/pt_plan.h: planFrame, batchFor,
pipeDepthFor) on contexts filled by hand -- tests/native/plan_table.cpp, a host-only program: no
device, no HIP library. The expected values were read off the frame path before the policy moved
into pt_plan.h (pt_runtime.cpp's createOne, uploadScene and renderOne), not taken from the program.

Unless a case says otherwise: the regen default (PT_REGEN_WIDE unset), both runtime trees built, a
small scene, env 1024 x 512, 1920 x 1080, tile_world 1, no flags, 4 frames wanted while other
launches are in flight.
"""
import subprocess

import pytest

from opengl_ray_tracing_amd import _build

# case: (regen, wide, walk4, pass, bins, ordered, oneCall), further fields
PLANS = {
    1: ((1, 1, 1, 1, 1, 0, 0), {"rowTable": 0, "envNt": 0}),   # Lambert, 12 frames wanted, solo
    2: ((0, 0, 0, 0, 1, 1, 1), {}),                             # Lambert, one frame, solo: the megakernel
    3: ((1, 1, 1, 1, 1, 0, 0), {}),                             # Lambert, one frame, others in flight
    4: ((1, 1, 1, 1, 1, 0, 1), {}),                             # Lambert, FLAG_REGEN, one frame, solo
    5: ((0, 0, 0, 0, 1, 1, 0), {}),                             # Disney, 16 frames
    6: ((1, 0, 0, 0, 0, 0, 0), {}),                             # Disney, FLAG_REGEN: the narrow kernel, no pass, no bins
    7: ((1, 0, 0, 1, 1, 0, 0), {}),                             # Disney, FLAG_REGEN | FLAG_PRIMARY_PASS
    8: ((1, 1, 1, 1, 1, 0, 0), {}),                             # MIS at its shader's 2 bounces, 16 frames
    9: ((0, 0, 0, 0, 1, 1, 0), {"rowTable": 1}),                # MIS, 8 bounces, env 2048 x 1024
    90: ((0, 0, 0, 0, 1, 1, 0), {"rowTable": 0}),               # ... env 1024 x 512
    10: ((1, 1, 1, 1, 1, 0, 0), {"envNt": 1, "wideScene": 1}),  # MIS, large scene, one frame, solo
    11: ((0, 1, 1, 0, 1, 1, 0), {}),                            # ... FLAG_MEGAKERNEL
    12: ((1, 1, 0, 1, 1, 0, 0), {}),                            # ... FLAG_REFERENCE_TREE
    13: ((1, 1, 1, 1, 1, 0, 0), {"wideScene": 0, "envNt": 1}),  # Lambert, large scene, one frame, solo
    14: ((0, 0, 0, 0, 0, 0, 0), {"piped": 0}),                  # Lambert, FLAG_COUNT_FETCHES | FLAG_REGEN
    15: ((0, 0, 0, 0, 1, 1, 0), {}),                            # Lambert, FLAG_NO_CULL
    16: ((1, 1, 1, 1, 1, 0, 0), {}),                            # Disney, PT_REGEN_WIDE = 1, one frame, solo
    17: ((0, 0, 0, 0, 1, 1, 0), {}),                            # Lambert, PT_REGEN_WIDE = 0
    18: ((1, 1, 1, 1, 1, 0, 0), {"piped": 0}),                  # Lambert, FLAG_SERIAL_FRAMES
    19: ((1, 1, 1, 1, 0, 0, 0), {}),                            # Lambert, FLAG_NO_BINS, 12 frames
    20: ((0, 0, 0, 0, 0, 1, 0), {}),                            # MIS, 8 bounces, no runtime tree
}
PLAN_FIELDS = ("regen", "wide", "walk4", "pass", "bins", "ordered", "oneCall")

# frames per launch at a pipe depth <= 3, and above (test_frame_batches_equal_serial_frames asserts
# the small scenes' on the GPU): times tile_world, at most 32; pt_config.frame_batch overrides
BATCHES = {
    "lambert": (12, 2), "mis2": (16, 4), "mis8": (32, 4), "disney": (16, 4),
    "large_disney": (2, 1), "large_mis": (2, 1),
    "lambert_world8": (32, 16), "mis8_world2": (32, 8), "frame_batch5": (5, 5),
}

# (context, hardware queues): frames in flight
DEPTHS = {("lambert", 12): 6, ("lambert", 4): 2, ("mis", 12): 8, ("lambert_world8", 12): 8,
          ("lambert_regenwide0", 12): 8}


@pytest.fixture(scope="module")
def table():
    out = subprocess.run([str(_build.build_plan_table())], capture_output=True, text=True, check=True).stdout
    rows = {"plan": {}, "batch": {}, "depth": {}}
    for line in out.splitlines():
        kind, *w = line.split()
        if kind == "plan":
            rows["plan"][int(w[0])] = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        elif kind == "batch":
            rows["batch"][w[0]] = (int(w[1]), int(w[2]))
        else:
            rows["depth"][(w[0], int(w[1]))] = int(w[2])
    return rows


@pytest.mark.parametrize("case", sorted(PLANS))
def test_plan_frame(table, case):
    got = table["plan"][case]
    main, more = PLANS[case]
    want = {**dict(zip(PLAN_FIELDS, main)), **more}
    assert {k: got[k] for k in want} == want
    # what every case implies: no kernel variant without its kernel, no lists without a pass
    assert got["walk4"] <= got["wide"] and got["count"] + got["cull"] <= 1


def test_plan_covers_every_case(table):
    assert sorted(table["plan"]) == sorted(PLANS)
    assert table["batch"].keys() == BATCHES.keys() and table["depth"].keys() == DEPTHS.keys()


def test_batch_for(table):
    assert table["batch"] == BATCHES


def test_pipe_depth_for(table):
    assert table["depth"] == DEPTHS
