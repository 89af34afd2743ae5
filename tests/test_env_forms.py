"""The view of the environment's store that the kernels get (opengl_ray_tracing_amd/csrc/pt_envupdate.h:
envForms, the one place the view is written, and compactLevel, pt_frame_stats.env_compact) for stores
filled by hand -- tests/native/env_forms_table.cpp, a host-only program: no device, no HIP library.

The expected values were read off pt_update_env's hand-over as it stood before the view became a
function (pt_env.cpp updateEnvOne: compact = hdr8 && !bad, rows = compact && cacheRow && !rowsBad; trig
with compact, light with compact and trig, cacheRow and cacheY with rows), not taken from the program.
A store's buffers are the integers 1..8 in the order of FIELDS; 0 is a null pointer.
"""
import subprocess

import pytest

from opengl_ray_tracing_amd import _build

FIELDS = ("hdr", "cache", "hdr8", "cache4", "cacheRow", "cacheY", "trig", "light")
FLOAT_ONLY = (1, 2, 0, 0, 0, 0, 0, 0)

# case: (the eight pointers, (w, h), env_compact)
CASES = {
    "no_compact": (FLOAT_ONLY, (37, 19), 0),                  # no compact buffers
    "no_compact_rest_allocated": (FLOAT_ONLY, (37, 19), 0),   # ... whatever else is allocated
    "compact_bad": (FLOAT_ONLY, (37, 19), 0),                 # compact buffers, not exact: trig, light and rows null too
    "compact_bad_rows_bad": (FLOAT_ONLY, (37, 19), 0),
    "rows_bad": ((1, 2, 3, 4, 0, 0, 7, 8), (37, 19), 1),      # compact exact, rows not
    "exact": ((1, 2, 3, 4, 5, 6, 7, 8), (37, 19), 2),
    "no_trig": ((1, 2, 3, 4, 5, 6, 0, 0), (37, 19), 2),       # light is null without trig, though allocated
    "no_light": ((1, 2, 3, 4, 5, 6, 7, 0), (37, 19), 2),
    "no_cache_row": ((1, 2, 3, 4, 0, 0, 7, 8), (37, 19), 1),  # no cacheRow: cacheY null too, level at most 1
    "upload_exact": ((1, 2, 3, 4, 5, 6, 7, 8), (37, 19), 2),  # an upload's store: the same view
    "empty": ((0,) * 8, (0, 0), 0),
    "empty_flags_bad": ((0,) * 8, (0, 0), 0),
}


@pytest.fixture(scope="module")
def table():
    out = subprocess.run([str(_build.build_env_forms_table())], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        name, *fields = line.split()
        rows[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return rows


def test_every_case_is_printed_once(table):
    assert sorted(table) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_view_of_a_store(table, name):
    ptrs, (w, h), level = CASES[name]
    got = table[name]
    assert tuple(got[f] for f in FIELDS) == ptrs, (name, got)
    assert (got["w"], got["h"]) == (w, h), (name, got)
    assert got["level"] == level, (name, got)
