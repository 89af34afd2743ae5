"""The leaf step's memory round trip, read from the generated code (no GPU): every leaf loop of the
regen kernels fetches its pair record (pt_trace.h pairTestT, PAIR_F4 = 7 float4) as seven 16-byte
loads from one base register at offsets 0, 16, ..., 96, issued in the loop's first block, and holds
no other load from that base.

Without pairTestT's register pin the compiler narrowed the record's loads to the dwords each path
uses and sank the first triangle's vertices behind the branch on its plane test: 20 loads in two
dependent trips per pair test. tools/leaf_loads.py compiles pt_regen.hip device-only with the
package's HIP_FLAGS and reports the loads; only their widths and offsets are looked at here.
"""
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from opengl_ray_tracing_amd import _build  # noqa: E402

pytestmark = pytest.mark.skipif(not (Path(_build.HIPCC).exists() or shutil.which("hipcc")),
                                reason="hipcc is not installed")

# regenKernel<INTEG, CULL, WAVES (0: the binary walk), WIDE, block LDS floats, FULL>
C2 = "pt::regenKernel<0, true, 4, true, 1024, true>"    # Lambert, the whole 4-wide tree in LDS: bench.py's c2
MIS_WIDE = ["pt::regenKernel<2, true, 4, true, 256, false>",  # MIS, 4-wide walk: large scenes (c5), 4 waves/SIMD
            "pt::regenKernel<2, true, 3, true, 256, false>"]  # and scenes that fit the L2s, 3 waves/SIMD
# the leaf loops of a 4-wide kernel: walk4Run's and the two reference walks' (the retrace of a tie
# or an unreachable winner, and the camera rays of a tile the camera-ray pass left to the kernel)
WIDE_LEAF_LOOPS = 3


@pytest.fixture(scope="module")
def report():
    import leaf_loads
    return leaf_loads.leaf_loads()


def check_kernel(k, name):
    for lp in k["leaf_loops"]:
        rec = lp["record_loads"]
        where = f"{name} leaf loop {lp['header']}: {rec}"
        assert [ld["bytes"] for ld in rec] == [16] * 7, where      # seven 16-byte loads, and no other from the base
        assert sorted(ld["offset"] for ld in rec) == [0, 16, 32, 48, 64, 80, 96], where
        assert {ld["block"] for ld in rec} == {lp["header"]}, where  # issued together: none behind a branch
        assert lp["one_trip"], where


@pytest.mark.parametrize("name", [C2, *MIS_WIDE])
def test_wide_kernels_fetch_the_record_in_one_trip(report, name):
    assert name in report, sorted(report)
    k = report[name]
    assert len(k["leaf_loops"]) == WIDE_LEAF_LOOPS, [lp["header"] for lp in k["leaf_loops"]]
    check_kernel(k, name)


def test_every_regen_kernel_fetches_the_record_in_one_trip(report):
    assert len(report) >= 12  # Lambert, Disney and MIS, each with its wide, binary and unculled forms
    for name, k in report.items():
        assert k["leaf_loops"], name  # every regen kernel walks a tree: a leaf loop must be found
        check_kernel(k, name)
