"""tests/material_looks.py, the inputs of the pt_update_materials tests, on the CPU alone: the looks
do what they claim on the oracle, their tables have the sizes claimed, and the four new symbols of the
C ABI exist and refuse NULL arguments (loading the library needs no GPU, as in tests/test_abi.py).
tests/native/material_table_check.cpp runs the library's own table function -- pt_scene_prep.cpp
materialTable, which prepareScene numbers an upload's materials by -- on every look and must agree with
material_scene.table_ids.
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import material_looks as ml
import material_scene as ms
from opengl_ray_tracing_amd import _build, _native

F = np.float32
ROOT = Path(__file__).resolve().parent.parent
INVALID = -1


def test_every_look_changes_the_image():
    base = ml.oracle_frames("material", 0, "mis", 2, 1)[0][0]
    assert np.isfinite(base).all()
    for k in ml.LOOKS[1:]:
        img = ml.oracle_frames("material", k, "mis", 2, 1)[0][0]
        assert np.isfinite(img).all(), k
        changed = (img.view(np.uint32) != base.view(np.uint32)).any(-1).mean()
        print(f"look {k}: {changed:.3f} of the pixels differ from look 0")
        assert changed > 0.01, k


def test_the_distinct_c2x3_materials_change_the_image():
    a = ml.oracle_frames("c2x3", 0, "lambert", 2, 1)[0][0]
    b = ml.oracle_frames("c2x3", 1, "lambert", 2, 1)[0][0]
    assert (a.view(np.uint32) != b.view(np.uint32)).any(-1).mean() > 0.05


def test_table_sizes():
    tris = ms.build()[0]
    assert tris.shape[0] == 1173
    for k, size in ml.SIZES.items():
        table, ids = ml.expected(ml.look(k))
        assert table.shape == (size, 18) and ids.max() == size - 1, k
    # look 1: the same keys as look 0 in another order
    t0, t1 = ml.expected(ml.look(0))[0], ml.expected(ml.look(1))[0]
    assert not ml.same_bits(t0, t1)
    assert sorted(r.tobytes() for r in t0) == sorted(r.tobytes() for r in t1)
    # look 4 merges the pair that differed in emission only
    assert ml.expected(ml.look(4))[0].shape[0] == ms.N_PALETTE - 1
    n = ml.scene_arrays("c2x3")[0].shape[0]
    assert n == 15004 and ml.expected(ml.c2x3_distinct())[0].shape[0] == n


def test_look_5_tail():
    m = ml.look(5)
    n = m.shape[0]
    w = m.view(np.uint32)
    table, ids = ml.expected(m)
    a = n - ml.TAIL
    assert (w[a] != w[a + 1]).sum() == 1 and w[a, 17] ^ w[a + 1, 17] == 1 and ids[a] != ids[a + 1]
    assert m[a + 2, ml.SHEEN] == m[a + 3, ml.SHEEN] == 0 and ids[a + 2] != ids[a + 3]  # equal as floats, not as bits
    assert np.isnan(m[a + 4:a + 7, ms.IOR]).all()
    assert ids[a + 4] == ids[a + 5] != ids[a + 6]                                       # the NaN keys split 2 + 1
    assert ids[n - 1] == ids[0] == 0
    assert table.shape[0] == ids.max() + 1 and ml.same_bits(table[ids], m)


def test_expected_restates_table_ids():
    tris = ms.build()[0]
    table, ids = ml.expected(ml.look(0))
    assert np.array_equal(ids, ms.table_ids(tris)) and ml.same_bits(table[ids], tris[:, 18:36])


def test_abi_symbols_and_null_arguments():
    lib = _native.load()
    for name in ("pt_update_materials", "pt_update_materials_device", "pt_material_count", "pt_download_materials"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    m = np.zeros((4, 18), F)
    fp = m.ctypes.data_as(_native.c_float_p)
    n = C.c_int(0)
    ids = np.zeros(4, np.int32)
    assert lib.pt_update_materials(None, fp, 4, 18) == INVALID
    assert lib.pt_update_materials_device(None, C.c_void_p(m.ctypes.data), 4, 18) == INVALID
    assert lib.pt_material_count(None, C.byref(n)) == INVALID
    assert lib.pt_download_materials(None, fp, 4, ids.ctypes.data_as(_native.c_int_p)) == INVALID


def test_library_table_function_agrees(tmp_path):
    """pt_scene_prep.cpp materialTable on every look, strides 18 and 36."""
    exe = _build.build_material_table_check()
    for k in ml.LOOKS:
        for stride in (18, 36):
            m = ml.look(k)
            rec = m if stride == 18 else ml.tris_of(np.full((m.shape[0], 36), 7.0, F), m)
            path = tmp_path / f"look{k}_{stride}.bin"
            np.ascontiguousarray(rec, F).tofile(path)
            out = subprocess.run([str(exe), str(path), str(m.shape[0]), str(stride)], capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, out.stderr
            rows = [list(map(int, line.split())) for line in out.stdout.splitlines()]
            table, ids = ml.expected(m)
            assert rows[0] == [table.shape[0]], (k, stride)
            assert np.array_equal(np.array(rows[1], np.int32), ids), (k, stride)
            assert np.array_equal(np.array(rows[2]), np.unique(ids, return_index=True)[1]), (k, stride)
