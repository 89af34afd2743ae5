"""The screen-tile share as the frame kernels compute it (csrc/pt_frame.h: ownedShards, slots,
tileOrigin, slotOf, pixelOfSlot), printed by tests/native/share_table.cpp -- a host-only program: no
device, no HIP library -- against distributed.packed_coords, numpy's independent statement of the
packed order. Sizes that are no multiple of any tile, one-pixel images, every tile_size the ABI is
used with, and every rank of worlds 1, 2, 3 and 8, ranks that own nothing included.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from opengl_ray_tracing_amd import _build, distributed

SIZES = [(1, 1), (8, 8), (33, 31), (70, 45), (160, 90)]
TILES = [8, 16, 32]
WORLDS = [1, 2, 3, 8]


@pytest.fixture(scope="module")
def cases():
    raw = subprocess.run([str(_build.build_share_table())], capture_output=True, check=True).stdout
    w = np.frombuffer(raw, np.int32)
    out, at = {}, 0
    while at < w.size:
        width, height, tile, world, rank, owned, slots, tiles = (int(v) for v in w[at:at + 8])
        at += 8
        px, py, inside, back = w[at:at + 4 * slots].reshape(slots, 4).T
        at += 4 * slots
        origin = w[at:at + 2 * tiles].reshape(tiles, 2)
        at += 2 * tiles
        out[(width, height, tile, world, rank)] = dict(owned=owned, slots=slots, tiles=tiles, px=px, py=py,
                                                       inside=inside.astype(bool), back=back, origin=origin)
    return out


def test_every_case_is_in_the_table(cases):
    want = {(w, h, t, n, r) for w, h in SIZES for t in TILES for n in WORLDS for r in range(n)}
    assert set(cases) == want
    assert any(c["owned"] == 0 for c in cases.values()), "some rank of some world owns nothing"


def test_counts(cases):
    for (w, h, t, n, r), c in cases.items():
        owned = distributed.owned_tiles(w, h, r, n, t).size
        assert c["owned"] == owned, (w, h, t, n, r)
        num_items = owned * (t // 8) ** 2  # pt_create's wave tiles of the rank
        assert c["tiles"] == num_items, (w, h, t, n, r)
        assert c["slots"] == num_items * 64 == owned * t * t, (w, h, t, n, r)


def test_pixel_of_slot_is_the_packed_order(cases):
    for (w, h, t, n, r), c in cases.items():
        px, py, valid = distributed.packed_coords(w, h, r, n, t)
        assert np.array_equal(c["px"], px) and np.array_equal(c["py"], py), (w, h, t, n, r)
        assert np.array_equal(c["inside"], valid), (w, h, t, n, r)


def test_slot_of_inverts_pixel_of_slot(cases):
    for key, c in cases.items():
        k = np.arange(c["slots"])
        assert np.array_equal(c["back"][c["inside"]], k[c["inside"]]), key


def test_wave_tiles_of_all_ranks_cover_the_image_once(cases):
    lane = np.arange(64)
    for w, h in SIZES:
        for t in TILES:
            for n in WORLDS:
                seen = np.zeros((h, w), np.int32)
                for r in range(n):
                    o = cases[(w, h, t, n, r)]["origin"]
                    px = (o[:, :1] + (lane & 7)[None]).ravel()
                    py = (o[:, 1:] + (lane >> 3)[None]).ravel()
                    assert (px >= 0).all() and (py >= 0).all()
                    inside = (px < w) & (py < h)
                    np.add.at(seen, (py[inside], px[inside]), 1)
                assert (seen == 1).all(), (w, h, t, n)


def test_wave_tile_k_holds_slots_of_one_shard_tile(cases):
    """Wave tile w's pixels are slots of shard tile w // (tile/8)^2 of the share: what lets the
    camera-ray pass index its per-tile results by wave tile and the colour buffer by slot."""
    lane = np.arange(64)
    for (w, h, t, n, r), c in cases.items():
        if not c["tiles"]:
            continue
        per = (t // 8) ** 2
        o = c["origin"]
        px = o[:, :1] + (lane & 7)[None]
        py = o[:, 1:] + (lane >> 3)[None]
        slot_px = c["px"].reshape(-1, t * t)
        j = np.arange(c["tiles"]) // per
        x0, y0 = slot_px[j, 0], c["py"].reshape(-1, t * t)[j, 0]  # the shard tile's first pixel
        assert ((px >= x0[:, None]) & (px < x0[:, None] + t)).all(), (w, h, t, n, r)
        assert ((py >= y0[:, None]) & (py < y0[:, None] + t)).all(), (w, h, t, n, r)
