"""The host side of the moments gather of a screen-tile split (PT_FLAG_SHARE_MOMENTS), no GPU: the
numpy pack / unpack with the 5-channel slots of pt_pack_owned_stats, and the property the design
rests on -- every 8x8 tile of the image lies in one rank's shard tiles, so each rank can decide its
own tiles and the ranks' tile planes have disjoint support."""
import numpy as np
import pytest

from opengl_ray_tracing_amd import distributed as D

SIZES = [(33, 31), (100, 76)]
WORLDS = [2, 3, 8]
SHARDS = [8, 16, 32]


def owner_of_pixels(w, h, world, shard):
    """(h, w) int: the rank whose packed slots hold each pixel; every pixel exactly once."""
    own = np.full((h, w), -1, np.int64)
    seen = np.zeros((h, w), np.int64)
    for k in range(world):
        p = D.owned_pixels(w, h, k, world, shard)
        own[p[:, 1], p[:, 0]] = k
        seen[p[:, 1], p[:, 0]] += 1
    assert np.all(seen == 1)
    return own


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("world", WORLDS)
def test_five_channel_pack_round_trip(w, h, world):
    rng = np.random.default_rng(w * 131 + world)
    stats = rng.random((h, w, 5), np.float32)  # r, g, b, m1, m2
    out = np.zeros_like(stats)
    slots = 0
    for k in range(world):
        packed = D.pack(stats, k, world)
        assert packed.shape == (D.packed_count(w, h, k, world), 5) and packed.dtype == np.float32
        px, py, valid = D.packed_coords(w, h, k, world)
        assert not packed[~valid].any()  # a slot outside the image is zeros
        assert np.array_equal(packed[valid], stats[py[valid], px[valid]])
        D.unpack(out, packed, k, world)
        slots += int(valid.sum())
    assert slots == w * h
    assert np.array_equal(out.view(np.uint32), stats.view(np.uint32))
    if world == 3 and (w, h) == (33, 31):  # two shard tiles, three ranks: the last owns nothing
        assert D.packed_count(w, h, 2, world) == 0 and D.pack(stats, 2, world).shape == (0, 5)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shard", SHARDS)
def test_owned_image_tiles_partition_the_tiles(w, h, world, shard):
    tiles_y, tiles_x = (h + 7) // 8, (w + 7) // 8
    masks = [D.owned_image_tiles(w, h, k, world, shard) for k in range(world)]
    assert all(m.shape == (tiles_y, tiles_x) and m.dtype == bool for m in masks)
    assert sum(int(m.sum()) for m in masks) == tiles_x * tiles_y
    assert np.all(np.sum(masks, axis=0) == 1)
    for k, m in enumerate(masks):  # a rank past the last shard tile owns no tile
        if D.packed_count(w, h, k, world, shard) == 0:
            assert not m.any()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shard", SHARDS)
def test_every_8x8_tile_has_one_owner(w, h, world, shard):
    own = owner_of_pixels(w, h, world, shard)
    tiles_y, tiles_x = (h + 7) // 8, (w + 7) // 8
    masks = [D.owned_image_tiles(w, h, k, world, shard) for k in range(world)]
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            ranks = np.unique(own[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8])  # clipped at the image's edge
            assert ranks.size == 1, (tx, ty, ranks)
            assert masks[int(ranks[0])][ty, tx]
