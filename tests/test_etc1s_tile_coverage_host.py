"""That the generated inputs of the ETC1S kernel parity tests (helpers.etc1s_planted_tiles, etc1s_spread_ladder, clusters_by_plant) reach what they were made to reach:
every intensity table as the winner of the per-block and of the cluster fit, winners that clamp low, high and at both ends, fits that end early with error 0 at different
trial depths, and every index of the per-spread table mask. CPU only, and the oracle only: the conditions are on the INPUTS, so a failure here is mended in the generators,
never in the thresholds. The figures in brackets are what the generators give today.
"""
import numpy as np
import pytest

import helpers as H
from helpers import oracle, ptr, u32p, u64p

BLOCK_FITS = [(0, 0), (1, 1), (1, 0), (2, 1), (2, 0), (6, 1), (6, 0)]   # (level, perceptual)


@pytest.fixture(scope="module")
def planted():
    return H.etc1s_planted_tiles()


@pytest.fixture(scope="module")
def block_fits(planted):
    """per (level, perceptual): winning table, clamp class of the winning endpoint, decoded-back-exactly flag of every planted tile"""
    tiles, _ = planted
    n = tiles.shape[0]
    out = {}
    for level, perceptual in BLOCK_FITS:
        enc = H.orc_encode_blocks(tiles, level, perceptual)
        color5, table = enc[:, :3] >> 3, enc[:, 3] >> 5
        assert (table == ((enc[:, 3] >> 2) & 7)).all()
        dec = H.decode_etc1s_blocks(enc, n, 1).reshape(4, n, 4, 3).transpose(1, 0, 2, 3)
        out[level, perceptual] = (table, H.etc1s_clamp_class(color5, table), (dec == tiles[..., :3]).reshape(n, -1).all(axis=1))
    return out


def test_planted_tiles_are_what_they_say(planted):
    tiles, meta = planted
    n = tiles.shape[0]
    assert tiles.shape == (n, 4, 4, 4) and tiles.dtype == np.uint8 and meta.shape == (n,) and (tiles[..., 3] == 255).all()
    n_ep = int(meta["endpoint"].max()) + 1
    assert n_ep == 198 and n == 198 * H.PLANT_TILES_PER_ENDPOINT   # 8 tables x 5 classes x 6, less `inside` of table 7 and `both` of tables 0-5
    assert (np.bincount(meta["endpoint"]) == H.PLANT_TILES_PER_ENDPOINT).all()
    assert (np.diff(meta["table"].astype(int) * 8 + meta["cls"]) >= 0).all()   # ordered by (table, class)
    # the class recorded is the class of the planted endpoint, and the noise-free tiles are made of its four colours alone, all four of them
    want = {"inside": 0, "low": 1, "high": 2, "both": 3, "split": 3}
    assert (H.etc1s_clamp_class(meta["color5"], meta["table"]) == np.array([want[H.PLANT_CLASSES[c]] for c in meta["cls"]])).all()
    base = (meta["color5"].astype(np.int32) << 3) | (meta["color5"] >> 2)
    colours = np.clip(base[:, None, :] + H.ETC1_INTEN_TABLES[meta["table"]][:, :, None], 0, 255)           # (n, 4, 3)
    px = tiles[..., :3].reshape(n, 16, 3).astype(np.int32)
    dist = np.abs(px[:, :, None, :] - colours[:, None, :, :]).max(axis=3).min(axis=2)                       # per texel, to the nearest planted colour
    assert (dist.max(axis=1) <= meta["noise"]).all() and (meta["noise"] == 0).sum() == n // 2
    span = base.max(axis=1) - base.min(axis=1)
    assert (span[meta["cls"] == H.PLANT_CLASSES.index("both")] < 60).all() and (span[meta["cls"] == H.PLANT_CLASSES.index("split")] >= 120).all()
    again, _ = H._planted_tiles.__wrapped__()
    assert (again == tiles).all()   # seeded


def test_every_table_wins_the_block_fit(block_fits):
    for key, (table, _, _) in block_fits.items():
        wins = np.bincount(table, minlength=8)
        print(key, "winners per table", wins.tolist())
        assert wins.min() >= 100, (key, wins.tolist())   # [190, table 7 at level 0]


def test_winners_of_every_clamp_class(block_fits):
    for key, (_, cls, _) in block_fits.items():
        count = np.bincount(cls, minlength=4)
        print(key, "winners that clamp nowhere / low / high / at both ends", count.tolist())
        assert count[1:].min() >= 200, (key, count.tolist())   # [561]


def test_zero_error_tiles_at_different_trial_depths(block_fits):
    zero = {key: int(z.sum()) for key, (_, _, z) in block_fits.items()}
    print("tiles decoded back exactly", zero)
    assert min(zero.values()) >= 200   # [512, at level 0]
    for perceptual in (1, 0):
        assert zero[6, perceptual] > zero[1, perceptual]   # [1131 vs 646, 1126 vs 642]: trials past level 1's sixteen end early too


def test_every_table_wins_the_cluster_fit(planted):
    tiles, meta = planted
    lists, block_cluster = H.clusters_by_plant(meta)
    assert len(lists) == 198 and all(l.size == 2 * H.PLANT_TILES_PER_ENDPOINT for l in lists) and (block_cluster == meta["endpoint"]).all()
    exact = H.planted_exact_clusters(meta)
    for l in exact:   # noise-free tiles of one endpoint
        assert l.size == 4 and (meta["noise"][l >> 1] == 0).all() and np.unique(meta["endpoint"][l >> 1]).size == 1
    k = len(lists) + len(exact)
    offs, idx = H.csr_from_lists(lists + exact)
    for level in (1, 2, 6):
        for perceptual in (1, 0):
            params = np.zeros((k, 4), np.uint8); err = np.zeros(k, np.uint64); valid = np.zeros(k, np.uint8)
            oracle().orc_generate_endpoint_codebook(ptr(tiles), k, ptr(offs, u32p), ptr(idx, u32p), level, perceptual, 0, ptr(params), ptr(err, u64p), ptr(valid))
            wins = np.bincount(params[:len(lists), 3], minlength=8)
            exact_zero = int((err[len(lists):] == 0).sum())
            print((level, perceptual), "clusters per winning table", wins.tolist(), "zero-error clusters", exact_zero, "of", len(exact))
            assert valid.all()
            assert wins.min() >= 15, (level, perceptual, wins.tolist())   # [22]
            assert exact_zero >= 8, (level, perceptual, exact_zero)


def test_ladder_reaches_every_spread():
    tiles = H.etc1s_spread_ladder()
    assert tiles.shape == (768, 4, 4, 4) and tiles.dtype == np.uint8 and (tiles[..., 3] == 255).all()
    px = tiles[..., :3].reshape(768, 16, 3).astype(np.int32)
    span = px.max(axis=1) - px.min(axis=1)                    # (768, 3)
    s, c = np.repeat(np.arange(256), 3), np.tile(np.arange(3), 256)
    assert (span[np.arange(768), c] == s).all() and (span.max(axis=1) == s).all()   # the carrying channel spans exactly s, the others no more
    assert (np.bincount(span.max(axis=1), minlength=256) == 3).all()
    assert (H.etc1s_spread_ladder.__wrapped__() == tiles).all()   # seeded
    both = H.etc1s_planted_test_tiles()
    assert both.shape[0] == 3144 and (both[-768:] == tiles).all()
