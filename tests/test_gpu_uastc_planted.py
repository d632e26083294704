"""-m gpu parity tests of the UASTC encoder and RDO kernels on tiles planted in every mode, partition pattern and dual-plane selector
(tests/uastc_planted.py; known answers of the reference in tests/golden/uastc_planted_vectors.npz).

The host build of uastc_core.h / uastc_rdo.h equals that file (test_uastc_planted_host.py), so what is under test here is the DEVICE build of the same source: the
partition and anchor tables as the kernels read them, the per-job staging of the least-squares rows in LDS, the selector rotations of the dual-plane jobs, the order
the finish kernel takes the blocks in, and with it the form of the ETC1 hint search a wave takes (uastc_core.h, BU_WAVE_ALL: the short form only where all 64 lanes
can; the host decides per block). All comparisons are bit-exact; a failure names the cells (mode, pattern, selector) of the differing blocks.
"""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import helpers
import uastc_planted as P
from basis_universal_amd import uastc
from test_gpu_uastc_rdo import params, strips_of

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
OLD_GOLDEN = ROOT / "tests" / "golden" / "uastc_reference_vectors.npz"
GUARD = 256


@pytest.fixture(scope="module")
def planted():
    return P.load()[0]


@pytest.fixture(scope="module")
def old_vectors():
    return np.load(OLD_GOLDEN)


def assert_blocks(got, want, what, planted_in=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), f"{what}: {P.describe_differences(got, want, planted_in)}"


@pytest.mark.parametrize("name,fam,flags,step", P.encoder_arrays(), ids=[a[0] for a in P.encoder_arrays()])
def test_family_equals_reference(hip_ctx, planted, name, fam, flags, step):
    tiles = np.ascontiguousarray(planted[f"{fam}_tiles"][::step])
    assert_blocks(uastc.encode_uastc_blocks(hip_ctx, tiles, flags), planted[name], name, P.planted_cells()[::step])


@pytest.mark.parametrize("mode", [m for m in range(19) if m != 8])
def test_one_mode_per_call(hip_ctx, planted, mode):
    """The tiles planted in one mode, of all four families, on their own at level 3: 24 tiles for a mode of one cell (a partial wave, every job's grid one workgroup),
    720 for a mode of 30 patterns; the waves of the finish kernel hold tiles of one mode only."""
    pick = np.flatnonzero(np.array([c[0] for c in P.planted_cells()]) == mode)
    tiles = np.ascontiguousarray(np.concatenate([planted[f"{fam}_tiles"][pick] for fam in P.FAMILIES]))
    want = np.concatenate([planted[f"{fam}_level3"][pick] for fam in P.FAMILIES])
    assert tiles.shape[0] == 4 * P.TILES_PER_CELL * len(P.cells_of_modes((mode,)))
    assert_blocks(uastc.encode_uastc_blocks(hip_ctx, tiles, 3), want, f"mode {mode} alone", [P.planted_cells()[i] for i in pick] * 4)


def encode_guarded(ctx, tiles, flags):
    """encode into a buffer that held 0xA5, with GUARD bytes behind it that must still hold it"""
    n = tiles.shape[0]
    d_out = ctx.alloc(n * 16 + GUARD)
    try:
        ctx.memset(d_out, 0xA5, n * 16 + GUARD)
        uastc.encode_uastc_blocks(ctx, np.ascontiguousarray(tiles), flags, out_device=d_out)
        got = ctx.download(d_out, (n + GUARD // 16, 16), np.uint8)
    finally:
        ctx.free(d_out)
    assert (got[n:] == 0xA5).all(), "bytes behind the last block were written"
    return got[:n]


@pytest.mark.parametrize("level", [2, 3])
def test_mixed_company(hip_ctx, planted, old_vectors, level):
    """Every tile with a known answer in one call under one fixed permutation: the four families, the 1,464 image-like tiles of uastc_reference_vectors.npz and, once
    more, its 48 solid tiles -- 5,592 blocks, two ordering workgroups. The finish kernel's sort puts each tile into a wave with other company than in the calls the
    answers came from, so the wave-wide choice of the ETC1 hint search's form falls differently; every block must still be the reference's."""
    old_tiles = old_vectors["blocks"]
    solid = np.flatnonzero((old_tiles.reshape(-1, 16, 4) == old_tiles.reshape(-1, 16, 4)[:, :1]).all(axis=(1, 2)))
    assert solid.size == 48
    tiles = np.concatenate([planted[f"{fam}_tiles"] for fam in P.FAMILIES] + [old_tiles, old_tiles[solid]])
    want = np.concatenate([planted[f"{fam}_level{level}"] for fam in P.FAMILIES] + [old_vectors[f"level{level}"], old_vectors[f"level{level}"][solid]])
    n = tiles.shape[0]
    assert n > 4096 and want.shape == (n, 16)
    order = np.random.default_rng(31).permutation(n)
    got = encode_guarded(hip_ctx, tiles[order], level)
    never = int((got == 0xA5).all(axis=1).sum())
    assert_blocks(got, want[order], f"level {level}, {never} blocks never written", None)


@pytest.mark.parametrize("level", [2, 3])
def test_edge_interleaved_with_exact(hip_ctx, planted, level):
    """edge and exact tile by tile: tiles whose ETC1 hint search clamps next to tiles of the same cell where it does not"""
    n = planted["exact_tiles"].shape[0]
    tiles = np.stack([planted["edge_tiles"], planted["exact_tiles"]], axis=1).reshape(2 * n, 4, 4, 4)
    want = np.stack([planted[f"edge_level{level}"], planted[f"exact_level{level}"]], axis=1).reshape(2 * n, 16)
    assert_blocks(encode_guarded(hip_ctx, tiles, level), want, f"level {level}", [c for c in P.planted_cells() for _ in range(2)])


@pytest.mark.parametrize("name,src,flags,jobs,kw", P.rdo_arrays(), ids=[a[0] for a in P.rdo_arrays()])
def test_rdo_equals_reference(hip_ctx, planted, name, src, flags, jobs, kw):
    packed, tiles, want = planted[src], planted["sibling_tiles"], planted[name]
    got, info = uastc.uastc_rdo(hip_ctx, packed, tiles, params(**kw), flags, jobs)
    assert_blocks(got, want, name)
    _, counts = helpers.host_uastc_rdo_counted(packed, tiles, flags, jobs, True, **kw)
    assert info == dict(counts, strips=strips_of(packed.shape[0], jobs)), name
    untouched = (want == packed).all(axis=1)
    assert 0 < untouched.sum() < packed.shape[0] and (got[untouched] == packed[untouched]).all()


@pytest.mark.parametrize("jobs", [3, 7])
def test_rdo_strips_that_begin_inside_a_cell(hip_ctx, planted, jobs):
    """The siblings of a cell are each other's candidates. 168 of the 170 cells (a multiple of both strip counts) in another, fixed order, the whole array rotated by
    three tiles: every strip begins in the middle of a cell, so its first three blocks find half of their siblings outside it. Against the host build of the same
    core, counters included."""
    n = 168 * P.TILES_PER_CELL
    cell_order = np.random.default_rng(32).permutation(planted["sibling_tiles"].shape[0] // P.TILES_PER_CELL)[:168]
    order = np.roll((cell_order[:, None] * P.TILES_PER_CELL + np.arange(P.TILES_PER_CELL)[None, :]).reshape(-1), 3)
    starts = np.arange(0, n, n // jobs)
    assert strips_of(n, jobs) == starts.size == jobs and ((starts - 3) % P.TILES_PER_CELL == 3).all()
    packed, tiles = np.ascontiguousarray(planted["sibling_level3"][order]), np.ascontiguousarray(planted["sibling_tiles"][order])
    want, counts = helpers.host_uastc_rdo_counted(packed, tiles, 3, jobs, True, lam=4.0)
    got, info = uastc.uastc_rdo(hip_ctx, packed, tiles, params(lam=4.0), 3, jobs)
    assert_blocks(got, want, f"jobs {jobs}")
    assert info == dict(counts, strips=starts.size)
    assert len(P.modified_cells(packed, want)) >= 85


CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import uastc_planted as P
from basis_universal_amd import capi, uastc
ctx = capi.Context()
got = uastc.encode_uastc_blocks(ctx, np.ascontiguousarray(P.load()[0]["exact_tiles"]), 3)
ctx.close()
got.tofile(sys.argv[2])
"""


def test_separate_scoring_pass(planted, tmp_path):
    """BU_UASTC_FUSED_SCORE=0 scores the candidates in a pass of its own (k_uastc_score) where the default scores them in the kernel that builds them. The library
    reads the variable once per process, so the encode runs in one fresh child process (started, never exec'ed into); `exact` at level 3, against the reference."""
    out = tmp_path / "exact_level3.bin"
    env = dict(os.environ, BU_UASTC_FUSED_SCORE="0")
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, f"the child process ended with status {r.returncode}:\n{r.stdout[-3000:]}"
    got = np.fromfile(out, np.uint8).reshape(-1, 16)
    assert_blocks(got, planted["exact_level3"], "separate scoring pass", P.planted_cells())
