"""-m gpu parity tests of the three paths of bu_hip_k_refine_endpoint_clusterization (bu_hip_tuning::refine_unsorted: 0 = sorted candidate lists with one block per lane --
k_refine_bucket_count / _scan / _scatter + k_refine_block_lanes --, 1 = the unsorted kernel, 2 = sorted lists with one block per wave), bit-exact against
oracle/etc1s_oracle.c on the inputs of refine_block_lane_cases.py. What those inputs reach (bucket sizes around a wave's 64 lanes, lanes that queue nothing beside lanes
that queue several times the queue's capacity, ties, lists without an admissible entry, blocks that are strangers to their list) is held on the CPU by
test_refine_block_lane_cases_host.py."""
import numpy as np
import pytest

import refine_block_lane_cases as RB

pytestmark = pytest.mark.gpu

NAMES = ("tiles", "block_cluster", "params", "cand_offsets", "cand_indices", "block_parent")


def _path_meant(mode, perceptual):
    """the linear metric has no one-block-per-lane kernel: refine_unsorted = 0 takes 2's path there"""
    return 2 if mode == 0 and not perceptual else mode


def _refine(hip_ctx, arrays, n_parents, perceptual, first=0, count=None):
    """one call on blocks [first, first + count): the per-block pointers offset, as a slab of a multi-device frontend offsets them"""
    tiles, cur, params, coffs, cidx, parent = arrays
    n = tiles.shape[0] if count is None else count
    bufs = [hip_ctx.upload(a) for a in arrays]
    d_out = hip_ctx.alloc(tiles.shape[0] * 4)
    try:
        hip_ctx.memset(d_out, 0xEE, tiles.shape[0] * 4)
        hip_ctx.check(hip_ctx.lib.k_refine_endpoint_clusterization(hip_ctx.h, bufs[0] + first * 64, n, bufs[1] + first * 4, bufs[2], params.shape[0], n_parents, bufs[3], bufs[4],
                                                                   bufs[5] + first, perceptual, d_out + first * 4), "k_refine")
        return hip_ctx.download(d_out, (tiles.shape[0],), np.uint32)
    finally:
        for p in bufs + [d_out]:
            hip_ctx.free(p)


@pytest.fixture
def mode_ctx(hip_ctx, request):
    def set_mode(mode):
        hip_ctx.set_tuning(refine_unsorted=mode)
        request.addfinalizer(hip_ctx.set_tuning)   # back to the process defaults
        return hip_ctx
    return set_mode


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("kind", RB.KINDS)
def test_refine_paths_agree_with_the_oracle(mode_ctx, kind, perceptual, mode):
    ctx = mode_ctx(mode)
    c = RB.lane_case(kind, perceptual)
    assert ctx.lib.refine_path(ctx.h, c["params"].shape[0], c["n_parents"], perceptual) == _path_meant(mode, perceptual)
    got = _refine(ctx, [c[name] for name in NAMES], c["n_parents"], perceptual)
    bad = np.nonzero(got != c["expected"])[0]
    keys = RB.bucket_keys(c)
    assert bad.size == 0, (f"{bad.size} of {got.size} blocks differ; first (block, bucket, group, current, got, expected): "
                           f"{[(int(b), int(keys[b]), int(c['group'][b]), int(c['block_cluster'][b]), int(got[b]), int(c['expected'][b])) for b in bad[:6]]}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("perceptual", [1, 0])
def test_refine_on_a_sub_range(mode_ctx, perceptual, mode):
    ctx = mode_ctx(mode)
    c = RB.lane_case("hier", perceptual)
    s0, s1 = RB.SLAB
    got = _refine(ctx, [c[name] for name in NAMES], c["n_parents"], perceptual, first=s0, count=s1 - s0)
    assert (got[s0:s1] == c["expected"][s0:s1]).all(), np.nonzero(got[s0:s1] != c["expected"][s0:s1])[0][:8] + s0
    assert (got[:s0] == 0xEEEEEEEE).all() and (got[s1:] == 0xEEEEEEEE).all()   # nothing written outside the range


def test_refine_path_choice_and_refusal(hip_ctx, request):
    request.addfinalizer(hip_ctx.set_tuning)
    path = hip_ctx.lib.refine_path
    assert hip_ctx.tuning()["refine_unsorted"] == 0
    assert path(hip_ctx.h, 1000, 16, 1) == 0 and path(hip_ctx.h, 1000, 0, 1) == 0 and path(hip_ctx.h, 1000, 16, 0) == 2
    assert path(hip_ctx.h, 65535, 16, 1) == 0 and path(hip_ctx.h, 65536, 16, 1) == 1 and path(hip_ctx.h, 65536, 16, 0) == 1   # ids and positions share a dword
    assert path(None, 1000, 16, 1) == 0                                       # the process defaults
    hip_ctx.set_tuning(refine_unsorted=2)
    assert path(hip_ctx.h, 1000, 16, 1) == 2 and path(hip_ctx.h, 65536, 16, 1) == 1
    hip_ctx.set_tuning(refine_unsorted=1)
    assert path(hip_ctx.h, 1000, 16, 1) == 1
    with pytest.raises(Exception, match="out of range"):
        hip_ctx.set_tuning(refine_unsorted=3)
    assert hip_ctx.tuning()["refine_unsorted"] == 1                           # a refused call changes nothing


def test_one_bucket_of_many_waves(mode_ctx):
    """65,536 + 7 blocks in ONE bucket (one parent of sixteen, every current cluster of one table): 1,025 waves find their place in a single bucket by the prefix search.
    Against the other two paths' output, which the tests above hold to the oracle."""
    c = RB.lane_case("hier", 1)
    rng = np.random.default_rng(5300)
    n = 65536 + 7
    li = 5
    members = c["lists"][li]
    of_table = members[c["params"][members, 3] == 6]
    assert of_table.size >= 4
    arrays = [np.ascontiguousarray(c["tiles"][rng.integers(0, c["tiles"].shape[0], n)]), np.ascontiguousarray(rng.choice(of_table, n).astype(np.uint32)), c["params"],
              c["cand_offsets"], c["cand_indices"], np.full(n, li, np.uint8)]
    got = {}
    for mode in (0, 1, 2):
        ctx = mode_ctx(mode)
        assert ctx.lib.refine_path(ctx.h, c["params"].shape[0], c["n_parents"], 1) == mode
        got[mode] = _refine(ctx, arrays, c["n_parents"], 1)
    assert (got[1] == got[2]).all()
    bad = np.nonzero(got[0] != got[1])[0]
    assert bad.size == 0, (bad.size, bad[:8], got[0][bad[:8]], got[1][bad[:8]])
    assert np.isin(got[0], members).all() and (got[0] != arrays[1]).sum() > n // 10
