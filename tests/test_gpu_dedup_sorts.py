"""-m gpu parity tests of the three entry points that sort: bu_hip_k_unique_selector_vectors, bu_hip_k_unique_endpoint_vectors (unique_kernels.hip) and
bu_hip_k_map_rank_blocks (bookkeeping_kernels.hip), on every path sort_pairs.h can take -- the single-block sort, the merge sort, the one-sweep radix sort -- and on
both sides of both switches between them.

The cases and the expected values are tests/dedup_sort_cases.py's: keys by the format's definition, then numpy (np.unique, a stable argsort, np.add.reduceat on uint64).
tests/test_dedup_sort_cases_host.py holds the cases to what they were built for and the keys to the plain-C oracle, without a GPU. Everything is integer work: every
comparison is exact, and a failure names the entry point, the case, the output, the first differing index and got / want.

Every output buffer has its documented capacity (n entries; n + 1 offsets; k + 1 sizes and offsets of the ranking) and SLACK bytes behind it, all of it 0xAB before the
call: the slack must come back untouched. Nothing is asserted about the entries between the number of distinct vectors and the capacity: the scan legitimately writes
there."""
import ctypes as C

import numpy as np
import pytest

import dedup_sort_cases as D

pytestmark = pytest.mark.gpu

SLACK = 64
FILL = 0xAB
TOO_MANY = (1 << 30) + 1


# ----------------------------------------------------------------------------- buffers with a sentinel

def _out(ctx, nbytes):
    """a device buffer of nbytes + SLACK bytes, all 0xAB"""
    d = ctx.alloc(nbytes + SLACK)
    ctx.check(ctx.lib.memset(ctx.h, d, FILL, nbytes + SLACK), "memset")
    return d


def _fetch(ctx, d, count, dtype, what):
    """the first `count` entries of a buffer made by _out (then freed); the SLACK bytes behind them must still hold the sentinel"""
    nbytes = count * np.dtype(dtype).itemsize
    raw = ctx.download(d, (nbytes + SLACK,), np.uint8)
    ctx.free(d)
    assert (raw[nbytes:] == FILL).all(), f"{what}: wrote past its {count} entries: bytes {np.nonzero(raw[nbytes:] != FILL)[0][:8]} of the slack"
    return raw[:nbytes].copy().view(dtype)


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape} entries, want {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at [{bad[0]}]: got {got[bad[0]]} want {want[bad[0]]}"


# ----------------------------------------------------------------------------- running a case

def _run_unique(ctx, case):
    """-> (u, keys[n], offsets[n + 1], idx[n], weights[n] or None) as the device left them"""
    n, L = case.n, ctx.lib
    what = f"unique_{case.kind}_vectors {case.name} (n {n}, {case.path})"
    key_t = np.uint32 if case.kind == "selector" else np.uint64
    d_blocks = ctx.upload(case.blocks)
    d_idx, d_keys, d_ofs = _out(ctx, n * 4), _out(ctx, n * np.dtype(key_t).itemsize), _out(ctx, (n + 1) * 4)
    u = C.c_uint32(12345)
    if case.kind == "selector":
        d_w, d_uw = ctx.upload(case.weights), _out(ctx, n * 8)
        ok = L.k_unique_selector_vectors(ctx.h, d_blocks, d_w, n, d_idx, d_keys, d_uw, d_ofs, C.byref(u))
    else:
        d_w = d_uw = None
        ok = L.k_unique_endpoint_vectors(ctx.h, d_blocks, n, d_idx, d_keys, d_ofs, C.byref(u))
    err = L.last_error(ctx.h) if not ok else ""
    got = (u.value, _fetch(ctx, d_keys, n, key_t, what + " keys"), _fetch(ctx, d_ofs, n + 1, np.uint32, what + " offsets"), _fetch(ctx, d_idx, n, np.uint32, what + " block order"),
           _fetch(ctx, d_uw, n, np.uint64, what + " weights") if d_uw else None)
    ctx.free(d_blocks)
    if d_w:
        ctx.free(d_w)
    assert ok, f"{what}: {err}"
    return got


def _check_unique(case, got):
    what = f"unique_{case.kind}_vectors {case.name} (n {case.n}, {case.path})"
    uniq, offsets, order, sums = case.reference
    u, keys, ofs, idx, w = got
    assert u == uniq.size, f"{what}: {u} distinct vectors, want {uniq.size}"
    _same(what + " distinct keys", keys[:u], uniq)
    _same(what + " group offsets", ofs[:u + 1], offsets)
    _same(what + " block order", idx, order)
    if sums is not None:
        _same(what + " weight sums", w[:u], sums)


def _used(got):
    """the defined part of a result (everything up to the number of distinct vectors), for byte comparisons between two runs"""
    u, keys, ofs, idx, w = got
    return [np.uint32(u).tobytes(), keys[:u].tobytes(), ofs[:u + 1].tobytes(), idx.tobytes(), b"" if w is None else w[:u].tobytes()]


def _run_rank(ctx, case, with_pos):
    """-> (sizes[k + 1], offsets[k + 1], sorted[n], pos[n] or None)"""
    n, k = case.n, case.k
    what = f"map_rank_blocks {case.name} (n {n}, k {k}, {case.path}, {'with' if with_pos else 'no'} pos)"
    d_cluster = ctx.upload(case.cluster)
    d_sizes, d_offsets, d_sorted = _out(ctx, (k + 1) * 4), _out(ctx, (k + 1) * 4), _out(ctx, n * 4)
    d_pos = _out(ctx, n * 4) if with_pos else None
    ok = ctx.lib.k_map_rank_blocks(ctx.h, d_cluster, n, k, d_sizes, d_offsets, d_sorted, d_pos)
    err = ctx.lib.last_error(ctx.h) if not ok else ""
    got = (_fetch(ctx, d_sizes, k + 1, np.uint32, what + " sizes"), _fetch(ctx, d_offsets, k + 1, np.uint32, what + " offsets"),
           _fetch(ctx, d_sorted, n, np.uint32, what + " sorted blocks"), _fetch(ctx, d_pos, n, np.uint32, what + " positions") if with_pos else None)
    ctx.free(d_cluster)
    assert ok, f"{what}: {err}"
    return got


def _check_rank(case, got, with_pos):
    what = f"map_rank_blocks {case.name} (n {case.n}, k {case.k}, {case.path}, {'with' if with_pos else 'no'} pos)"
    sizes, offsets, order, pos = case.reference
    _same(what + " sorted blocks", got[2], order)
    _same(what + " offsets", got[1], offsets)
    _same(what + " sizes", got[0], sizes)
    if with_pos:
        _same(what + " positions", got[3], pos)


# ----------------------------------------------------------------------------- parity (and, on the radix path, repeatability)

def _unique_parity(ctx, kind, name):
    case = D.unique_case(kind, name)
    got = _run_unique(ctx, case)
    _check_unique(case, got)
    if case.path == "radix":        # the one-sweep sort's look-back order differs from run to run; the result may not
        assert _used(_run_unique(ctx, case)) == _used(got), f"unique_{kind}_vectors {name}: two runs differ"


@pytest.mark.parametrize("name", D.SELECTOR_CASES)
def test_unique_selector_vectors(hip_ctx, name):
    _unique_parity(hip_ctx, "selector", name)


@pytest.mark.parametrize("name", D.ENDPOINT_CASES)
def test_unique_endpoint_vectors(hip_ctx, name):
    _unique_parity(hip_ctx, "endpoint", name)


@pytest.mark.parametrize("with_pos", [True, False], ids=["pos", "no_pos"])
@pytest.mark.parametrize("name", D.RANK_CASES)
def test_map_rank_blocks(hip_ctx, name, with_pos):
    case = D.rank_case(name)
    got = _run_rank(hip_ctx, case, with_pos)
    _check_rank(case, got, with_pos)
    if case.path == "radix":
        again = _run_rank(hip_ctx, case, with_pos)
        assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(got, again)), f"map_rank_blocks {name}: two runs differ"


# ----------------------------------------------------------------------------- the shared workspace

def test_results_do_not_depend_on_the_workspaces_last_user(hip_ctx):
    """All three entry points carve their temporaries out of one arena of the context. A large selector case, a small ranking, a large endpoint case, a small selector
    case and the first one again, back to back on one context: each finds the arena as the one before left it (and, after the large ones, larger than it needs), each
    must equal its reference, and the two runs of the first must be byte-equal."""
    scales = D.unique_case("selector", "run_scales")
    first = _run_unique(hip_ctx, scales)
    _check_unique(scales, first)
    rank = D.rank_case("switch_n1024_k37")
    _check_rank(rank, _run_rank(hip_ctx, rank, True), True)
    ep = D.unique_case("endpoint", "random_selectors")
    _check_unique(ep, _run_unique(hip_ctx, ep))
    small = D.unique_case("selector", "switch_n1025")
    _check_unique(small, _run_unique(hip_ctx, small))
    second = _run_unique(hip_ctx, scales)
    _check_unique(scales, second)
    assert _used(first) == _used(second), "selector run_scales: the run after the other entry points differs from the run before them"


# ----------------------------------------------------------------------------- more blocks than the sorts take

@pytest.mark.parametrize("entry", ["selector", "endpoint", "rank"])
def test_more_than_2_30_blocks_are_refused(hip_ctx, entry):
    """n = 2^30 + 1: the call returns 0 and names the limit, the count of distinct vectors is 0, and nothing is written -- the outputs here are a few sentinel-filled
    bytes, far smaller than such a call's, and the refusal comes before the workspace for 2^30 blocks would be reserved."""
    L = hip_ctx.lib
    d_in = hip_ctx.upload(np.zeros(64, np.uint64))
    outs = [_out(hip_ctx, 256) for _ in range(4)]
    u = C.c_uint32(12345)
    if entry == "selector":
        ok = L.k_unique_selector_vectors(hip_ctx.h, d_in, d_in, TOO_MANY, outs[0], outs[1], outs[2], outs[3], C.byref(u))
    elif entry == "endpoint":
        ok = L.k_unique_endpoint_vectors(hip_ctx.h, d_in, TOO_MANY, outs[0], outs[1], outs[2], C.byref(u))
    else:
        ok = L.k_map_rank_blocks(hip_ctx.h, d_in, TOO_MANY, 37, outs[0], outs[1], outs[2], outs[3])
    err = L.last_error(hip_ctx.h)
    hip_ctx.sync()
    raw = [hip_ctx.download(d, (256 + SLACK,), np.uint8) for d in outs]
    for d in outs + [d_in]:
        hip_ctx.free(d)
    assert ok == 0, f"{entry}: accepted {TOO_MANY} blocks"
    assert "more than 2^30" in err and str(TOO_MANY) in err, err
    name = {"selector": "unique_selector_vectors", "endpoint": "unique_endpoint_vectors", "rank": "map_rank_blocks"}[entry]
    assert err.startswith(name + ":"), err
    if entry != "rank":
        assert u.value == 0
    assert all((r == FILL).all() for r in raw), f"{entry}: an output was written"
