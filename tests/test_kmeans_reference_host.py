"""CPU only. (1) tests/kmeans_reference.py, the vectorised numpy statement of the k-means steps, against brute-force loops in Python integers and scalars on
tiny inputs. (2) The inputs of tests/test_gpu_kmeans_kernels.py (tests/kmeans_cases.py) are hard enough: judged by the reference alone, a kernel that takes
the runner-up, drops a tie rule or never comes near a carry could not pass on them."""
import numpy as np
import pytest

import kmeans_cases as K
import kmeans_reference as R


# ----------------------------------------------------------------------------- (1) the reference against loops

def test_unpack_selectors_against_loops():
    rng = np.random.default_rng(1)
    comps = rng.integers(0, 4, size=(50, 16))
    keys = [sum(int(v) << (30 - 2 * d) for d, v in enumerate(row)) for row in comps]
    assert (R.unpack_selectors(np.array(keys, np.uint32)) == comps).all()
    assert R.unpack_selectors(np.array([0xC0000000, 1], np.uint32)).tolist() == [[3] + [0] * 15, [0] * 15 + [1]]   # value 0 in the top two bits


def test_unpack_endpoints_against_loops():
    rng = np.random.default_rng(2)
    comps = rng.integers(0, 256, size=(50, 6))
    keys = [sum(int(v) << (40 - 8 * d) for d, v in enumerate(row)) for row in comps]
    sizes = rng.integers(1, 1000, size=50)
    vec, w = R.unpack_endpoints(np.array(keys, np.uint64), np.concatenate([[0], np.cumsum(sizes)]))
    assert (vec[:, :6] == comps).all() and (vec[:, 6:] == 0).all()
    assert w.dtype == np.uint64 and w.tolist() == [2 * int(s) for s in sizes]


@pytest.mark.parametrize("n,k", [(1, 1), (7, 1), (7, 7), (40, 13), (100, 99)])
@pytest.mark.parametrize("pattern", ["uniform", "heavy_first", "heavy_middle", "heavy_last", "huge", "wide", "random"])
def test_seeding_against_loops(n, k, pattern):
    w = np.random.default_rng(n).integers(1, 50, size=n).astype(np.uint64) if pattern == "random" else K.seed_weights(0, n, pattern)
    wl = [int(x) for x in w]
    total = sum(wl)
    pick = []
    for c in range(k):
        target = total * (2 * c + 1) // (2 * k)
        u = 0
        while sum(wl[:u + 1]) <= target:
            u += 1
        pick.append(u)
    assert R.seed_pick(w, k).tolist() == pick
    distinct = [c + min(max(pick[j] - j for j in range(c + 1)), n - k) for c in range(k)]
    got = R.make_distinct(pick, n, k).tolist()
    assert got == distinct and got == R.seeds(w, n, k).tolist()
    assert all(b > a for a, b in zip(got, got[1:])) and 0 <= got[0] and got[-1] < n


@pytest.mark.parametrize("n,k", [s for s in K.SEED_SHAPES if s[1] > 1])
def test_wide_seed_weights_need_more_than_64_bits(n, k):
    total = int(sum(int(x) for x in K.seed_weights(0, n, "wide")))
    assert total < 2 ** 64 <= total * (2 * k - 1)


def test_gemm_centroid_against_scalars():
    rng = np.random.default_rng(3)
    cen = np.concatenate([rng.uniform(0, 255, size=(20, 16)), rng.uniform(0, 3, size=(20, 16)), [[0.0] * 16], [[1.0 / 3] * 16]]).astype(np.float32)
    got = R.gemm_centroids(cen)
    for c in range(cen.shape[0]):
        for d in range(16):
            a = np.float32(-2.0) * cen[c, d]
            hi = np.float16(a)
            lo = np.float16(np.float32(a - np.float32(hi)))
            assert got[c, d] == -0.5 * (float(hi) + float(lo))
            assert np.float32(hi) + np.float32(lo) == np.float32(float(hi) + float(lo)), "the device adds the halves in float32: exact"
    assert abs(got - cen.astype(np.float64)).max() <= 255 * 2.0 ** -21   # two f16 halves keep 22 bits
    assert (got[-2] == 0).all()


def test_distances_and_eps_against_loops():
    rng = np.random.default_rng(4)
    vec = rng.integers(0, 256, size=(9, 16)); vec[:, 6:] = 0
    cp = R.gemm_centroids(rng.uniform(0, 255, size=(5, 16)).astype(np.float32)); cp[:, 6:] = 0
    live = np.array([1, 0, 9, 1, 1], np.uint64)
    d, e = R.distances(vec, cp, live), R.eps_bound(vec, cp, live)
    for u in range(9):
        s_max, d_min = 0.0, np.inf
        for c in range(5):
            dd = sum((float(vec[u, i]) - cp[c, i]) ** 2 for i in range(16))
            if live[c] == 0:
                assert d[u, c] == np.inf
                continue
            assert abs(d[u, c] - dd) <= 1e-9 * dd
            s_max = max(s_max, sum(cp[c, i] ** 2 for i in range(16)) + 2 * sum(abs(cp[c, i] * float(vec[u, i])) for i in range(16)))
            d_min = min(d_min, dd)
        assert abs(e[u] - 2.0 ** -24 * (178 * s_max + 40 * d_min)) <= 1e-9 * e[u]


def test_integer_distances_equal_the_float64_ones():
    rng = np.random.default_rng(7)
    vec, cen = rng.integers(0, 256, size=(40, 16)), rng.integers(0, 256, size=(11, 16))
    live = np.ones(11, np.uint64); live[[0, 5]] = 0
    di, df = R.integer_distances(vec, cen, live), R.distances(vec, R.gemm_centroids(cen.astype(np.float32)), live)
    assert (di[:, live != 0] == df[:, live != 0]).all() and np.isinf(df[:, live == 0]).all() and (di[:, live == 0] > 2 ** 62).all()


def test_sums_update_against_loops():
    rng = np.random.default_rng(5)
    n, k = 60, 7
    vec = rng.integers(0, 256, size=(n, 16))
    w = rng.integers(1, 2 ** 40, size=n).astype(np.uint64)
    assign = rng.integers(0, k - 1, size=n)   # cluster k - 1 stays empty
    for dims in (6, 16):
        got = R.sums_from_assign(vec, w, assign, k, dims)
        exp = [[0] * 17 for _ in range(k)]
        for u in range(n):
            for d in range(dims):
                exp[assign[u]][d] += int(w[u]) * int(vec[u, d])
            exp[assign[u]][16] += int(w[u])
        assert got.dtype == np.uint64 and got.tolist() == exp
        old = rng.uniform(0, 255, size=(k, 16)).astype(np.float32)
        new = R.update(got, old)
        for c in range(k):
            for d in range(16):
                assert new[c, d] == (np.float32(float(exp[c][d]) / float(exp[c][16])) if exp[c][16] else old[c, d])
        assert (new[k - 1] == old[k - 1]).all()


def test_reseed_and_compact_against_loops():
    rng = np.random.default_rng(6)
    n, k = 1300, 9    # three groups of 512, the last one short
    vec = rng.integers(0, 4, size=(n, 16))
    w = rng.integers(1, 5, size=n).astype(np.uint64)
    bd = rng.integers(0, 6, size=n).astype(np.float64)   # few distinct keys: equal keys inside and between groups
    groups = []
    for g0 in range(0, n, 512):
        best = None
        for u in range(g0, min(g0 + 512, n)):
            key = float(np.float32(bd[u]) * np.float32(w[u]))
            if best is None or key > best[0]:
                best = (key, u)
        groups.append(best)
    assert [(float(a), b) for a, b in R.worst_of_groups(bd, w)] == groups
    assert len({g[0] for g in groups}) < 3, "equal keys between groups were meant to occur"
    words = R.worst_words(bd, w)
    assert [int(x) >> 32 for x in words] == [int(np.float32(g[0]).view(np.uint32)) for g in groups]
    assert [0xFFFFFFFF - (int(x) & 0xFFFFFFFF) for x in words] == [g[1] for g in groups]
    order = sorted(range(3), key=lambda i: (-groups[i][0], groups[i][1]))
    assert sorted(range(3), key=lambda i: -int(words[i])) == order, "descending words = descending key, ascending index"
    for empties in ([], [0], [8], [0, 4, 8], [0, 1, 4, 7, 8]):
        sums = np.zeros((k, 17), np.uint64); sums[:, 16] = 5; sums[empties, 16] = 0
        old = rng.uniform(0, 3, size=(k, 16)).astype(np.float32)
        cen, live = R.reseed(vec, w, bd, sums, old)
        for j, c in enumerate(empties):
            if j < 3:
                assert (cen[c] == vec[groups[order[j]][1]]).all() and live[c] == 1
            else:
                assert (cen[c] == old[c]).all() and live[c] == 0
        rest = [c for c in range(k) if c not in empties]
        assert (cen[rest] == old[rest]).all() and (live[rest] == 5).all()
    assign = rng.integers(0, k, size=n); assign[assign == 3] = 2
    sums = R.sums_from_assign(vec, w, assign, k, 16)
    got, kl = R.compact(assign, sums)
    used = sorted(set(assign.tolist()))
    assert kl == len(used) == k - 1 and got.tolist() == [used.index(a) for a in assign]


# ----------------------------------------------------------------------------- (2) the GPU tests' inputs

@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,k", K.FRACTIONAL_SHAPES)
def test_fractional_inputs_have_clear_winners(kind, n, k):
    """At least 90 % of the vectors have a float64 gap between nearest and second-nearest c' above 4 eps(u) (a kernel that takes the runner-up fails on them);
    fewer than 2 % lie within eps of a tie (where the bound could hide a wrong choice). Both f16 halves of -2c are in use."""
    prob, cen = K.fractional_problem(kind, n, k)
    cp = R.gemm_centroids(cen)
    d = np.sort(R.distances(prob.vec, cp), axis=1)
    gap, eps = d[:, 1] - d[:, 0], R.eps_bound(prob.vec, cp)
    clear, close = (gap > 4 * eps).mean(), (gap <= eps).mean()
    print(f"{K.KIND_NAME[kind]} n={n} k={k}: gap > 4 eps for {clear:.1%}, gap <= eps for {close:.2%}; median eps {np.median(eps):.3g}, median gap {np.median(gap):.3g}")
    assert clear >= 0.90 and close < 0.02
    a = (np.float32(-2) * cen[:, :prob.dims]).astype(np.float32)
    lo = (a - a.astype(np.float16).astype(np.float32)).astype(np.float16)
    assert (a.astype(np.float16) != 0).mean() > 0.9 and (lo != 0).mean() > 0.5


def _tile(c):
    return c // 32


def _half(c):
    return (c % 32) // 4 % 2   # rows (r & 3) + 8 (r >> 2) + 4 kb: bit 2 of the row is the half-wave


@pytest.mark.parametrize("kind", K.KINDS)
def test_integer_inputs_have_ties_across_tiles_and_half_waves(kind):
    prob, cen_idx, bases = K.tie_problem(kind)
    d = R.distances(prob.vec, R.gemm_centroids(prob.vec[cen_idx].astype(np.float32)))
    across_tiles = across_halves = 0
    for u in bases:
        tied = np.nonzero(d[u] == d[u].min())[0]
        assert d[u].min() == 1.0 and tied.size >= 2
        across_tiles += len({_tile(c) for c in tied}) > 1
        across_halves += any(_tile(a) == _tile(b) and _half(a) != _half(b) for a in tied for b in tied)
    assert across_tiles >= 1 and across_halves >= 1
    # random integer data ties by itself too (selectors: few distinct distances), counted for the record
    nat = sum(1 for u in range(prob.n) if (d[u] == d[u].min()).sum() > 1)
    print(f"{K.KIND_NAME[kind]}: planted ties across tiles {across_tiles}, across half-waves {across_halves}; vectors with any tie {nat} of {prob.n}")


@pytest.mark.parametrize("kind", K.KINDS)
def test_zero_centroid_input(kind):
    prob, cen_idx, near = K.zero_problem(kind)
    cen = prob.vec[cen_idx].astype(np.float32)
    zero_row = int(np.nonzero((cen == 0).all(axis=1))[0][0])
    assert zero_row % 32 >= 4, "the zero centroid must not sit in group 0 of its tile, where a lost tag would go unnoticed"
    d = R.distances(prob.vec, R.gemm_centroids(cen))
    for u in near:
        assert np.argmin(d[u]) == zero_row and (d[u] == d[u].min()).sum() == 1
    keys = (cen.astype(np.float64) ** 2).sum(axis=1)[None, :] - 2 * prob.vec @ cen.astype(np.float64).T
    assert (keys[:, zero_row] == 0).all()


@pytest.mark.parametrize("kind", K.KINDS)
def test_packed_boundary_input(kind):
    v = K.MAX_VALUE[kind]
    prob, total = K.boundary_problem(kind, over=False)
    sums = R.sums_from_assign(prob.vec, prob.weights, np.zeros(prob.n, np.int64), 1, prob.dims)
    assert int(sums[0, 16]) == total and int(sums[0, 2]) == int(sums[0, 3]) == total * v
    assert 2 ** 32 - 2 ** 20 <= int(sums[0, 2]) < 2 ** 32, "packed, and the low half of the word is within 2^20 of carrying"
    assert (total + (2 if kind else 1)) * v >= 2 ** 32, "no larger total could be packed"
    prob, total = K.boundary_problem(kind, over=True)
    assert int(prob.weights.sum()) == total and total * v >= 2 ** 32 > (total - (2 if kind else 1)) * v
    assert (prob.vec[:, [2, 3]] == v).all() and (np.delete(prob.vec, [2, 3], axis=1) < v).all()


def test_colliding_ids_collide():
    for ids in K.colliding_ids(2049):
        assert len({(int(c) * 2654435761 % 2 ** 32) >> 24 for c in ids}) == 1 and ids.size >= 6


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("name", sorted(K.RESEED_CASES))
def test_reseed_inputs(kind, name):
    """the far centroids attract nobody; bd * w is exact in float32 (but for the two planted keys); the planted equal keys are equal, the largest of their groups, in different groups"""
    n, k, far, equal = K.RESEED_CASES[name]
    prob, cen, far = K.reseed_problem(kind, name)
    assert (cen == np.round(cen)).all()
    d = R.distances(prob.vec, R.gemm_centroids(cen))
    assert not np.isin(np.argmin(d, axis=1), far).any() and all((d[:, c] > d.min(axis=1)).all() for c in far)
    bd = d.min(axis=1)
    assert ((bd * prob.weights.astype(np.float64)) < 2 ** 24).all() or equal
    worst = R.worst_of_groups(bd, prob.weights)
    assert len(worst) == (n + 511) // 512
    if equal:
        assert worst[0][0] == worst[1][0] > worst[2][0] and worst[0][1] < 512 <= worst[1][1]
        a, b = worst[0][1], worst[1][1]
        # the two products are the same integer (beyond 2^24 for endpoints: both round to the same float32, and both factors are exact in float32)
        assert int(bd[a]) * int(prob.weights[a]) == int(bd[b]) * int(prob.weights[b]) and max(bd[a], bd[b], int(prob.weights[a]), int(prob.weights[b])) < 2 ** 24
