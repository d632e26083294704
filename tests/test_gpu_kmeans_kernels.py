"""-m gpu: the kernels of the codebook builders' fast mode (basis_universal_amd/csrc/kmeans_kernels.hip), one step at a time through bu_hip_k_kmeans_seed and
bu_hip_k_kmeans_round, against the float64 / exact-integer numpy reference tests/kmeans_reference.py. Inputs come from tests/kmeans_cases.py;
tests/test_kmeans_reference_host.py checks on the CPU that they are hard enough (ties, clear winners, a sum next to a carry).

Seeds, sums, centroid updates and re-seeding are compared for exact equality. The assignment is exact on integer centroids (every comparison key is an integer
below 2^22, the tag bits sit below its last bit): the assigned centroid's distance must EQUAL the minimum; any of several exactly tied centroids is accepted.
On fractional centroids it is held to eps(u) of kmeans_reference.eps_bound, derived from the float32 operations of the kernel and from nothing measured.
The last test chains the step calls and requires bu_hip_kmeans_codebook's output bit for bit: the steps tested here are the product.

Every output buffer has SLACK bytes of 0xAB behind it, which must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import kmeans_cases as K
import kmeans_reference as R

pytestmark = pytest.mark.gpu

SLACK = 256
FILL = 0xAB
KIND_IDS = [K.KIND_NAME[k] for k in K.KINDS]


class Device:
    """a Problem resident on the device, and the two step calls on it"""

    def __init__(self, ctx, prob):
        self.ctx, self.prob = ctx, prob
        self.d_keys = ctx.upload(prob.keys)
        self.d_weights = ctx.upload(prob.weights) if prob.kind == 0 else None
        self.d_goffs = ctx.upload(prob.goffs) if prob.kind == 1 else None
        self._bufs = [p for p in (self.d_keys, self.d_weights, self.d_goffs) if p]

    def close(self):
        for p in self._bufs:
            self.ctx.free(p)
        self._bufs = []

    def _out(self, nbytes):
        d = self.ctx.alloc(nbytes + SLACK)
        self.ctx.check(self.ctx.lib.memset(self.ctx.h, d, FILL, nbytes + SLACK), "memset")
        return d

    def _in_out(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.ctx.upload(np.concatenate([arr.reshape(-1).view(np.uint8), np.full(SLACK, FILL, np.uint8)]))

    def _fetch(self, d, shape, dtype):
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        raw = self.ctx.download(d, (nbytes + SLACK,), np.uint8)
        self.ctx.free(d)
        assert (raw[nbytes:] == FILL).all(), f"wrote past the end of a {np.dtype(dtype).name}{list(shape)} output"
        return raw[:nbytes].copy().view(dtype).reshape(shape)

    def seed(self, k):
        p = self.prob
        d_pick, d_cen = self._out(k * 4), self._out(k * 64)
        self.ctx.check(self.ctx.lib.k_kmeans_seed(self.ctx.h, p.kind, self.d_keys, self.d_weights, self.d_goffs, p.n, k, d_pick, d_cen), "k_kmeans_seed")
        return self._fetch(d_pick, (k,), np.uint32), self._fetch(d_cen, (k, 16), np.float32)

    def round(self, cen, live=None, update=False, worst=True):
        """-> dict(assign, sums, worst, cen, live); cen / live are the inputs back unless update"""
        p, k = self.prob, cen.shape[0]
        groups = (p.n + R.GROUP - 1) // R.GROUP
        cen = np.ascontiguousarray(cen, np.float32)
        assert cen.shape == (k, 16)
        d_cen = self._in_out(cen)
        d_live = self._in_out(np.asarray(live, np.uint64)) if live is not None else None
        d_assign, d_sums = self._out(p.n * 4), self._out(k * 17 * 8)
        d_worst = self._out(groups * 8) if worst else None
        self.ctx.check(self.ctx.lib.k_kmeans_round(self.ctx.h, p.kind, self.d_keys, self.d_weights, self.d_goffs, p.n, k, d_cen, d_live, int(update), d_assign, d_sums,
                                                   d_worst), "k_kmeans_round")
        out = {"assign": self._fetch(d_assign, (p.n,), np.uint32), "sums": self._fetch(d_sums, (k, 17), np.uint64),
               "worst": self._fetch(d_worst, (groups,), np.uint64) if worst else None, "cen": self._fetch(d_cen, (k, 16), np.float32),
               "live": self._fetch(d_live, (k,), np.uint64) if live is not None else None}
        if not update:
            assert (out["cen"].view(np.uint32) == cen.view(np.uint32)).all() and (live is None or (out["live"] == live).all()), "an assign-only round changed its inputs"
        return out


@pytest.fixture
def device(hip_ctx):
    made = []

    def make(prob):
        made.append(Device(hip_ctx, prob))
        return made[-1]
    yield make
    for d in made:
        d.close()


def _check_sums(prob, got, k):
    """the device's sums against integer numpy on the device's OWN assignment"""
    assert (got["assign"] < k).all()
    exp = R.sums_from_assign(prob.vec, prob.weights, got["assign"], k, prob.dims)
    bad = np.argwhere(got["sums"] != exp)
    assert bad.size == 0, f"sums differ at (cluster, word) {bad[:6].tolist()}: got {[int(got['sums'][c, d]) for c, d in bad[:6]]}, expected {[int(exp[c, d]) for c, d in bad[:6]]}"
    return exp


def _check_exact_assignment(prob, cen, got, live=None, what=""):
    """integer centroids: the assigned centroid is live and its distance EQUALS the minimum, for every vector"""
    d = R.integer_distances(prob.vec, cen, live)
    a = got["assign"].astype(np.int64)
    assert (a < cen.shape[0]).all(), what
    if live is not None:
        assert (np.asarray(live)[a] != 0).all(), f"{what}: vectors {np.nonzero(np.asarray(live)[a] == 0)[0][:8]} were assigned to dead clusters"
    mine, best = d[np.arange(prob.n), a], d.min(axis=1)
    bad = np.nonzero(mine != best)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {prob.n} vectors are not on a nearest centroid; first {bad[:6].tolist()} -> rows {a[bad[:6]].tolist()} at distance "
                           f"{mine[bad[:6]].tolist()}, nearest rows {np.argmin(d[bad[:6]], axis=1).tolist()} at {best[bad[:6]].tolist()}")
    return best


# ----------------------------------------------------------------------------- seeding

# weights near 2^40 / 2^52 exist for selectors only (endpoint weights are 2 x a 32-bit group size)
SEED_PARAMS = [pytest.param(kind, n, k, pattern, id=f"{K.KIND_NAME[kind]}-{n}-{k}-{pattern}") for kind in K.KINDS for n, k in K.SEED_SHAPES for pattern in K.SEED_WEIGHTS
               if K.seed_weights(kind, n, pattern) is not None]


@pytest.mark.parametrize("kind,n,k,pattern", SEED_PARAMS)
def test_seeding_equals_the_reference(device, kind, n, k, pattern):
    w = K.seed_weights(kind, n, pattern)
    prob = K.random_problem(kind, n, 21, weights=w)
    pick, cen = device(prob).seed(k)
    exp = R.seeds(prob.weights, n, k)
    assert (pick == exp).all(), f"picks differ first at centroid {int(np.nonzero(pick != exp)[0][0])}: {pick[pick != exp][:5]} against {exp[pick != exp][:5]}"
    assert (cen == prob.vec[exp].astype(np.float32)).all()
    if k == n:
        assert (pick == np.arange(n)).all()


# ----------------------------------------------------------------------------- assignment, integer centroids

@pytest.mark.parametrize("n", K.ASSIGN_N)
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_assignment_is_exact_on_integer_centroids(device, kind, n):
    prob = K.random_problem(kind, n, 31)
    dev = device(prob)
    rng = np.random.default_rng([32, kind, n])
    for k in [k for k in K.ASSIGN_K if k <= n]:
        for s, idx in enumerate(K.centroid_index_sets(n, k, rng)):
            cen = prob.vec[idx].astype(np.float32)
            got = dev.round(cen)
            _check_exact_assignment(prob, cen, got, None, f"n={n} k={k} set {s}")
            assert (got["assign"][idx] == np.arange(k)).all(), "a vector that IS a centroid has no other nearest centroid"
            _check_sums(prob, got, k)
        for m, live in enumerate(K.dead_masks(k, rng)):
            got = dev.round(cen, live=live)
            _check_exact_assignment(prob, cen, got, live, f"n={n} k={k} dead mask {m}")
            _check_sums(prob, got, k)


@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_assignment_with_planted_ties(device, kind):
    """exact ties of the minimum between tiles and between the half-waves of a tile (test_kmeans_reference_host.py shows they are there): any tied centroid is
    accepted, nothing else"""
    prob, idx, bases = K.tie_problem(kind)
    cen = prob.vec[idx].astype(np.float32)
    got = device(prob).round(cen)
    best = _check_exact_assignment(prob, cen, got, None, "ties")
    assert (best[bases] == 1).all()
    print(f"{K.KIND_NAME[kind]}: tied vectors {bases.tolist()} went to rows {got['assign'][bases].tolist()}")
    _check_sums(prob, got, idx.size)


@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_assignment_with_the_zero_vector_as_a_centroid(device, kind):
    """its key is exactly 0.0 for every vector, so the tagged keys are denormals: the zero vector and its neighbours must still find it"""
    prob, idx, near = K.zero_problem(kind)
    cen = prob.vec[idx].astype(np.float32)
    got = device(prob).round(cen)
    _check_exact_assignment(prob, cen, got, None, "zero centroid")
    zero_row = int(np.nonzero((cen == 0).all(axis=1))[0][0])
    assert (got["assign"][near] == zero_row).all()


# ----------------------------------------------------------------------------- assignment, fractional centroids

@pytest.mark.parametrize("n,k", K.FRACTIONAL_SHAPES)
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_assignment_is_within_eps_on_fractional_centroids(device, kind, n, k):
    """dist(u, assigned) - min_c dist(u, c) <= eps(u) for every vector, distances in float64 to the centroids c' the GEMM really uses.

    eps(u) = 2^-24 (178 max_c S_c(u) + 40 d_min(u)), S_c(u) = |c'|^2 + 2 sum_d |c'_d u_d| (kmeans_reference.eps_bound has the derivation): a comparison key
    carries at most 16 (float32 norm of 16 terms) + 64 (32 MFMA additions of exact products, one ulp each since the matrix core's rounding is undocumented) +
    8 (the tag, 2^-21 |key|) units of 2^-24 S_c, 89 with second-order terms, twice that between two keys; the direct evaluation of the winning four rows adds
    2 x 19 units of 2^-24 d. On these inputs at least 90 % of the vectors have a gap above 4 eps (host test), so taking the runner-up fails here."""
    prob, cen = K.fractional_problem(kind, n, k)
    got = device(prob).round(cen)
    cp = R.gemm_centroids(cen)
    d, eps = R.distances(prob.vec, cp), R.eps_bound(prob.vec, cp)
    a = got["assign"].astype(np.int64)
    assert (a < k).all()
    excess = d[np.arange(n), a] - d.min(axis=1)
    off = int((a != np.argmin(d, axis=1)).sum())
    print(f"{K.KIND_NAME[kind]} n={n} k={k}: {off} of {n} vectors not on the float64 argmin; largest excess / eps = {float((excess / eps).max()):.3g}")
    bad = np.nonzero(excess > eps)[0]
    assert bad.size == 0, f"{bad.size} vectors beyond eps: first {bad[:6].tolist()}, excess {excess[bad[:6]].tolist()}, eps {eps[bad[:6]].tolist()}"
    _check_sums(prob, got, k)


# ----------------------------------------------------------------------------- sums

@pytest.mark.parametrize("over", [False, True], ids=["largest_packed", "smallest_unpacked"])
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_sums_at_the_packing_boundary(device, kind, over):
    """k = 1, the largest value in components 2 and 3 of every vector. Packed: total weight x value is the largest below 2^32 the weights allow (selectors
    2^32 - 1, endpoints 2^32 - 256: endpoint weights are even), one step from carrying into the neighbouring half. The next total must not be packed."""
    prob, total = K.boundary_problem(kind, over)
    got = device(prob).round(prob.vec[:1].astype(np.float32))
    assert (got["assign"] == 0).all()
    exp = _check_sums(prob, got, 1)
    assert int(exp[0, 2]) == total * K.MAX_VALUE[kind] and (int(exp[0, 2]) >= 2 ** 32) == over


@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_sums_unpacked_with_large_weights(device, kind):
    n, k = 600, 40
    prob = K.random_problem(kind, n, 41, weights=K.unpacked_weights(kind, n, np.random.default_rng([41, kind])))
    assert int(prob.weights.sum()) * K.MAX_VALUE[kind] >= 2 ** 32
    cen = prob.vec[::n // k][:k].astype(np.float32)
    got = device(prob).round(cen)
    _check_exact_assignment(prob, cen, got, None, "unpacked")
    _check_sums(prob, got, k)


@pytest.mark.parametrize("n", [512, 1024])
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_sums_when_a_workgroup_sees_more_clusters_than_slots(device, kind, n):
    """512 centroids equal to vectors: a workgroup of 512 vectors sees up to 512 distinct clusters against 256 LDS slots, the rest goes straight to global
    atomics; with n = 1024 two workgroups add to the same sums"""
    prob = K.random_problem(kind, n, 42)
    idx = np.arange(512) * (n // 512)
    cen = prob.vec[idx].astype(np.float32)
    got = device(prob).round(cen)
    _check_exact_assignment(prob, cen, got, None, "slot overflow")
    assert (got["assign"][idx] == np.arange(512)).all()
    for g0 in range(0, n, 512):
        assert np.unique(got["assign"][g0:g0 + 512]).size > 256, "the case was meant to overflow the slot table"
    _check_sums(prob, got, 512)


@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_sums_with_colliding_cluster_ids(device, kind):
    """only clusters whose ids share a first slot are live: every insertion probes past occupied slots"""
    n, k = 2100, 2049   # k <= n
    prob = K.random_problem(kind, n, 43)
    ids = np.concatenate(K.colliding_ids(k))
    live = np.zeros(k, np.uint64); live[ids] = 1
    cen = np.tile(prob.vec[0].astype(np.float32), (k, 1))
    cen[ids] = prob.vec[np.linspace(0, n - 1, ids.size).astype(np.int64)].astype(np.float32)
    got = device(prob).round(cen, live=live)
    _check_exact_assignment(prob, cen, got, live, "colliding ids")
    assert np.unique(got["assign"]).size == ids.size
    _check_sums(prob, got, k)


# ----------------------------------------------------------------------------- update and reseed

@pytest.mark.parametrize("name", sorted(K.RESEED_CASES))
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_update_and_reseed_equal_the_reference(device, kind, name):
    prob, cen, far = K.reseed_problem(kind, name)
    k = cen.shape[0]
    got = device(prob).round(cen, live=np.ones(k, np.uint64), update=True)
    best = _check_exact_assignment(prob, cen, got, None, name)
    sums = _check_sums(prob, got, k)
    assert sorted(np.nonzero(sums[:, 16] == 0)[0].tolist()) == sorted(far), "exactly the far centroids come out empty"
    assert (got["worst"] == R.worst_words(best, prob.weights)).all()
    exp_cen, exp_live = R.reseed(prob.vec, prob.weights, best, sums, R.update(sums, cen))
    assert (got["live"] == exp_live).all()
    assert (got["cen"].view(np.uint32) == exp_cen.view(np.uint32)).all(), f"centroids differ in clusters {np.unique(np.nonzero(got['cen'] != exp_cen)[0])[:8]}"
    groups = (prob.n + R.GROUP - 1) // R.GROUP
    left = far[groups:]
    assert (exp_live[far[:groups]] == 1).all() and (exp_live[left] == 0).all() and (got["cen"][left] == cen[left]).all()


# ----------------------------------------------------------------------------- the steps are the product

def _public(ctx, dev, max_clusters, n_parents, iterations):
    p = dev.prob
    d_cl, d_par = dev._out(p.n * 4), dev._out(p.n * 4)
    oc, op = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)
    ctx.check(ctx.lib.kmeans_codebook(ctx.h, p.kind, dev.d_keys, dev.d_weights, dev.d_goffs, p.n, max_clusters, n_parents, iterations, d_cl, d_par if n_parents else None,
                                      C.byref(oc), C.byref(op)), "kmeans_codebook")
    return dev._fetch(d_cl, (p.n,), np.uint32), dev._fetch(d_par, (p.n,), np.uint32), oc.value, op.value


@pytest.mark.parametrize("iterations", [0, 1, 4])
@pytest.mark.parametrize("n,k", [(513, 65), (1500, 300)])
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_the_steps_are_the_product(hip_ctx, device, kind, n, k, iterations):
    """seed, `iterations` rounds with update, one assign-only round, compaction on the host = bu_hip_kmeans_codebook, bit for bit"""
    prob = K.random_problem(kind, n, 51)
    dev = device(prob)
    _, cen = dev.seed(k)
    live = np.ones(k, np.uint64)
    for _ in range(iterations):
        r = dev.round(cen, live=live, update=True)
        cen, live = r["cen"], r["live"]
    last = dev.round(cen, live=live, worst=False)
    exp, exp_k = R.compact(last["assign"], last["sums"])
    cl, _, out_k, _ = _public(hip_ctx, dev, k, 0, iterations)
    assert out_k == exp_k and (cl == exp).all()


@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_public_call_contract(hip_ctx, device, kind):
    n = 700
    prob = K.random_problem(kind, n, 52)
    dev = device(prob)
    for max_clusters, n_parents in ((90, 0), (90, 8), (n + 50, 0), (n + 50, 900), (1, 1)):
        cl, par, kc, kp = _public(hip_ctx, dev, max_clusters, n_parents, 3)
        assert 1 <= kc <= min(max_clusters, n) and sorted(np.unique(cl).tolist()) == list(range(kc)), "every id in [0, out_clusters) occurs, and no other"
        if n_parents:
            assert 1 <= kp <= min(n_parents, kc) and sorted(np.unique(par).tolist()) == list(range(kp)), "every parent in [0, out_parents) is used"
            first = {}
            for c, p in zip(cl.tolist(), par.tolist()):
                assert first.setdefault(c, p) == p, "two vectors of one cluster share their parent"
        else:
            assert kp == 0


def test_null_and_zero_arguments_are_refused(hip_ctx, device):
    """they return 0 before anything is launched"""
    prob = K.random_problem(0, 40, 53)
    dev = device(prob)
    lib, h = hip_ctx.lib, hip_ctx.h
    d = dev._out(40 * 17 * 8)
    ok = (h, 0, dev.d_keys, dev.d_weights, None, 40, 5, d, d)
    for i, v in ((0, None), (2, None), (3, None), (5, 0), (6, 0), (7, None), (8, None)):
        args = list(ok); args[i] = v
        assert lib.k_kmeans_seed(*args) == 0
    assert lib.k_kmeans_seed(h, 1, dev.d_keys, None, None, 40, 5, d, d) == 0, "endpoints need group offsets"
    ok = (h, 0, dev.d_keys, dev.d_weights, None, 40, 5, d, None, 0, d, d, None)
    for i, v in ((0, None), (2, None), (3, None), (5, 0), (6, 0), (7, None), (10, None), (11, None), (9, 1)):
        args = list(ok); args[i] = v
        assert lib.k_kmeans_round(*args) == 0
    assert lib.kmeans_codebook(h, 0, dev.d_keys, dev.d_weights, None, 0, 5, 0, 1, d, None, C.byref(C.c_uint32()), None) == 0
    assert lib.kmeans_codebook(h, 0, dev.d_keys, dev.d_weights, None, 40, 0, 0, 1, d, None, C.byref(C.c_uint32()), None) == 0
    assert lib.kmeans_codebook(h, 0, None, dev.d_weights, None, 40, 5, 0, 1, d, None, C.byref(C.c_uint32()), None) == 0
    hip_ctx.sync()
    dev._fetch(d, (40 * 17,), np.uint64)   # the sentinel everywhere: nothing ran
