"""Inputs of the k-means kernel tests, made on the CPU from fixed seeds: tests/test_gpu_kmeans_kernels.py runs them on the device,
tests/test_kmeans_reference_host.py checks -- with the numpy reference alone -- that they are hard enough (ties where ties are wanted, clear winners where a
bound is asserted), so that a test on them cannot pass vacuously.

A problem is distinct vectors in ascending key order, as bu_hip_k_unique_*_vectors deliver them: kind 0 = selector vectors (16 values 0..3 packed into a
uint32, explicit uint64 weights), kind 1 = endpoint vectors (6 bytes in a 48-bit key + 10 zero pads, weight = 2 x group size from group offsets)."""
import numpy as np

import kmeans_reference as R

KINDS = (0, 1)
KIND_NAME = {0: "selectors", 1: "endpoints"}
DIMS = {0: 16, 1: 6}
MAX_VALUE = {0: 3, 1: 255}


class Problem:
    """keys (ascending, distinct), weights (uint64), and for endpoints the group offsets the weights come from"""

    def __init__(self, kind, keys, weights):
        self.kind = kind
        self.keys = np.sort(np.asarray(keys, np.uint32 if kind == 0 else np.uint64))
        assert self.keys.size == np.unique(self.keys).size
        self.n = self.keys.size
        w = np.asarray(weights, np.uint64)
        assert w.size == self.n and (w > 0).all()
        if kind == 0:
            self.vec, self.weights, self.goffs = R.unpack_selectors(self.keys), w, None
        else:
            assert (w % np.uint64(2) == 0).all(), "endpoint weights are 2 x group size"
            self.goffs = np.concatenate([[0], np.cumsum(w // np.uint64(2))]).astype(np.uint64)
            assert int(self.goffs[-1]) < 2 ** 32
            self.goffs = self.goffs.astype(np.uint32)
            self.vec, self.weights = R.unpack_endpoints(self.keys, self.goffs)
            assert (self.weights == w).all()
        self.dims = DIMS[kind]

    def index_of(self, keys):
        i = np.searchsorted(self.keys, np.asarray(keys, self.keys.dtype))
        assert (self.keys[i] == np.asarray(keys, self.keys.dtype)).all()
        return i


def key_of(kind, comps):
    """the key of a vector given as a list of components (missing ones 0)"""
    key = 0
    for d, v in enumerate(comps):
        assert 0 <= int(v) <= MAX_VALUE[kind] and d < DIMS[kind]
        key |= int(v) << ((30 - 2 * d) if kind == 0 else (40 - 8 * d))
    return key


def random_keys(kind, n, rng, exclude=()):
    bits = 32 if kind == 0 else 48
    keys = np.unique(rng.integers(0, 2 ** bits, size=2 * n + 64, dtype=np.uint64))
    keys = np.setdiff1d(keys, np.asarray(list(exclude), np.uint64))
    return rng.permutation(keys)[:n]


def small_weights(kind, n, rng, hi=40):
    w = rng.integers(1, hi, size=n).astype(np.uint64)
    return w * np.uint64(2) if kind == 1 else w


def random_problem(kind, n, seed, weights=None):
    rng = np.random.default_rng([seed, kind, n])
    return Problem(kind, random_keys(kind, n, rng), small_weights(kind, n, rng) if weights is None else weights)


# ----------------------------------------------------------------------------- seeding

SEED_SHAPES = [(1, 1), (33, 1), (64, 64), (513, 65), (1500, 1025), (3000, 2049)]
SEED_WEIGHTS = ["uniform", "heavy_first", "heavy_middle", "heavy_last", "huge", "wide"]


def seed_weights(kind, n, pattern):
    """uniform; one vector with 99.9 % of the weight first / in the middle / last; (selectors) weights
    near 2^40, and near 2^52: at these sizes (n <= 3000, k <= 2049) it takes the latter for total * (2c + 1) to need more than 64 bits"""
    unit = 2 if kind == 1 else 1
    w = np.full(n, unit, np.uint64)
    if pattern.startswith("heavy"):
        at = {"heavy_first": 0, "heavy_middle": n // 2, "heavy_last": n - 1}[pattern]
        w[at] = unit * max(999 * (n - 1), 1)   # 999 / 1000 of the total
    elif pattern in ("huge", "wide"):
        if kind == 1:
            return None   # endpoint weights are 2 x a 32-bit group size
        rng = np.random.default_rng([40, n])
        w = (np.uint64(2 ** (40 if pattern == "huge" else 52)) - rng.integers(0, 2 ** 20, size=n).astype(np.uint64))
    return w


# ----------------------------------------------------------------------------- assignment on integer centroids

ASSIGN_N = [1, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1025]
ASSIGN_K = [1, 2, 31, 32, 33, 63, 64, 65, 129, 300]


def centroid_index_sets(n, k, rng):
    """centroids that are data vectors: the first k (entry j is nearest to vector j: winners in every row of every tile, first and last), the last k in
    descending order, and a random subset in random order"""
    return [np.arange(k), n - 1 - np.arange(k), rng.permutation(n)[:k]]


def dead_masks(k, rng):
    """live words: a group of four rows dead, every other cluster dead, all but the last dead"""
    out = []
    if k >= 9:
        m = np.ones(k, np.uint64); m[4:8] = 0; m[k - 1] = 0; out.append(m)
    if k >= 2:
        m = np.ones(k, np.uint64); m[rng.permutation(k)[:k // 2]] = 0; out.append(m)
        m = np.zeros(k, np.uint64); m[k - 1] = 7; out.append(m)
    return out


def tie_problem(kind, seed=5):
    """Planted exact ties of the minimum distance (1): between the two half-waves of one tile (rows whose bit 2 differs), between tiles, and both at once.
    Returns the problem, the centroid indices (65 rows + filler = 3 tiles), and the indices of the vectors that carry the ties."""
    rng = np.random.default_rng([seed, kind])
    v = MAX_VALUE[kind] // 2 + 1
    bases = [[v, v, v, v, v, v], [v, 0, v, 0, v, 0], [0, v, 0, v, 0, v], [v, v, 0, 0, v, v]]

    def moved(b, d, by):
        c = list(b); c[d] += by
        return key_of(kind, c)
    # (base, row of the +e_d neighbour, row of the -e_d neighbour, d)
    plan = [(0, 1, 5, 0), (0, 33, None, 1),       # base 0: rows 1 | 5 (one tile, two halves) | 33 (next tile): a three-way tie
            (1, 2, 66, 0),                        # base 1: tile 0 against tile 2
            (2, 9, 13, 1),                        # base 2: rows 9 | 13: halves of tile 0, different groups of four
            (3, 40, 44, 4)]                       # base 3: rows 40 | 44: halves of tile 1
    rows = {}
    for b, r_plus, r_minus, d in plan:
        rows[r_plus] = moved(bases[b], d, +1)
        if r_minus is not None:
            rows[r_minus] = moved(bases[b], d, -1)
    base_keys = [key_of(kind, b) for b in bases]
    planted = set(rows.values()) | set(base_keys)
    assert len(planted) == len(rows) + len(bases)
    n, k = 200, 80
    # distinct integer vectors are at least 1 apart, so the planted neighbours ARE nearest; a random vector can only add to a tie
    other = [int(x) for x in random_keys(kind, n - len(planted), rng, exclude=planted)]
    prob = Problem(kind, sorted(planted) + other, small_weights(kind, n, rng))
    filler = [int(i) for i in prob.index_of(np.array(other[:k], prob.keys.dtype))]
    cen = []
    for r in range(k):
        cen.append(int(prob.index_of([rows[r]])[0]) if r in rows else filler[r])
    return prob, np.array(cen), prob.index_of(np.array(base_keys, prob.keys.dtype))


def zero_problem(kind, seed=6):
    """The all-zero vector as a centroid (its comparison key is exactly 0.0 for every vector: the tagged keys are denormals), not in the first group of four
    rows, with its neighbours e_d and the zero vector itself among the vectors. Returns problem, centroid indices, indices of zero vector + neighbours."""
    rng = np.random.default_rng([seed, kind])
    near = [0] + [key_of(kind, [0] * d + [1]) for d in range(DIMS[kind])]
    n, k, row = 150, 70, 46   # row 46 = tile 1, rows 44..47: group 1, upper half
    other = [int(x) for x in random_keys(kind, n - len(near), rng, exclude=near)]
    prob = Problem(kind, near + other, small_weights(kind, n, rng))
    vec_other = prob.vec[prob.index_of(np.array(other, prob.keys.dtype))]
    far = [o for o, u in zip(other, vec_other) if (u * u).sum() > 2 * u.max() + 2][:k - 1]   # key |c|^2 - 2 c_d > 0 for every neighbour
    cen = [int(i) for i in prob.index_of(np.array(far, prob.keys.dtype))]
    cen.insert(row, int(prob.index_of([0])[0]))
    return prob, np.array(cen), prob.index_of(np.array(near, prob.keys.dtype))


# ----------------------------------------------------------------------------- assignment on fractional centroids

FRACTIONAL_SHAPES = [(513, 65), (1025, 300)]
FRACTIONAL_SEED = {0: 11, 1: 11}


def fractional_problem(kind, n, k):
    """centroids = float32 means of 3, 5, 6 or 7 random vectors (never a power of two: both f16 halves of -2c are non-zero)"""
    prob = random_problem(kind, n, FRACTIONAL_SEED[kind])
    rng = np.random.default_rng([FRACTIONAL_SEED[kind], kind, n, k])
    cen = np.zeros((k, 16), np.float32)
    for c in range(k):
        members = rng.permutation(n)[:rng.choice([3, 5, 6, 7])]
        cen[c] = (prob.vec[members].sum(axis=0).astype(np.float64) / members.size).astype(np.float32)
    return prob, cen


# ----------------------------------------------------------------------------- sums

def boundary_problem(kind, over):
    """k = 1, every vector holds the largest value in components 2 (low half of a packed word) and 3 (its high half). over = False: the total weight is the
    largest with total * value < 2^32 (packed; the low half one step from carrying); over = True: the next possible total (must not be packed)."""
    v, unit = MAX_VALUE[kind], (2 if kind == 1 else 1)
    total = (2 ** 32 - 1) // v // unit * unit
    if over:
        total += unit
    assert (total * v >= 2 ** 32) == over
    n = 40
    rng = np.random.default_rng([7, kind])
    keys = set()
    while len(keys) < n:
        c = [int(x) for x in rng.integers(0, v, size=DIMS[kind])]   # below the largest value
        c[2] = c[3] = v
        keys.add(key_of(kind, c))
    w = np.full(n, unit, np.uint64)
    w[n // 3] = total - unit * (n - 1)
    return Problem(kind, sorted(keys), w), total


def unpacked_weights(kind, n, rng):
    """selector weights near 2^31, endpoint group sizes near 10^6: total * largest value >= 2^32"""
    if kind == 0:
        return (np.uint64(2 ** 31) - rng.integers(0, 1000, size=n).astype(np.uint64))
    return np.uint64(2) * (np.uint64(10 ** 6) - rng.integers(0, 1000, size=n).astype(np.uint64))


def colliding_ids(k, slots=3, least=6):
    """cluster ids below k that share their first slot (c * 2654435761 mod 2^32) >> 24 of the workgroup's 256-slot table: the ids of `slots` such slots"""
    c = np.arange(k, dtype=np.uint64)
    h = ((c * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
    out = []
    for s in np.argsort(-np.bincount(h.astype(np.int64), minlength=256), kind="stable")[:slots]:
        ids = np.nonzero(h == s)[0]
        assert ids.size >= least
        out.append(ids)
    return out


# ----------------------------------------------------------------------------- update and reseed

def far_centroid(kind):
    """an integer centroid far from every vector (exact in f16 after the doubling)"""
    c = np.zeros(16, np.float32)
    c[:DIMS[kind]] = 40.0 if kind == 0 else 1000.0
    return c


RESEED_CASES = {
    # name: (n, k, indices of the far (= empty) centroids, plant equal worst keys in the first two groups)
    "fewer_empty_than_groups": (1500, 20, [0, 19], False),
    "more_empty_than_groups": (600, 12, [0, 3, 4, 8, 11], False),
    "no_empty": (600, 8, [], False),
    "k_above_1024": (1500, 1100, [0, 1030, 1099], False),
    "equal_worst_keys": (1100, 16, [2, 9, 15], True),
}


def reseed_problem(kind, name):
    n, k, far, equal = RESEED_CASES[name]
    rng = np.random.default_rng([8, kind, n, k])
    prob = random_problem(kind, n, 8)
    cen = prob.vec[rng.permutation(n)[:k]].astype(np.float32)
    cen[far] = far_centroid(kind)
    if equal:
        # one vector of group 0 and one of group 1 get weights that make their keys bd * w equal and the largest of their groups
        bd = R.distances(prob.vec, R.gemm_centroids(cen)).min(axis=1)
        a = int(np.argmax(bd[:512])); b = 512 + int(np.argmax(bd[512:1024]))
        unit = 2 if kind == 1 else 1
        w = prob.weights.copy()
        w[a], w[b] = unit * 64 * int(bd[b]), unit * 64 * int(bd[a])
        prob = Problem(kind, prob.keys, w)
    return prob, cen, far
