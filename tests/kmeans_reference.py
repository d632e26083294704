"""A float64 / exact-integer statement of every step of the codebook builders' fast mode (basis_universal_amd/csrc/kmeans_kernels.hip), with no kernel
structure in it: no tiles, no tags, no half-waves, no slots. What tests/test_gpu_kmeans_kernels.py holds the kernels to; itself held to brute-force loops in
tests/test_kmeans_reference_host.py.

Vectors are (n, 16) int64 arrays (endpoint vectors: 6 components + 10 zeros), weights Python-int-safe uint64 arrays, centroids (k, 16) float32 arrays as the
device keeps them. Sums are uint64 and wrap like the device's 64-bit atomics (nothing here comes near 2^64)."""
import numpy as np

DIM = 16
GROUP = 512          # vectors per workgroup of the assignment kernel = per "worst vector" report
U24 = 2.0 ** -24     # float32 unit roundoff


# ----------------------------------------------------------------------------- key unpacking

def unpack_selectors(keys):
    """uint32 packed selector vectors, value 0 in the top two bits -> (n, 16) int64"""
    keys = np.asarray(keys, np.uint32).astype(np.int64)
    return np.stack([(keys >> (30 - 2 * d)) & 3 for d in range(DIM)], axis=1)


def unpack_endpoints(keys, group_offsets):
    """uint64 48-bit colour keys (first byte in bits 47..40) -> (n, 16) int64 with ten zero pads, and the weights 2 x group size"""
    keys = np.asarray(keys, np.uint64)
    vec = np.zeros((keys.size, DIM), np.int64)
    for d in range(6):
        vec[:, d] = ((keys >> np.uint64(40 - 8 * d)) & np.uint64(255)).astype(np.int64)
    goffs = np.asarray(group_offsets, np.int64)
    return vec, (2 * (goffs[1:] - goffs[:-1])).astype(np.uint64)


# ----------------------------------------------------------------------------- seeding

def seed_pick(weights, k):
    """pick_c = the first u with cum[u] > total * (2c + 1) // (2k), in Python integers (the product needs more than 64 bits)"""
    cum, t = [], 0
    for w in np.asarray(weights, np.uint64).tolist():
        t += int(w)
        cum.append(t)
    cum_arr = np.array(cum, dtype=object)
    out = []
    for c in range(k):
        target = t * (2 * c + 1) // (2 * k)
        lo, hi = 0, len(cum) - 1
        while lo < hi:   # cum is non-decreasing
            mid = (lo + hi) // 2
            if cum_arr[mid] > target:
                hi = mid
            else:
                lo = mid + 1
        out.append(lo)
    return np.array(out, np.int64)


def make_distinct(pick, n, k):
    """u_c = c + min(max_{j <= c}(pick_j - j), n - k): strictly ascending, the last ones capped so that they still find a vector"""
    pick = np.asarray(pick, np.int64)
    run = np.maximum.accumulate(pick - np.arange(k))
    return np.arange(k) + np.minimum(run, n - k)


def seeds(weights, n, k):
    return make_distinct(seed_pick(weights, k), n, k)


# ----------------------------------------------------------------------------- assignment

def gemm_centroids(cen):
    """The centroid the GEMM really uses: -2c split into two f16 halves, c' = -0.5 (hi + lo), carried in float64. (k, 16) float32 -> float64"""
    a = (np.float32(-2.0) * np.asarray(cen, np.float32)).astype(np.float32)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return -0.5 * (hi.astype(np.float64) + lo.astype(np.float64))


def distances(vec, cprime, live=None):
    """|u - c'|^2 in float64, (n, k); dead clusters (live word 0) at +inf"""
    u = np.asarray(vec, np.float64)
    d = ((u[:, None, :] - np.asarray(cprime, np.float64)[None, :, :]) ** 2).sum(axis=2)
    if live is not None:
        d[:, np.asarray(live) == 0] = np.inf
    return d


def integer_distances(vec, cen, live=None):
    """the same for integer-valued centroids (c' = c), in int64: exact; dead clusters at the largest int64"""
    u, c = np.asarray(vec, np.int64), np.asarray(cen, np.int64)
    d = (u * u).sum(axis=1)[:, None] - 2 * (u @ c.T) + (c * c).sum(axis=1)[None, :]
    if live is not None:
        d[:, np.asarray(live) == 0] = np.iinfo(np.int64).max
    return d


KEY_ULPS = 89       # per comparison key, in units of 2^-24 S (eps_bound's docstring)
RECOVER_ULPS = 40   # the row recovery, in units of 2^-24 d_min


def eps_bound(vec, cprime, live=None):
    """eps(u) = 2^-24 (2 * 89 * max_c S_c(u) + 40 * d_min(u)),  S_c(u) = |c'|^2 + 2 sum_d |c'_d u_d|,  d_min(u) = min_c |u - c'|^2.

    The device orders centroids by key_c = |c'|^2 - 2 c'.u = |u - c'|^2 - |u|^2, so differences of keys are differences of distances. With u = 2^-24:
      * |c'|^2: 16 products rounded once each and 15 additions, <= 16 u |c'|^2;
      * the two MFMAs add 32 exact products (f16 x f16 fits float32) to it, 32 additions; the matrix core's internal rounding is not documented, so each
        addition is allowed one whole ulp (2 u) of a partial sum, and partial sums are bounded by S_c: <= 64 u S_c;
      * the two tag bits replace the two lowest mantissa bits: <= 3 ulp <= 2^-21 |key| = 8 u |key| <= 8 u S_c;
      * second-order terms and |hi| + |lo| - |hi + lo| <= 2^-9 |hi|: a factor below 1 + 2^-7, which turns 88 into 89.
    A key is therefore off by at most 89 u S_c, and the winner of a comparison of two keys can be worse than the loser by twice that.
    The group of four rows the key names is then evaluated directly, sum (u_d - c'_d)^2 in float32: a subtraction, a product and 16 additions, <= 19 u d per
    distance, so the row taken can be worse than the group's best by 2 * 19 u d <= 40 u d_min (the group's best is within the first term of d_min).
    Nothing here was fitted to device output."""
    u = np.abs(np.asarray(vec, np.float64))
    c = np.asarray(cprime, np.float64)
    s = (c * c).sum(axis=1)[None, :] + 2.0 * (u[:, None, :] * np.abs(c)[None, :, :]).sum(axis=2)
    if live is not None:
        s[:, np.asarray(live) == 0] = 0.0
    dmin = distances(vec, cprime, live).min(axis=1)
    return U24 * (2 * KEY_ULPS * s.max(axis=1) + RECOVER_ULPS * dmin)


# ----------------------------------------------------------------------------- sums, update, reseed

def sums_from_assign(vec, weights, assign, k, dims):
    """(k, 17) uint64: sums[c][d] = sum of w u_d over the vectors assigned to c (d < dims, else 0), sums[c][16] = sum of w"""
    vec = np.asarray(vec, np.int64).astype(np.uint64)
    w = np.asarray(weights, np.uint64)
    out = np.zeros((k, 17), np.uint64)
    assign = np.asarray(assign, np.int64)
    for d in range(dims):
        np.add.at(out[:, d], assign, w * vec[:, d])
    np.add.at(out[:, 16], assign, w)
    return out


def update(sums, cen):
    """float32(float64(sum) / float64(w)); clusters without weight keep their centroid"""
    sums = np.asarray(sums, np.uint64)
    out = np.array(cen, np.float32, copy=True)
    w = sums[:, 16]
    has = w != 0
    out[has] = (sums[has, :16].astype(np.float64) / w[has].astype(np.float64)[:, None]).astype(np.float32)
    return out


def worst_of_groups(best_dist, weights):
    """per group of 512 consecutive vectors: (key, index) of the vector of largest float32(bd) * float32(w), lowest index among equals"""
    key = (np.asarray(best_dist, np.float64).astype(np.float32) * np.asarray(weights, np.uint64).astype(np.float32)).astype(np.float32)
    out = []
    for g0 in range(0, key.size, GROUP):
        i = g0 + int(np.argmax(key[g0:g0 + GROUP]))   # argmax: the first among equals
        out.append((key[i], i))
    return out


def worst_words(best_dist, weights):
    """the 64-bit words the assignment reports: float bits << 32 | ~index"""
    return np.array([(int(np.float32(kf).view(np.uint32)) << 32) | (0xFFFFFFFF - i) for kf, i in worst_of_groups(best_dist, weights)], np.uint64)


def reseed(vec, weights, best_dist, sums, cen):
    """The empty clusters (weight 0), in index order, take the groups' worst vectors, largest key first (lowest index among equal keys); only as many as there are
    groups. Returns the new centroids and live words (weight; 1 for a re-seeded cluster; 0 for one left empty)."""
    worst = sorted(worst_of_groups(best_dist, weights), key=lambda t: (-float(t[0]), t[1]))
    cen = np.array(cen, np.float32, copy=True)
    live = np.asarray(sums, np.uint64)[:, 16].copy()
    empty = np.nonzero(live == 0)[0]
    for c, (_, i) in zip(empty, worst):
        cen[c] = np.asarray(vec)[i].astype(np.float32)
        live[c] = 1
    return cen, live


def compact(assign, sums):
    """non-empty clusters, index order kept: (cluster of every vector, number of clusters)"""
    livec = np.asarray(sums, np.uint64)[:, 16] != 0
    new = np.cumsum(livec) - 1
    return new[np.asarray(assign, np.int64)].astype(np.uint32), int(livec.sum())
