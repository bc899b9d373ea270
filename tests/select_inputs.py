"""Tie-heavy and straddling inputs of the median select, and the exact references they are judged by (a helper of
test_select_inputs.py, test_gpu_select_images.py and test_gpu_select_lattice.py, not a test).

Two kinds of input:

    lattices   particles with small integer coordinates: every squared distance is an integer that every distance path
               computes exactly, so the expected order statistics come from an int64 D and no GPU output enters them
               line       d = 1, theta_i = i mod m: m distinct distances, both targets deep inside one huge tie
               grid       d = 2, (i mod 37, i // 37): hundreds of distinct values, lo == hi
               two        half the particles at the origin, half at (3, 3): lo = 0 | hi = 18, the diagonal inside lo's tie
               simplex4   d = 5, four clusters: the target ranks sit exactly on the seam of two adjacent tied values
               identical  every distance 0
               scatter    d = 2, seeded random integer points in [0, 200]^2: twelve thousand distinct distances in ties of a
                          hundred, the seed chosen so that the two targets lie on DIFFERENT values (10600 | 10601 at n = 768,
                          1024 keys apart: both inside the 8192-key window, in different high bytes of it)
    images     fp32 matrices written directly (no particles behind them) for the staged select, which takes the distance
               image as an argument: adjacent keys either side of a bin edge of each radix level, negatives and both
               zeros, denormals to +inf, and three-valued ties with the targets at the first / an interior / the last
               position of a tie

The references sort: exact_median on fp32 values (NumPy), lattice_median on the int64 D.  The key function and
diverge_level only CLASSIFY inputs (which branch of the select they reach); no expectation is computed from them.
"""
import numpy as np

from oracle import svgd_oracle as orc

SPEC_CAP = (1 << 21) - 2048     # entries of the window buffer: a copy of SPEC_CAP, stein_amd/csrc/stein_common.h:182


# ---- keys (classification only) ---------------------------------------------------------------------------------
def f32_key(x):
    """order-preserving uint32 key of fp32 values: ~u if the sign bit is set, otherwise u | 0x80000000"""
    x = np.asarray(x, dtype=np.float32)
    u = np.ascontiguousarray(x).reshape(-1).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32).reshape(x.shape)


def key_f32(k):
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return u.reshape(-1).view(np.float32).reshape(k.shape)


def diverge_level(lo, hi):
    """the radix level (11 + 11 + 10 key bits) at which the two targets part: "same", "L0", "L1" or "L2" """
    a, b = int(f32_key(np.float32(lo))), int(f32_key(np.float32(hi)))
    if a == b:
        return "same"
    if a >> 21 != b >> 21:
        return "L0"
    if a >> 10 != b >> 10:
        return "L1"
    return "L2"


# ---- references ---------------------------------------------------------------------------------------------------
def target_ranks(total):
    """0-based ascending ranks of the two median targets (compute_median.py:12-15)"""
    return (total // 2 - 1, total // 2) if total % 2 == 0 else (total // 2, total // 2)


def exact_median(values_f32, weights=None):
    """(lo, hi, med) of fp32 values by an exact sort; weights: positive integer multiplicities.  med = 0.5f * (lo + hi)
    in fp32 for an even count (the arithmetic of median_bandwidth, stein_common.h:205), lo for an odd one."""
    v = np.asarray(values_f32, dtype=np.float32).reshape(-1)
    assert not np.isnan(v).any()
    if weights is None:
        s = np.sort(v)
        r0, r1 = target_ranks(s.size)
        lo, hi = s[r0], s[r1]
    else:
        w = np.asarray(weights, dtype=np.int64).reshape(-1)
        order = np.argsort(v, kind="stable")
        s, cum = v[order], np.cumsum(w[order])
        r0, r1 = target_ranks(int(cum[-1]))
        lo, hi = s[np.searchsorted(cum, r0, side="right")], s[np.searchsorted(cum, r1, side="right")]
    with np.errstate(invalid="ignore", over="ignore"):
        med = np.float32(0.5) * (lo + hi) if r0 != r1 else lo
    return np.float32(lo), np.float32(hi), np.float32(med)


def bandwidth(med, n):
    """h^2 of the reference's graph for this median (NaN for a negative one)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.float32(orc.bandwidth_sq(np.float32(med), n, np.float32))


def with_stray_low(values_f32, k):
    """(lo, hi) a select returns that counted k entries BELOW every value besides the values (a pass that read padding
    holding a low sentinel): the ranks stay those of the true total"""
    s = np.sort(np.asarray(values_f32, dtype=np.float32).reshape(-1))
    r0, r1 = target_ranks(s.size)
    return (np.float32(-np.inf) if r0 < k else s[r0 - k]), (np.float32(-np.inf) if r1 < k else s[r1 - k])


def multiplicity(values, x, weights=None):
    """how many entries (how much weight) equal x; +0.0 and -0.0 count as equal, as they do in a sort"""
    eq = np.asarray(values).reshape(-1) == x
    return int(eq.sum()) if weights is None else int(np.asarray(weights).reshape(-1)[eq].sum())


def lattice_D(P):
    """int64 squared distances of integer particles [n, d]"""
    P = np.asarray(P, dtype=np.int64)
    D = np.zeros((P.shape[0], P.shape[0]), dtype=np.int64)
    for k in range(P.shape[1]):                        # ((a - b) ** 2).sum(), a coordinate at a time
        D += (P[:, None, k] - P[None, :, k]) ** 2
    return D


class LatticeRef:
    """exact order statistics of the n^2 integer distances: lo / hi (ints), their multiplicities, med and h2 (fp32)"""

    def __init__(self, P):
        self.P = np.asarray(P, dtype=np.int64)
        self.n = self.P.shape[0]
        self.D = lattice_D(self.P)
        every = np.bincount(self.D.reshape(-1))                           # a counting sort of the n^2 integers
        vals = np.flatnonzero(every)
        counts = every[vals]
        cum = np.cumsum(counts)
        r0, r1 = target_ranks(self.n * self.n)
        i0, i1 = np.searchsorted(cum, r0, side="right"), np.searchsorted(cum, r1, side="right")
        self.lo, self.hi = int(vals[i0]), int(vals[i1])
        self.mult_lo, self.mult_hi = int(counts[i0]), int(counts[i1])
        self.distinct = int(vals.size)
        assert max(abs(self.lo), abs(self.hi)) < 1 << 24                  # exact as fp32
        self.med = np.float32(0.5) * (np.float32(self.lo) + np.float32(self.hi)) if r0 != r1 else np.float32(self.lo)
        self.h2 = bandwidth(self.med, self.n)
        # the fused single-rank call buffers the upper triangle's entries inside the window, one per entry
        self.upper_mult_lo = int((np.triu(self.D == self.lo)).sum())


# ---- lattice families ------------------------------------------------------------------------------------------
def line(n, m=9):
    return (np.arange(n, dtype=np.int64) % m).reshape(n, 1)


def grid(n, w=37):
    i = np.arange(n, dtype=np.int64)
    return np.stack([i % w, i // w], axis=1)


def two(n):
    P = np.zeros((n, 2), dtype=np.int64)
    P[n // 2:] = 3
    return P


def simplex4(n, off, step, seed=0):
    assert n % 4 == 0
    c = np.arange(n) % 4
    P = np.zeros((n, 5), dtype=np.int64)
    P[np.arange(n), c] = off
    P[:, 4] = step * (c >= 2)
    return P[np.random.default_rng([seed, n, off, step]).permutation(n)]


def identical(n):
    return np.tile(np.array([[2, 1, 3]], dtype=np.int64), (n, 1))


SCATTER_SEED = {768: 23, 1536: 39}      # found by trying seeds 0, 1, ... until lo != hi (test_select_inputs.py asserts it)


def scatter(n, seed, extent=200):
    return np.random.default_rng([seed, n, 11]).integers(0, extent + 1, size=(n, 2)).astype(np.int64)


def lattice(name, n):
    """the families by the names the GPU tests use"""
    if name == "scatter":
        return scatter(n, SCATTER_SEED[n])
    if name == "line":
        return line(n, 9)
    if name == "grid":
        return grid(n, 37)
    if name == "two":
        return two(n)
    if name == "identical":
        return identical(n)
    if name.startswith("simplex4_"):
        off, step = (int(x) for x in name.split("_")[1:])
        return simplex4(n, off, step, seed=n)
    raise ValueError(name)


SIMPLEX = ("simplex4_128_1", "simplex4_128_2", "simplex4_64_1", "simplex4_8_1")

# the particle counts of the GPU tests, by select path (test_gpu_select_lattice.py)
SMALL_N = (7, 8, 129, 160)          # the one-kernel path's LDS select
SOLO_N = (129, 384, 512)            # solo_select, then the single-rank window
HIST_ALL_N = (768, 1001, 2304)      # k_hist_all (2304: line only)
STEAL_CASES = (("simplex4_128_1", 2304),)
WINDOW_N = (768, 1536)              # k_spec_select
RANK_N = (768,)                     # tally / pick over two row blocks, and the staged calls
OVER_CAPACITY = (("two", 3072), ("identical", 2304))
PANEL_N = (384, 512, 768, 1536, 2304, 3072)   # every multiple of 128 above: the staged calls behind the forced panel kernel


def families_at(n):
    out = ["line", "grid"]
    if n % 2 == 0:
        out.append("two")
    if n % 4 == 0:
        out.extend(SIMPLEX)
    if n in SCATTER_SEED:
        out.append("scatter")
    return out + ["identical"]


def lattice_cases():
    """every (family, n) a GPU test runs"""
    cases = set(STEAL_CASES) | set(OVER_CAPACITY)
    for n in SMALL_N + SOLO_N + HIST_ALL_N + WINDOW_N + RANK_N:
        cases |= {(f, n) for f in (families_at(n) if n != 2304 else ["line"])}
    for n in PANEL_N:
        cases |= {(f, n) for f in families_at(n)}
    return sorted(cases)


_REFS = {}


def lattice_ref(name, n):
    """LatticeRef of lattice(name, n), computed once per process and shared"""
    if (name, n) not in _REFS:
        _REFS[(name, n)] = LatticeRef(lattice(name, n))
    return _REFS[(name, n)]


def gaussian_scores(n, d, seed=0):
    return np.random.default_rng([seed, n, d, 41]).normal(size=(n, d)).astype(np.float32)


# ---- image families: sorted (value, weight) lists ------------------------------------------------------------------------
# every family returns its distinct fp32 values in ascending order with integer weights that sum to `total`
ADJ_HI_KEY = {0: 0xC0000000, 1: 0xC0000000 + 5 * (1 << 10), 2: 0xC0000000 + 5 * (1 << 10) + 7}   # around 2.0f
IMAGE_FAMILIES = ("adjacent0", "adjacent1", "adjacent2", "negative", "wide", "ties_first", "ties_interior", "ties_last")
NEGATIVES = (-1e-6, -3e-7, -1e-7, -3e-8, -1e-8, -1e-9)


def _half(total):
    """weight at or below the lower target for the two targets to sit either side of a seam (odd total: the one target is
    the last entry at or below the seam)"""
    return total // 2 if total % 2 == 0 else total // 2 + 1


def _deal(total, k):
    """total dealt to k parts as evenly as it goes, the first parts one larger"""
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def adjacent_weights(level, total):
    kb = ADJ_HI_KEY[level]
    a, b = key_f32(np.uint32(kb - 1)), key_f32(np.uint32(kb))
    low, high = _half(total), total - _half(total)
    wu, wv = low // 3, high // 3                       # a far value on either side: other bins are populated too
    return [(np.float32(0.5), wu), (np.float32(a), low - wu), (np.float32(b), high - wv), (np.float32(8.0), wv)]


def negative_weights(total):
    neg = max(total * 5 // 8, total // 2 + 1)
    rest = total - neg
    zeros = [1 if rest >= 1 else 0, 1 if rest >= 2 else 0]
    pos = _deal(rest - sum(zeros), 4)
    vals = list(NEGATIVES) + [-0.0, 0.0, 1e-9, 1e-6, 0.5, 2.0]
    return [(np.float32(v), w) for v, w in zip(vals, _deal(neg, len(NEGATIVES)) + zeros + pos)]


WIDE_VALUES = tuple([1e-45, 1e-40, float(np.finfo(np.float32).tiny)] + [2.0 ** e for e in range(-30, 31, 4)] + [float("inf")])


def wide_weights(total):
    return [(np.float32(v), w) for v, w in zip(WIDE_VALUES, _deal(total, len(WIDE_VALUES)))]


TIE_KEYS = (0xC0400000, 0xC0400001, 0xC0400001 + (3 << 10))      # 3.0f, the next float, one three level-1 digits on


def ties_weights(position, total):
    r0, r1 = target_ranks(total)
    w2 = min(total // 4 + 2, total)
    if position == "first":            # the lower target is the first entry of the middle tie
        w1 = r0
    elif position == "last":           # the upper target is its last entry
        w1 = r1 + 1 - w2
    else:
        w1, w2 = total // 4, total // 2 + 1
    w1 = min(max(w1, 0), total - w2)
    v = key_f32(np.array(TIE_KEYS, dtype=np.uint32))
    return [(np.float32(v[0]), w1), (np.float32(v[1]), w2), (np.float32(v[2]), total - w1 - w2)]


def image_weights(family, total):
    if family.startswith("adjacent"):
        vw = adjacent_weights(int(family[-1]), total)
    elif family == "negative":
        vw = negative_weights(total)
    elif family == "wide":
        vw = wide_weights(total)
    else:
        vw = ties_weights(family.split("_")[1], total)
    assert sum(w for _, w in vw) == total and all(w >= 0 for _, w in vw)
    return [(v, w) for v, w in vw if w > 0]


def image_rect(family, rows, cols, seed=0):
    """row-major fp32 [rows, cols] holding the family's multiset in a seeded order"""
    vw = image_weights(family, rows * cols)
    flat = np.repeat(np.array([v for v, _ in vw], dtype=np.float32), [w for _, w in vw])
    np.random.default_rng([seed, rows, cols]).shuffle(flat)
    return flat.reshape(rows, cols)


def _sym_fill(n, upper_vw, diag_vw, seed):
    up = np.repeat(np.array([v for v, _ in upper_vw], dtype=np.float32), [w for _, w in upper_vw])
    dg = np.repeat(np.array([v for v, _ in diag_vw], dtype=np.float32), [w for _, w in diag_vw])
    assert up.size == n * (n - 1) // 2 and dg.size == n
    rng = np.random.default_rng([seed, n, 7])
    rng.shuffle(up)
    rng.shuffle(dg)
    M = np.zeros((n, n), dtype=np.float32)
    M[np.triu_indices(n, 1)] = up
    M = M + M.T                                       # (0 + x: exact, and -0.0 + 0 only loses a sign off the stored triangle)
    M[np.triu_indices(n, 1)] = up                     # ... which is written again as it was
    M[np.diag_indices(n)] = dg
    return M


def image_sym(family, n, seed=0):
    """symmetric fp32 [n, n] whose n^2 entries hold the family's multiset: every value's weight w is split into j diagonal
    entries and (w - j) / 2 entries above the diagonal (and their mirror images).  The diagonal goes to the targets' own
    values first, so that the target ranks fall inside a tie that contains weight-1 and weight-2 entries."""
    vw = image_weights(family, n * n)
    vals = np.array([v for v, _ in vw], dtype=np.float32)
    w = np.array([x for _, x in vw], dtype=np.int64)
    lo, hi, _ = exact_median(vals, w)
    j = w % 2
    left = n - int(j.sum())
    assert left >= 0 and left % 2 == 0
    first = [i for i in range(len(vw)) if vals[i] == lo or vals[i] == hi]
    for i in first + [i for i in range(len(vw)) if i not in first]:
        add = min(left, int(w[i] - j[i]))             # (even)
        j[i] += add
        left -= add
    assert left == 0
    return _sym_fill(n, [(v, int(k)) for v, k in zip(vals, (w - j) // 2)], [(v, int(k)) for v, k in zip(vals, j)], seed)


def sym_feasible(family, n):
    """can the family's weights be split into n diagonal entries and pairs?  (n = 2 holds too few odd weights)"""
    return sum(w % 2 for _, w in image_weights(family, n * n)) <= n


RECT_SHAPES = ((1, 33), (127, 95), (128, 32), (129, 1000), (300, 1001), (640, 1536))
SYM_SIZES = (2, 33, 128, 129, 257, 1000, 1536)
SYM_CASES = tuple((f, n) for n in SYM_SIZES for f in IMAGE_FAMILIES if sym_feasible(f, n))

DIAG_VALUE, DIAG_BELOW, DIAG_ABOVE = np.float32(5.0), np.float32(1.25), np.float32(9.0)


def image_own_diagonal(n, seed=0):
    """symmetric [n, n] whose diagonal holds a value of its own (5.0, weight n in all) between 1.25 and 9.0 off the diagonal.
    Even n: the diagonal's tie ENDS at the lower target (lo = 5, hi = 9): a diagonal entry counted twice makes hi 5, one
    not counted makes lo 9.  Odd n: the one target is the FIRST diagonal entry: without the diagonal's weight it is 1.25."""
    total = n * n
    below = total // 2 - n if total % 2 == 0 else total // 2           # weight below the diagonal's value
    assert below % 2 == 0 and below >= 0
    k = below // 2
    return _sym_fill(n, [(DIAG_BELOW, k), (DIAG_ABOVE, n * (n - 1) // 2 - k)], [(DIAG_VALUE, n)], seed)
