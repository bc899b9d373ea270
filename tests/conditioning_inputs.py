"""Badly scaled and degenerate inputs of the SVGD step, and the per-column yardstick they are judged by (a helper of
test_conditioning_inputs.py and test_gpu_conditioning.py, not a test).

Every generator is seeded and returns fp64 (theta, score) whose entries are exactly representable in fp32, so the fp64
oracle and a kernel fed the fp32 tensors see the same numbers.

    graded      score column c times 2^e_c, theta column c times 2^f_c: every column its own scale exponent
    zero_const  exact zero score columns 0, d // 2, d - 1; theta column 1 zero, theta column 2 constant 3.0
    spike       one score entry of 1e6; a score column of 1e-6 entries with a single 1
    far         particle FAR_ROW displaced by far * normal(d): its kernel row underflows but for the diagonal
    offset      a tight cluster away from the origin (r + r^T - 2 T T^T cancels)
    pow2        theta times 2^a and score column c times 2^(b_c): exponents move, significands do not
"""
import numpy as np

FAMILIES = ("graded", "zero_const", "spike", "far10", "far100")
FAR_ROW = 5
ZERO_THETA_COL, CONST_THETA_COL, CONST_VALUE = 1, 2, 3.0


def f32(x):
    """round through float32: the values a float32 tensor of x holds, as fp64"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _normal_pair(n, d, seed):
    rng = np.random.default_rng([seed, n, d])
    return f32(rng.normal(size=(n, d))), f32(rng.normal(size=(n, d))), rng


def neighbours_differ(e):
    """every column's exponent differs from the next column's -- in particular either side of every multiple of 16 (the
    contraction's column blocks of one wave) and of 128 (its column blocks of one workgroup)"""
    e = np.asarray(e)
    return bool(np.all(e[1:] != e[:-1]))


def blocks_differ(e):
    """no 16-column block carries the exponents of the block 16 or 128 columns further on"""
    e = np.asarray(e)
    for shift in (16, 128):
        for c0 in range(0, len(e) - shift, 16):
            m = min(16, len(e) - shift - c0)
            if m >= 2 and np.array_equal(e[c0:c0 + m], e[c0 + shift:c0 + shift + m]):
                return False
    return True


def graded_exponents(d, period, rng):
    """A seeded permutation of (c mod period) - period // 2, c < d, repaired by seeded swaps until no two neighbouring
    columns share an exponent (a plain random permutation of a multiset nearly always has such a pair)."""
    values = np.arange(d) % period - period // 2
    if d < 3:
        return rng.permutation(values)

    def clash(i):
        return (i > 0 and e[i] == e[i - 1]) or (i + 1 < d and e[i] == e[i + 1])

    for _ in range(64):                        # (a draw whose blocks coincide -- a few per cent of them -- is drawn again)
        e = rng.permutation(values)
        for _ in range(100 * d):
            bad = [c for c in range(1, d) if e[c] == e[c - 1]]
            if not bad:
                break
            c = bad[0]
            for j in rng.permutation(d):
                e[c], e[j] = e[j], e[c]
                if not (clash(c) or clash(j)):
                    break
                e[c], e[j] = e[j], e[c]
        if neighbours_differ(e) and blocks_differ(e):
            break
    assert neighbours_differ(e) and blocks_differ(e), "graded exponents: neighbouring columns or blocks coincide"
    return e


def graded(n, d, seed=0, with_exponents=False):
    T, G, rng = _normal_pair(n, d, seed)
    e = graded_exponents(d, 41, rng)          # score: 2^-20 .. 2^20
    f = graded_exponents(d, 9, rng)           # theta: 2^-4 .. 2^4
    T, G = T * 2.0 ** f, G * 2.0 ** e
    return (T, G, e, f) if with_exponents else (T, G)


def zero_score_cols(d):
    return sorted({0, d // 2, d - 1})


def zero_const(n, d, seed=0):
    T, G, _ = _normal_pair(n, d, seed)
    G[:, zero_score_cols(d)] = 0.0
    T[:, ZERO_THETA_COL] = 0.0
    T[:, CONST_THETA_COL] = CONST_VALUE
    return T, G


def spike(n, d, seed=0):
    T, G, _ = _normal_pair(n, d, seed)
    G[7, 3] = 1e6
    one = 11
    G[:, d - 2] *= 1e-6
    G[one, d - 2] = 1.0
    return T, f32(G)


def far(n, d, seed=0, far=10.0):
    T, G, rng = _normal_pair(n, d, seed)
    T[FAR_ROW] += far * rng.normal(size=d)
    return f32(T), G


def offset(n, d, seed=0):
    T, G, _ = _normal_pair(n, d, seed)
    return f32(0.5 + 0.01 * T), G


def make(family, n, d, seed=0):
    if family == "far10":
        return far(n, d, seed, 10.0)
    if family == "far100":
        return far(n, d, seed, 100.0)
    return {"graded": graded, "zero_const": zero_const, "spike": spike, "offset": offset}[family](n, d, seed)


def pow2(T, G, a, seed=0, lo=-40, hi=40):
    """(theta * 2^a, score column c * 2^(b_c), b): b a seeded pattern in [lo, hi] with differing neighbours"""
    d = T.shape[1]
    rng = np.random.default_rng([seed, d, 77])
    b = rng.integers(lo, hi + 1, size=d)
    for c in range(1, d):
        while b[c] == b[c - 1]:
            b[c] = rng.integers(lo, hi + 1)
    T2, G2 = T * 2.0 ** a, G * 2.0 ** b
    assert np.array_equal(f32(T2), T2) and np.array_equal(f32(G2), G2)     # still fp32 values: only exponents moved
    return T2, G2, b


# ---- yardsticks ------------------------------------------------------------------------------------------------
def column_errors(got, ref, skip_rows=()):
    """(relative 2-norm error of every column with a non-zero reference column, mask of those columns); columns whose
    reference is exactly zero come back as 0 and False and are the caller's to check"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if len(skip_rows):
        keep = np.setdiff1d(np.arange(ref.shape[0]), np.asarray(skip_rows))
        got, ref = got[keep], ref[keep]
    num, den = np.linalg.norm(got - ref, axis=0), np.linalg.norm(ref, axis=0)
    live = den > 0
    return np.where(live, num / np.where(live, den, 1.0), 0.0), live


def frobenius_error(got, ref):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / np.linalg.norm(ref))


def constant_theta_cols(T):
    """columns of theta that hold one value: dK vanishes there identically (sum_j K_ij (theta_i - theta_j))"""
    return np.flatnonzero(np.all(T == T[:1], axis=0))


def bf16_k_model(T, G):
    """The documented arithmetic of the bf16-input step in fp64: D, the bandwidth and exp as the fp64 oracle has them, K
    rounded ONCE to bf16 (round to nearest even), both the contraction and rowsum(K) taken from the rounded K.
    -> dict(phi, dK)"""
    from oracle import svgd_oracle as orc
    T, G = np.asarray(T, dtype=np.float64), np.asarray(G, dtype=np.float64)
    n = T.shape[0]
    D = orc.pairwise_sq_dists(T, np.float64)
    h2 = orc.bandwidth_sq(orc.median_all(D), n, np.float64)
    K = round_bf16(np.exp(-D / h2 / 2.0))
    dK = (K.sum(axis=1)[:, None] * T - K @ T) / h2
    return dict(phi=(K @ G + dK) / n, dK=dK)


def round_bf16(x):
    """fp64 -> nearest bf16 (ties to even, through fp32 as the kernel does) -> fp64"""
    u = np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)
