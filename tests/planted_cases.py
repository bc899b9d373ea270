"""Planted inputs on which every bit of stein_ksd_boot's q_out and stein_ksd_matmul's out is known (a helper of
test_planted_cases.py and test_gpu_stein_u_elements.py, not a test).

Every row of X is the same vector x of even integers in [-4, 4], G holds integers in [-3, 3], h2 = 2, d is even.  Then

    D = 0 for every pair, so k = exp2(-0) = rsq(1) = 1 and
    u_ij = g_i.g_j + d / h2 (RBF)   or   g_i.g_j + d / (2 h2) (IMQ),

and everything the kernel forms on the way is a multiple of 1/2 (QUANTUM): w = g - x / 2 is an integer vector,
b_i = g_i.x / 2 - r / 8 with r = |x|^2 a multiple of 4 (RBF), a_i = g_i.x an even integer and the cross Gram an even integer
times 1 / 4 (IMQ), d / 2 or d / 4 with d even.  The operand planes hold small integers times a power of two (lo = 0), the
image holds u without rounding, and an fp32 sum of multiples of one quantum is exact IN ANY ORDER as long as the sum of the
magnitudes stays below 2^24 quanta -- which test_planted_cases.py proves per case for the element's terms, for the
contraction and both tails.  The weights are a row of ones plus sign rows (forms) or integers in {-2 .. 2} (products).
"""
import functools

import numpy as np

import boot_ref as B

H2 = 2.0
QUANTUM = 0.5
BUDGET = 2.0 ** 24 * QUANTUM        # a sum of magnitudes below this is exact in fp32 in any order
SHAPES = [(129, 6), (300, 34), (257, 130)]
REPS = (1, 33, 129, 257)
SPLITS = (0, 1, 2, 3)               # 0: the plan's own rule
# these rows of G are one vector of +-3 (first and second 16-row block of a wave, three row tiles): among them
# g_i.g_j = 9 d, and at d = 130 the IMQ entries 1170 + 32.5 need more than the 11 bits of the image's hi plane -- without
# them every u fits hi alone and a lost lo plane would go unseen
ALIGNED_ROWS = (3, 20, 150, 256)


@functools.lru_cache(maxsize=None)
def inputs(n, d):
    """(X, G) as fp32"""
    assert d % 2 == 0
    rng = np.random.default_rng([n, d, 4242])
    x = 2 * rng.integers(-2, 3, d)
    x[0] = 4                                   # never the zero vector
    X = np.tile(x, (n, 1)).astype(np.float32)
    G = rng.integers(-3, 4, (n, d)).astype(np.float32)
    G[[i for i in ALIGNED_ROWS if i < n]] = 3.0 * (1 - 2 * rng.integers(0, 2, d)).astype(np.float32)
    return X, G


def closed_form(G, kernel):
    """[n, n] U in fp64: exact (integers and halves)"""
    G = np.asarray(G, np.float64)
    d = G.shape[1]
    return G @ G.T + d / (H2 if kernel == "rbf" else 2.0 * H2)


@functools.lru_cache(maxsize=None)
def weights(n, reps):
    """[reps, n] fp32: a row of ones, then sign rows"""
    W = B.sign_rows(reps, n, 900 + n)
    W[0] = 1.0
    return W


@functools.lru_cache(maxsize=None)
def factors(n, reps):
    """[reps, n] fp32 integers in {-2 .. 2}, row 0 all ones"""
    V = np.random.default_rng([n, reps, 77]).integers(-2, 3, (reps, n)).astype(np.float32)
    V[0] = 1.0
    return V


def term_magnitudes(X, G, kernel):
    """[n, n]: the sum of the magnitudes of everything the element function adds up for one pair, as the kernel forms it
    (RbfBoot::u: |w_i.w_j| + |D / (2 h2^2)| + |b_i| + |b_j| + d / h2;  ImqBoot::u: |g_i.g_j| + (|a_i| + |a_j| + |cross|) / c2 +
    d / c2 + 3 D / c2^2 at k = 1)"""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    d = X.shape[1]
    r = (X * X).sum(1)
    gx = (G * X).sum(1)
    if kernel == "rbf":
        W = G - X / H2
        b = np.abs(gx / H2) + r / (2.0 * H2 ** 2)          # the two products k_boot_rows subtracts, with their magnitudes
        return np.abs(W @ W.T) + b[:, None] + b[None, :] + d / H2
    c2 = 2.0 * H2
    cross = np.abs(G @ X.T) + np.abs(X @ G.T)
    return np.abs(G @ G.T) + (np.abs(gx)[:, None] + np.abs(gx)[None, :] + cross) / c2 + d / c2


def expected_forms(U, W):
    W = np.asarray(W, np.float64)
    return ((W @ U) * W).sum(1)


def expected_products(U, V):
    return np.asarray(V, np.float64) @ U
