"""fp64 reference of the KSD test's quadratic forms (a helper of the bootstrap tests, not a test; include/steinhip.h,
stein_ksd_boot):   Q_b = sum_ij w_bi w_bj u_p(x_i, x_j),   diag = sum_i u_p(x_i, x_i).

`pairwise_u` forms the Stein-kernel matrix U from the pairs' differences (imq: imq_ref.pairwise_u's formula; rbf:
u = k (g_i.g_j + (g_i - g_j).(x_i - x_j) / h2 + d / h2 - D / h2^2), k = exp(-D / (2 h2))), `quadratic_forms` contracts it.

The allowance is a forward bound on the arithmetic of k_ksd_boot (stein_amd/csrc/stein_boot.hip), worst case and for any
order of the sums; nothing in it was fitted to the kernel's output (DESIGN.md section 6h records the largest error over
allowance the MI355X showed).  u = 2^-24; X, G, h2 and the weights are fp32 values.

  operand planes   a value a of a matrix with largest magnitude amax is split into hi + lo fp16 at a power-of-two scale that
                   puts amax into [2^13, 2^14): |a - hi - lo| <= 2^-22 |a| + 2^-38 amax.
  Gram             three fp16 products per pair of terms (lo lo dropped: 2^-22), accumulated in fp32 over the depth K, taken as
                   a sequential chain of 3 K additions: for rows a_i, b_j
                       E_ab(i, j) = (3 K + 20) u A_ab(i, j) + 2^-37 (amax |b_j|_1 + bmax |a_i|_1),   A_ab = sum_c |a_ic| |b_jc|
  D                r_i (fp32 row norms, (d + 2) u) + r_j - 2 x_i.x_j:   E_D = 2 E_xx + (d + 8) u (r_i + r_j + 2 A_xx)
  per particle     fp32 sums of d products: (d + 8) u of the magnitudes (rbf: B_i = sum_c |g_ic x_ic| / h2 + r_i / (2 h2^2);
                   imq: a_i = sum_c |g_ic x_ic|)
  rbf              W = G - X / h2 elementwise, one fma with a rounded 1 / h2: |dW| <= u (|G| + 3 |X| / h2) = u P, which moves
                   w_i.w_j by at most T = u (P |W|^T + |W| P^T).  The bracket M' = A_ww + D / (2 h2^2) + B_i + B_j + d / h2
                   carries  E_B = E_ww + T + E_D / (2 h2^2) + 3 u D / (2 h2^2) + (d + 8) u (B_i + B_j) + 2 u d / h2 + 4 u M',
                   the exponent kappa = E_D / (2 h2) + 4 u D / (2 h2) + 4 u (exp2 within 2 ulp), and
                       a_ij = k E_B + (kappa + 2 u) k M'
  imq              t = 1 + D / c2 >= 1 carries E_D / c2 + 3 u t, so k = rsq(t) carries kappa = that / (2 t) + 4 u, k^3
                   3 kappa + 2 u, k^5 5 kappa + 4 u.  The four terms with their magnitudes m1 = k A_gg,
                   m2 = k^3 (a_i + a_j + A_x) / c2 (A_x the depth-2d cross Gram's), m3 = d k^3 / c2, m4 = 3 k^5 D / c2^2:
                       a_ij = k E_gg + (kappa + u) m1 + k^3 (E_x + (d + 8) u (a_i + a_j)) / c2 + (3 kappa + 7 u) m2
                              + (3 kappa + 4 u) m3 + 3 k^5 E_D / c2^2 + (5 kappa + 8 u) m4 + 4 u (m1 + m2 + m3 + m4)
  image            u_p times a power of two that puts the device's bound on |u_p| (`bound`) into [2^13, 2^14), hi + lo fp16:
                       a_ij += 2^-22 |u_ij| + 2^-37 bound
  contraction      the weights are split like an operand matrix (largest magnitude wmax); fp32 accumulation over the padded
                   n, sequential model; the tail multiplies by w_bi and adds 32 rows and two lane groups in fp32 (34 u); the
                   partials are added in fp64.  With M_ij >= |u_ij| the sum of the magnitudes of u_p's terms (k M' or
                   m1 + .. + m4) and scale_b = sum_ij |w_bi| |w_bj| M_ij:
                       allow_b = 1.01 [ sum_ij |w_bi| |w_bj| a_ij + (3 R + 50) u scale_b + 2^-37 wmax sum_ij |w_bi| M_ij ]
                   (R = n rounded up to 128; 1.01 for the second-order terms).
"""
import math

import numpy as np

U32 = 2.0 ** -24
KERNELS = ("imq", "rbf")


def f32(x):
    return float(np.float32(x))


def median_h2(X):
    """the median-heuristic bandwidth^2 in fp64 (median of all n^2 squared distances over ln n), rounded to fp32"""
    X = np.asarray(X, np.float64)
    r = (X * X).sum(1)
    D = np.sort(np.maximum(r[:, None] + r[None, :] - 2.0 * X @ X.T, 0.0).reshape(-1))
    c = D.size
    med = D[c // 2] if c % 2 else 0.5 * (D[c // 2 - 1] + D[c // 2])
    return f32(med / math.log(X.shape[0]))


def _pairs(X, G, block=32):
    """(D, cross, gg) of all pairs from the differences, `block` rows at a time"""
    n = X.shape[0]
    D, cross = np.empty((n, n)), np.empty((n, n))
    for i0 in range(0, n, block):
        dx = X[i0:i0 + block, None, :] - X[None, :, :]
        dg = G[i0:i0 + block, None, :] - G[None, :, :]
        D[i0:i0 + block] = (dx * dx).sum(-1)
        cross[i0:i0 + block] = (dg * dx).sum(-1)
    return D, cross, G @ G.T


def pairwise_u(X, G, h2, kernel):
    """[n, n] Stein-kernel matrix in fp64 from the differences"""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    d, c2 = X.shape[1], 2.0 * h2
    D, cross, gg = _pairs(X, G)
    if kernel == "imq":
        k = (1.0 + D / c2) ** -0.5
        return k * gg + k ** 3 * cross / c2 + d * k ** 3 / c2 - 3.0 * k ** 5 * D / c2 ** 2
    if kernel == "rbf":
        return np.exp(-D / c2) * (gg + cross / h2 + d / h2 - D / h2 ** 2)
    raise ValueError(kernel)


def diag_sum(G, h2, kernel):
    G = np.asarray(G, np.float64)
    n, d = G.shape
    return float((G * G).sum() + n * d / (2.0 * h2 if kernel == "imq" else h2))


def device_bound(X, G, h2, kernel):
    """the bound on |u_p| k_boot_scale derives (in fp64; the image's absolute error is 2^-38 of it, doubled below)"""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    d = X.shape[1]
    if kernel == "rbf":
        W = G - X / h2
        b = (G * X).sum(1) / h2 - (X * X).sum(1) / (2.0 * h2 ** 2)
        return float((W * W).sum(1).max() + 2.0 * np.abs(b).max() + (d + 1) / h2)
    c2 = 2.0 * h2
    g2 = float((G * G).sum(1).max())
    return g2 + math.sqrt(g2 / c2) + (d + 3) / c2


def _gram_err(A, B, depth):
    """E_ab of the module docstring for the rows of A against the rows of B"""
    aa, bb = np.abs(A), np.abs(B)
    return (3 * depth + 20) * U32 * (aa @ bb.T) + 2.0 ** -37 * (aa.max() * bb.sum(1)[None, :] + bb.max() * aa.sum(1)[:, None])


def element_model(X, G, h2, kernel):
    """(U, M, a): the fp64 Stein-kernel matrix, the magnitudes M_ij >= |u_ij| of its terms as the kernel forms them, and the
    per-element allowance a_ij of the module docstring"""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    n, d = X.shape
    dk = (d + 31) // 32 * 32
    c2 = 2.0 * h2
    U = pairwise_u(X, G, h2, kernel)
    r = (X * X).sum(1)
    aX = np.abs(X)
    A_xx = aX @ aX.T
    D = np.maximum(r[:, None] + r[None, :] - 2.0 * X @ X.T, 0.0)
    E_xx = _gram_err(X, X, dk)
    rr = r[:, None] + r[None, :]
    E_D = 2.0 * E_xx + (d + 8) * U32 * (rr + 2.0 * A_xx)
    agx = (np.abs(G) * aX).sum(1)
    if kernel == "rbf":
        W = G - X / h2
        aW = np.abs(W)
        P = np.abs(G) + 3.0 * aX / h2
        T = U32 * (P @ aW.T + aW @ P.T)
        B = agx / h2 + r / (2.0 * h2 ** 2)
        BB = B[:, None] + B[None, :]
        k = np.exp(-D / c2)
        Mb = aW @ aW.T + D / (2.0 * h2 ** 2) + BB + d / h2
        E_B = _gram_err(W, W, dk) + T + E_D / (2.0 * h2 ** 2) + 3 * U32 * D / (2.0 * h2 ** 2) + (d + 8) * U32 * BB + \
            2 * U32 * d / h2 + 4 * U32 * Mb
        kappa = E_D / c2 + 4 * U32 * D / c2 + 4 * U32
        M = k * Mb
        a = k * E_B + (kappa + 2 * U32) * M
    elif kernel == "imq":
        aG = np.abs(G)
        t = 1.0 + D / c2
        k = t ** -0.5
        k3, k5 = k ** 3, k ** 5
        kappa = (E_D / c2 + 3 * U32 * t) / (2.0 * t) + 4 * U32
        aa = agx[:, None] + agx[None, :]
        A_x = aX @ aG.T + aG @ aX.T
        E_x = _gram_err(np.hstack([G, X]), np.hstack([X, G]), 2 * dk)
        m1, m2, m3, m4 = k * (aG @ aG.T), k3 * (aa + A_x) / c2, d * k3 / c2, 3.0 * k5 * D / c2 ** 2
        M = m1 + m2 + m3 + m4
        a = k * _gram_err(G, G, dk) + (kappa + U32) * m1 + k3 * (E_x + (d + 8) * U32 * aa) / c2 + (3 * kappa + 7 * U32) * m2 + \
            (3 * kappa + 4 * U32) * m3 + 3.0 * k5 * E_D / c2 ** 2 + (5 * kappa + 8 * U32) * m4 + 4 * U32 * M
    else:
        raise ValueError(kernel)
    a = a + 2.0 ** -22 * np.abs(U) + 2.0 ** -37 * device_bound(X, G, h2, kernel)
    return U, M, a


class Forms:
    """what `quadratic_forms` returns:  q [reps] the fp64 Q_b;  diag the fp64 sum_i u_ii;  scale [reps] sum_ij |w_bi| |w_bj|
    M_ij;  allow [reps] the allowance of the module docstring"""


def quadratic_forms(X, G, h2, kernel, weights):
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    Wt = np.asarray(weights, np.float64)
    n = X.shape[0]
    R = (n + 127) // 128 * 128
    U, M, a = element_model(X, G, h2, kernel)
    aw = np.abs(Wt)
    f = Forms()
    f.q = ((Wt @ U) * Wt).sum(1)
    f.diag = diag_sum(G, h2, kernel)
    awM = aw @ M
    f.scale = (awM * aw).sum(1)
    f.allow = 1.01 * (((aw @ a) * aw).sum(1) + (3 * R + 50) * U32 * f.scale + 2.0 ** -37 * aw.max() * awM.sum(1))
    return f


def sign_rows(reps, n, seed, flip_prob=0.5):
    """[reps, n] fp32 sign processes: first entry +-1, each next one the previous times -1 with probability flip_prob"""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, 2, (reps, 1))
    flips = (rng.random((reps, n - 1)) < flip_prob).astype(np.int64)
    return (1 - 2 * (np.concatenate([first, flips], 1).cumsum(1) & 1)).astype(np.float32)


def p_value(q):
    """(1 + #{b >= 1 : Q_b >= Q_0}) / reps for q = [Q_0, Q_1 .. Q_B] (reps = B + 1 rows, the statistic's first)"""
    q = np.asarray(q)
    return (1.0 + float((q[1:] >= q[0]).sum())) / q.size


def undecided(q, allow):
    """how many replicates lie within 4 x (their allowance + the statistic's) of Q_0"""
    q, allow = np.asarray(q), np.asarray(allow)
    return int((np.abs(q[1:] - q[0]) <= 4.0 * (allow[1:] + allow[0])).sum())
