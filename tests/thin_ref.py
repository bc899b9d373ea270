"""fp64 reference of Stein thinning (a helper of the thinning tests, not a test; include/steinhip.h, stein_thin).

With c2 = 2 h2, D = |x - y|^2, cross = (g_x - g_y).(x - y), gg = g_x.g_y, all from the differences:

    imq  k = (1 + D / c2)^(-1/2):  u_p = k gg + k^3 cross / c2 + d k^3 / c2 - 3 k^5 D / c2^2,   u_p(j, j) = |g_j|^2 + d / c2
    rbf  k = exp(-D / c2):         u_p = k (gg + cross / h2 + d / h2 - D / h2^2),               u_p(j, j) = |g_j|^2 + d / h2
    obj_t[j] = u_p(j, j) / 2 + sum_{i < t} u_p(x_{s_i}, x_j),   s_t = argmin_j obj_t[j] (np.argmin: the lowest index),
    S_t = S_{t-1} + 2 obj_t[s_t],   KSD^2_V of the first t picks = S_t / t^2

`greedy` is that loop.  An argmin cannot be compared index by index -- one near-tie would change every later pick -- so the
GPU's picks are checked TEACHER-FORCED (`teacher_forced`): given its own sequence s_1 .. s_m, obj_t is recomputed in fp64
for every t and the pick must be within allow_t of the minimum; where the fp64 runner-up lies more than 4 allow_t above
the minimum (a DECISIVE step) the pick must be the fp64 argmin itself.

The allowance (u = 2^-24, gamma_k = k u; X, G and h2 are fp32 values, so the differences are formed from exact inputs).
It is a forward bound on ONE fp32 evaluation of u_p(s, j) by the formulas above, for any order of the sums:
  - a difference is one rounding (1 + delta), |delta| <= u.  D is a sum of d non-negative squares: |D^ - D| <= gamma_{d+2} D.
    cross and gg are sums of d products: |C^ - cross| <= gamma_{d+2} A_c, A_c = sum_c |dg_c| |dx_c|;
    |G^ - gg| <= gamma_d A_g, A_g = sum_c |g_sc| |g_jc|.
  - rsqrt and exp are taken as within 2 ulp: 4 u relative (the device library documents 1 ulp for both).
  - imq: b = 1 + D^ / c2 >= 1 carries gamma_{d+4} relative, so k^ = k (1 + kappa), |kappa| <= gamma_{d+4} / 2 + 4 u; k^3 carries
    3 kappa + 2 u and k^5 5 kappa + 4 u.  The four terms, each with its own roundings, against their magnitudes:
        k A_g            (kappa + u + gamma_d)
        k^3 A_c / c2     (3 kappa + 4 u + gamma_{d+2})
        d k^3 / c2       (3 kappa + 4 u)
        3 k^5 D / c2^2   (5 kappa + 8 u + gamma_{d+2})
    and three additions, 3 u M with M the sum of the four magnitudes.
  - rbf: e = D^ / c2 carries gamma_{d+3}, so kappa <= e gamma_{d+3} + 4 u (it grows with the distance, as k falls).  The bracket's
    terms: A_g gamma_d, (A_c / h2) gamma_{d+3}, (d / h2) u, (D / h2^2) gamma_{d+4}, three additions 3 u M' (M' their magnitudes'
    sum) and the product with k^: (kappa + u) M'.
  - second-order terms: the sum is multiplied by 1.01 (d u < 2^-10 for every d a test uses).
u_p(j, j) / 2 is taken in fp64, a sum of d squares in any order: (d + 4) 2^-53 of it.  The objective is summed in fp64: one
conversion and one addition per pick, 2^-50 of the magnitudes covers them.  So with
    A_t[j] = (d + 4) 2^-53 u_p(j, j) / 2 + sum_{i < t} allowance(s_i, j)
the computed obj_t[j] is within A_t[j] of the fp64 value, the pick s_t satisfies
obj_t[s_t] - min_j obj_t[j] <= A_t[s_t] + A_t[argmin] <= allow_t := 2 max_j A_t[j], and S_t is within
2 sum_{t' <= t} A_t'[s_t'] of the fp64 S of the same picks.  Nothing here was fitted to the kernel; the largest error over
allowance the MI355X showed is recorded in DESIGN.md section 6g.
"""
import math

import numpy as np

U32 = 2.0 ** -24
KERNELS = ("imq", "rbf")


def f32(x):
    return float(np.float32(x))


def median_h2(X):
    """the median-heuristic bandwidth^2 in fp64: median of all n^2 squared distances (the mean of the middle two for an
    even count) over ln n, rounded to fp32 as the library holds it"""
    X = np.asarray(X, np.float64)
    diff = X[:, None, :] - X[None, :, :]
    D = np.sort((diff * diff).sum(-1).reshape(-1))
    c = D.size
    med = D[c // 2] if c % 2 else 0.5 * (D[c // 2 - 1] + D[c // 2])
    return f32(med / math.log(X.shape[0]))


def diag_half(G, h2, kernel):
    """u_p(j, j) / 2 for every j"""
    G = np.asarray(G, np.float64)
    d = G.shape[1]
    return 0.5 * ((G * G).sum(1) + d / (2.0 * h2 if kernel == "imq" else h2))


def stein_row(X, G, s, h2, kernel):
    """(u_p(x_s, x_j), magnitude M, allowance) for every j: fp64 value, the sum of its terms' magnitudes, and the forward
    fp32 bound of the module docstring"""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    d = X.shape[1]
    dx, dg = X[s][None, :] - X, G[s][None, :] - G
    D = (dx * dx).sum(1)
    cross, A_c = (dg * dx).sum(1), (np.abs(dg) * np.abs(dx)).sum(1)
    gg, A_g = G @ G[s], np.abs(G) @ np.abs(G[s])
    c2 = 2.0 * h2
    g = lambda k: k * U32   # noqa: E731
    if kernel == "imq":
        k = (1.0 + D / c2) ** -0.5
        k3, k5 = k ** 3, k ** 5
        kappa = g(d + 4) / 2 + 4 * U32
        m1, m2, m3, m4 = k * A_g, k3 * A_c / c2, d * k3 / c2, 3.0 * k5 * D / c2 ** 2
        u = k * gg + k3 * cross / c2 + m3 - m4
        M = m1 + m2 + m3 + m4
        allow = m1 * (kappa + U32 + g(d)) + m2 * (3 * kappa + 4 * U32 + g(d + 2)) + m3 * (3 * kappa + 4 * U32) + \
            m4 * (5 * kappa + 8 * U32 + g(d + 2)) + 3 * U32 * M
    elif kernel == "rbf":
        e = D / c2
        k = np.exp(-e)
        kappa = e * g(d + 3) + 4 * U32
        m1, m2, m3, m4 = A_g, A_c / h2, d / h2 + 0.0 * D, D / h2 ** 2
        u = k * (gg + cross / h2 + d / h2 - m4)
        M = k * (m1 + m2 + m3 + m4)
        allow = k * (m1 * g(d) + m2 * g(d + 3) + m3 * U32 + m4 * g(d + 4)) + (kappa + 4 * U32) * M
    else:
        raise ValueError(kernel)
    return u, M, 1.01 * allow + 2.0 ** -50 * M


def greedy(X, G, h2, kernel, m):
    """the fp64 greedy loop -> (picks int64 [m], KSD^2_V after each pick [m])"""
    obj = diag_half(G, h2, kernel)
    picks, ksd2, S = np.empty(m, np.int64), np.empty(m), 0.0
    for t in range(m):
        s = int(np.argmin(obj))
        S += 2.0 * obj[s]
        picks[t], ksd2[t] = s, S / (t + 1.0) ** 2
        obj = obj + stein_row(X, G, s, h2, kernel)[0]
    return picks, ksd2


class Forced:
    """what teacher_forced returns, one entry per pick t = 1 .. m:
    gap       obj_t[s_t] - min_j obj_t[j]                     (>= 0)
    allow     allow_t = 2 max_j A_t[j]
    argmin    the fp64 argmin of obj_t (lowest index)
    decisive  the fp64 runner-up (the least objective at any OTHER index) lies more than 4 allow_t above the minimum
    ksd2      the fp64 S_t / t^2 of these picks;   ksd2_allow: 2 sum_{t' <= t} A_t'[s_t'] / t^2
    scale     sum over the pairs of the first t picks of u_p's magnitude M (what another implementation's V-statistic of
              the picked set is measured against)"""


def teacher_forced(X, G, h2, kernel, picks):
    picks = np.asarray(picks, np.int64)
    m, n = picks.size, np.asarray(X).shape[0]
    assert picks.min() >= 0 and picks.max() < n, "a pick outside [0, n)"
    diag = diag_half(G, h2, kernel)
    obj, A = diag.copy(), (np.asarray(X).shape[1] + 4) * 2.0 ** -53 * diag
    r = Forced()
    r.gap, r.allow, r.argmin, r.decisive = np.empty(m), np.empty(m), np.empty(m, np.int64), np.empty(m, bool)
    r.ksd2, r.ksd2_allow, r.scale = np.empty(m), np.empty(m), np.empty(m)
    S = S_allow = scale = 0.0
    hits = np.zeros(n)                       # how often each index has been picked so far
    for t in range(m):
        s = int(picks[t])
        j = int(np.argmin(obj))
        lo = obj[j]
        r.gap[t], r.argmin[t], r.allow[t] = obj[s] - lo, j, 2.0 * A.max()
        rest = np.delete(obj, j)
        r.decisive[t] = bool(rest.size == 0 or rest.min() - lo > 4.0 * r.allow[t])
        S += 2.0 * obj[s]
        S_allow += 2.0 * A[s]
        u, M, allow = stein_row(X, G, s, h2, kernel)
        scale += 2.0 * float(M @ hits) + float(M[s])
        hits[s] += 1.0
        r.ksd2[t], r.ksd2_allow[t], r.scale[t] = S / (t + 1.0) ** 2, S_allow / (t + 1.0) ** 2, scale
        obj, A = obj + u, A + allow
    return r
