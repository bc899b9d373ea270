"""fp64 reference of the Stein-kernel products and the Stein importance weights (a helper of their tests, not a test;
include/steinhip.h, stein_ksd_matmul and stein_weights).  Nothing here was fitted to the kernels; the largest error over
allowance the MI355X showed is recorded in DESIGN.md section 6i.  u = 2^-24.

PRODUCTS.  out[b, i] = sum_j u_p(x_i, x_j) V[b, j]; the reference is boot_ref.pairwise_u(...) @ V.T.  The kernel is
k_ksd_boot's j loop, so boot_ref's per-entry bound a_ij and magnitudes M_ij (boot_ref.element_model) carry over; what the
quadratic forms add on top -- the outer factor w_bi and the tail's 34 u (32 rows and two lane groups added in fp32) -- is
dropped, and the result is rounded to float once (R = n rounded up to 128, vmax the largest |V|):

    allow[b, i] = 1.01 [ sum_j |V_bj| a_ij + (3 R + 50) u sum_j |V_bj| M_ij + 2^-37 vmax sum_j M_ij ] + u (|out_bi| + the bracket)

ITERATION, teacher-forced (as thin_ref.teacher_forced, for the same reason: one near-tie changes every later step).  The
device starts from the float row fl(1 / n) through the product kernel, the reference from w_0 = 1 / n in fp64, so
    A_0 = allow(V = fl(1 / n)) + |U| |fl(1 / n) - 1 / n|          (the second term is exact arithmetic on the inputs)
Given the device's own (s_t, gamma_t), w and g are replayed in fp64,
    w_t = (1 - gamma_t) w_{t-1} + gamma_t e_{s_t},   g_t = (1 - gamma_t) g_{t-1} + gamma_t U[s_t, :]
and since the device forms its row in fp32 within thin_ref.stein_row's allowance (the same device code) and updates in
fp64 by the same formula,
    A_t = (1 - gamma_t) A_{t-1} + gamma_t allowance(s_t, .) + 2^-50 (|g_t| + gamma_t M(s_t, .))
(the last term covers the roundings of 1 - gamma, of gamma u and of the fused update: 3 x 2^-53 of those magnitudes).
Step t looks at the state before it:
  - s_t is the device's argmin of its g: g_{t-1}[s_t] - min g_{t-1} <= A[s_t] + A[argmin] <= 2 max A_{t-1}
  - where the fp64 runner-up lies more than 4 x that above the minimum (a DECISIVE step), s_t is the fp64 argmin
  - gamma_t.  The device computes f^ = sum_j w_j g^_j in fp64: |f^ - f| <= A_f = sum_j w_j A_j + (n + 4 t + 8) 2^-53 sum_j w_j
    |g_j| (n additions; its w differs from the replayed one by the roundings of t updates); g^_s within A_s = A[s_t];
    u_p(s, s) = |g_s|^2 + d / c summed in fp64 in any order: A_u = (d + 8) 2^-53 u_p(s, s).  So its numerator lies in
    num +- (A_f + A_s) and its denominator in den +- (A_f + 2 A_s + A_u), with num = f - g_s, den = f - 2 g_s + u_p(s, s).
    gamma = 0 where num <= 0 or den <= 0 and min(1, num / den) elsewhere is non-decreasing in num and, for num > 0,
    non-increasing in den, so it lies between the values at (num_lo, den_hi) and (num_hi, den_lo) -- the upper end is 1 when
    num_hi > 0 and den_lo <= 0 (a tiny positive denominator), the lower end is 0 when den_lo <= 0 -- widened by 2^-50 for the
    division.
CERTIFICATE.  stats_out is taken from a fresh product of fl(w_out): g^ is within allow(V = fl(w)) + |U| |fl(w) - w| = A_g of
U w, so |f^ - w^T U w| <= sum_i w_i A_g[i] + (n + 8) 2^-53 sum_i w_i |g_i|, |min g^ - min g| <= max A_g, and the gap carries
both.  f(uniform) is the same with w = 1 / n and A_0.
"""
import numpy as np

import boot_ref as B
import thin_ref as T

U32 = 2.0 ** -24
KERNELS = ("imq", "rbf")
f32 = B.f32
median_h2 = B.median_h2


class Model:
    """boot_ref.element_model of one input, computed once: U, M, a and R = n rounded up to 128"""

    def __init__(self, X, G, h2, kernel):
        self.X, self.G, self.h2, self.kernel = np.asarray(X, np.float64), np.asarray(G, np.float64), h2, kernel
        self.n, self.d = self.X.shape
        self.U, self.M, self.a = B.element_model(X, G, h2, kernel)
        self.R = (self.n + 127) // 128 * 128

    def products(self, V):
        """(out, allow): the fp64 products [reps, n] and the allowance of the module docstring"""
        V = np.asarray(V, np.float64)
        av = np.abs(V)
        out = V @ self.U
        bracket = 1.01 * (av @ self.a + (3 * self.R + 50) * U32 * (av @ self.M) + 2.0 ** -37 * av.max() * self.M.sum(0)[None, :])
        return out, bracket + U32 * (np.abs(out) + bracket)

    def cast_allow(self, w):
        """(fl(w), A): the float row the device contracts and the allowance of its product against U w"""
        w = np.asarray(w, np.float64)
        wf = w.astype(np.float32)
        return wf, self.products(wf[None, :])[1][0] + np.abs(self.U) @ np.abs(wf.astype(np.float64) - w)

    def diag(self, s):
        G = self.G[s]
        return float(G @ G + self.d / (2.0 * self.h2 if self.kernel == "imq" else self.h2))

    def row(self, s):
        return T.stein_row(self.X, self.G, s, self.h2, self.kernel)


def step_length(f, gs, uss):
    num, den = f - gs, f - 2.0 * gs + uss
    return min(1.0, num / den) if num > 0.0 and den > 0.0 else 0.0


def frank_wolfe(m, iters):
    """the fp64 iteration on the exact matrix -> (w, idx [iters], gamma [iters], f [iters + 1] with f[0] = f(uniform))"""
    n = m.n
    w = np.full(n, 1.0 / n)
    g = m.U @ w
    idx, gam, fs = np.empty(iters, np.int64), np.empty(iters), np.empty(iters + 1)
    fs[0] = w @ g
    for t in range(iters):
        s = int(np.argmin(g))
        gamma = step_length(w @ g, g[s], m.U[s, s])
        w = (1.0 - gamma) * w
        w[s] += gamma
        g = (1.0 - gamma) * g + gamma * m.U[s]
        idx[t], gam[t], fs[t + 1] = s, gamma, w @ g
    return w, idx, gam, fs


def gamma_interval(num, den, e_num, e_den):
    lo_n, hi_n, lo_d, hi_d = num - e_num, num + e_num, den - e_den, den + e_den
    lo = min(1.0, lo_n / hi_d) if lo_n > 0.0 and lo_d > 0.0 else 0.0
    if hi_n <= 0.0 or hi_d <= 0.0:
        hi = 0.0
    else:
        hi = 1.0 if lo_d <= 0.0 else min(1.0, hi_n / lo_d)
    return lo * (1.0 - 2.0 ** -50), min(1.0, hi * (1.0 + 2.0 ** -50))


class Forced:
    """what teacher_forced returns, one entry per step t = 1 .. iters:
    gap       g_{t-1}[s_t] - min g_{t-1}  (>= 0);   allow: 2 max A_{t-1};   argmin: the fp64 argmin (lowest index)
    decisive  the fp64 runner-up lies more than 4 allow above the minimum
    g_lo, g_hi  the interval of the module docstring for gamma_t;   f [iters + 1]: the fp64 w^T g before / after every step
    w, g, A   the replayed state after the last step"""


def teacher_forced(m, idx, gamma):
    idx, gamma = np.asarray(idx, np.int64), np.asarray(gamma, np.float64)
    iters, n = idx.size, m.n
    assert iters == 0 or (idx.min() >= 0 and idx.max() < n), "a vertex outside [0, n)"
    w = np.full(n, 1.0 / n)
    g = m.U @ w
    A = m.cast_allow(w)[1]
    r = Forced()
    r.gap, r.allow, r.argmin, r.decisive = np.empty(iters), np.empty(iters), np.empty(iters, np.int64), np.empty(iters, bool)
    r.g_lo, r.g_hi, r.f = np.empty(iters), np.empty(iters), np.empty(iters + 1)
    r.f[0] = w @ g
    for t in range(iters):
        s, gm = int(idx[t]), float(gamma[t])
        j = int(np.argmin(g))
        lo = g[j]
        r.gap[t], r.argmin[t], r.allow[t] = g[s] - lo, j, 2.0 * A.max()
        r.decisive[t] = bool(np.delete(g, j).min() - lo > 4.0 * r.allow[t])
        f, uss = float(w @ g), m.diag(s)
        A_f = float(w @ A) + (n + 4 * (t + 1) + 8) * 2.0 ** -53 * float(w @ np.abs(g))
        A_u = (m.d + 8) * 2.0 ** -53 * uss
        r.g_lo[t], r.g_hi[t] = gamma_interval(f - g[s], f - 2.0 * g[s] + uss, A_f + A[s], A_f + 2.0 * A[s] + A_u)
        u, M, allow = m.row(s)
        w = (1.0 - gm) * w
        w[s] += gm
        g = (1.0 - gm) * g + gm * u
        A = (1.0 - gm) * A + gm * allow + 2.0 ** -50 * (np.abs(g) + gm * M)
        r.f[t + 1] = w @ g
    r.w, r.g, r.A = w, g, A
    return r


def certificate(m, w):
    """((f, gap), (allow_f, allow_gap)) of the weights w (the device's w_out) in fp64"""
    w = np.asarray(w, np.float64)
    g = m.U @ w
    A_g = m.cast_allow(w)[1]
    a_f = float(w @ A_g) + (m.n + 8) * 2.0 ** -53 * float(w @ np.abs(g))
    f = float(w @ g)
    return (f, f - float(g.min())), (a_f, a_f + float(A_g.max()))
