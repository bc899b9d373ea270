"""fp64 references of the predictive producers (csrc/stein_predict.hip) with an a-priori fp32 error allowance per element.

TEST INFRASTRUCTURE ONLY.  Written by the rules at the top of tests/score_ref.py (u = 2^-24, gamma(m), expf charged 4 u,
the same charge for logf / log1pf; no safety factors) and, like it, against the operations NumPy arrays and torch tensors
share, so the same code runs on the CPU and in torch fp64 on the device.  Inputs are fp64 arrays holding fp32 values.

Outputs (z the linear output, f the reported one, [n, B]):
    dz        GLM: the dz of score_ref.glm_score, gamma(F + 6) sum_c |w_c x_bc|;  network: the dpred of score_ref.bnn_score
              (the kernel's summation order differs from the score kernels'; no term of it passes more roundings)
    df        = dz, or for sigmoid(z) = 1 / (1 + expf(-z)):  dz / 4 (sigmoid is 1/4-Lipschitz) + gamma(6) sigmoid (expf 4 u
              damped by 1 - sigmoid, the add, the division) + TINY
    TINY      = 2^-126: a result below the normal range may be flushed to zero

Log likelihoods l, [n, B]  (r = y - z, dr = dz + u (|r| + dz), R = |r| + dr):
    linear    l = c0 - h r^2, h = fl(tau / 2), c0 = fl(log(tau) / 2 - log(2 pi) / 2) rounded once on the host:
              dl = h (R^2 - r^2) + gamma(4) h R^2 + 2 u |c0| + u |l|        (h, r^2, the fma; c0's rounding and the result's)
    network   the same with h = expf(lg) / 2 (4 u more: gamma(8)) and c0 = fma(1/2, lg, -fl(log(2 pi) / 2)):
              dl = h (R^2 - r^2) + gamma(8) h R^2 + u (2 |c0| + log(2 pi) / 2 + |l|)
    logistic  l = y z - (max(z, 0) + log1pf(expf(-|z|))): y z moves by |y| dz and softplus, 1-Lipschitz, by dz;
              expf (4 u on e <= 1, passed through log1p with slope <= 1, and e / (1 + e) <= log1p(e)) and log1pf (4 u) are
              8 u log1p(e); the product, the sum and the difference are u (|y z| + softplus + |l|); TINY

Summaries of one row b over the particles.  The kernel cuts the particles into slices of `per` (tests/predict_cases.py
mirrors its plan); a lane walks its slice in order and the slices are merged in fp64, charged gamma64 = 2^-53 terms.
With D = max_p f - min_p f + 2 max_p df (the range of the values the kernel holds) and c = per:
    mean      Each slice runs Welford's update on g_k = fl(f_k - f_first) (|g| <= D, one rounding u D each):
              m_k = m_(k-1) + (g_k - m_(k-1)) / k with four roundings (the difference, 1 / k, the product, the sum; an fma
              saves one).  Against the exact running mean mu_k,
                  k |e_k| <= (k - 1) |e_(k-1)| + gamma(3) |g_k - m_(k-1)| + k u |m_k|,   both magnitudes <= D + |e|,
              so |e_c| <= E = a D / (1 - a),  a = gamma(4) + u (c + 1) / 2   (the u D of g itself is the fourth).
              The finish adds f_first + m in fp64 and merges the slice means pairwise, m += (m_s - m) c_s / (c + c_s): a
              convex combination, so the inputs' errors are not amplified, plus five fp64 roundings (f_first + m, the
              difference, the quotient, the product, the sum) of magnitudes <= |mean| + D.  The longest chain of merges
              in the finish kernel's tree (16 groups of consecutive slices, then the groups) is at most `slices` long:
                  e64 = gamma64(5 slices) (|mean| + D).
              allowance = mean_p df + E + u |mean| (the result's rounding) + e64.
    var       Exact statistics of perturbed values: (2 / n) sum_p |f - mean| df + mean_p df^2.  Welford's increment
              (g_k - m_(k-1)) (g_k - m_k) with both means off by <= E and g by <= u D errs by <= 2 (E + u D) D + (E + u D)^2
              + gamma(3) (D + E)^2 per particle; c of them are added with one rounding each (gamma(c) of the total, M2 <=
              n var); Chan's merge adds c_s (m_s - m)^2 with every m_s off by <= E: 4 D E + 4 E^2.  So
                  allowance = input + 2 E' D + E'^2 + gamma(c + 3) (var + (D + E)^2) + 4 D E + 4 E^2 + u var + v64,
              E' = E + u D.  The fp64 merge: every term of M2 is non-negative, so roundings are relative to partial sums
              <= n var: per merge the increment (m_s - m)^2 c c_s / (c + c_s) passes seven (the difference counted twice,
              the square, c c_s, the quotient, the product, the sum with M2_s) and the running sum two, the division by n
              one; the merged means are off by e64 each, as above for E:
                  v64 = gamma64(9 slices + 1) var + 4 D e64 + 4 e64^2.
    lpd       log-sum-exp is 1-Lipschitz in the sup norm: max_p dl.  A slice keeps (max, s = sum exp(l - max)); one step
              costs the subtraction (u |l - max| in the exponent: the shifts a term sees add up to its final distance x from
              the max, and x e^-x <= 1 / e while s >= 1), expf (4 u) and one fma or add: relative error of s at most
              rho = gamma(6 c); a term below the normal range is lost (c TINY).  The merge is in fp64.
                  allowance = max_p dl + rho / (1 - rho) + c TINY + u |lpd| + l64
              The fp64 merge: the max is exact; a slice's term s exp(max_s - top) passes the subtraction (as above, at
              most one relative rounding of the sum), exp (charged 4), the product and the add, seven in a chain of at
              most `slices`; then log (4, of |log sum| <= log n), log n (4), the sum with top and the difference (one
              each, of magnitudes <= |lpd| + 2 log n):
                  l64 = gamma64(7 slices) + 2^-53 (2 |lpd| + 12 log n).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402
from score_ref import EXP_U, LANES, U, gamma  # noqa: E402

TINY = 2.0 ** -126
U64 = 2.0 ** -53


def gamma64(m):
    return m * U64 / (1.0 - m * U64)
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def _xp(a):
    return sr._xp(a)


def _amax(a, xp):
    return a.max(0) if xp is np else a.max(0).values


def _amin(a, xp):
    return a.min(0) if xp is np else a.min(0).values


def glm_link(theta, w_col, F, X):
    """-> (z [n, B], dz)"""
    xp = _xp(theta)
    w = theta[:, w_col:w_col + F]
    return w @ X.T, gamma(F + LANES) * (xp.abs(w) @ xp.abs(X).T)


def bnn_link(theta, n_in, H, cols, X):
    """-> (z [n, B], dz, log_gamma [n]); cols as score_ref.bnn_score"""
    xp = _xp(theta)
    n, F = theta.shape[0], n_in
    c = dict(zip(sr.BNN_ORDER, cols))
    w1 = theta[:, c["w1"]:c["w1"] + F * H].reshape(n, F, H)
    b1, w2, b2 = theta[:, c["b1"]:c["b1"] + H], theta[:, c["w2"]:c["w2"] + H], theta[:, c["b2"]]
    aw2 = xp.abs(w2)[:, None, :]
    zh = X @ w1 + b1[:, None, :]                           # [n, B, H]
    dzh = gamma(F + 1) * (xp.abs(X) @ xp.abs(w1) + xp.abs(b1)[:, None, :])
    a = xp.maximum(zh, xp.zeros_like(zh))
    pred = (a * w2[:, None, :]).sum(-1) + b2[:, None]
    dpred = (dzh * aw2).sum(-1) + gamma(H + LANES + 1) * ((a * aw2).sum(-1) + xp.abs(b2)[:, None])
    return pred, dpred, theta[:, c["log_gamma"]]


def outputs(z, dz, sigmoid):
    """-> (f, df): f = z, or sigmoid(z) for the logistic model with STEIN_PRED_MEAN"""
    if not sigmoid:
        return z, dz
    xp = _xp(z)
    f = 1.0 / (1.0 + xp.exp(-z))
    return f, 0.25 * dz + gamma(2 + EXP_U) * f + TINY


def _gauss(z, dz, y, h, c0, k, extra):
    xp = _xp(z)
    r = y - z
    dr = dz + U * (xp.abs(r) + dz)
    R = xp.abs(r) + dr
    l = c0 - h * r * r
    return l, h * (R * R - r * r) + gamma(k) * h * R * R + 2.0 * U * abs(c0) + U * xp.abs(l) + extra


def loglik(model, z, dz, y, noise_precision=1.0, log_gamma=None):
    """-> (l [n, B], dl); model "linear" | "logistic" | "bnn" (log_gamma [n])"""
    xp = _xp(z)
    if model == "linear":
        tau = float(noise_precision)
        return _gauss(z, dz, y, 0.5 * tau, 0.5 * np.log(tau) - HALF_LOG_2PI, 4, 0.0)
    if model == "bnn":
        lg = log_gamma[:, None]
        return _gauss(z, dz, y, 0.5 * xp.exp(lg), 0.5 * lg - HALF_LOG_2PI, 4 + EXP_U, U * HALF_LOG_2PI)
    az = xp.abs(z)
    tail = xp.log1p(xp.exp(-az))
    sp = xp.maximum(z, xp.zeros_like(z)) + tail
    l = y * z - sp
    return l, (xp.abs(y) + 1.0) * dz + 2 * EXP_U * U * tail + U * (xp.abs(y * z) + sp + xp.abs(l)) + TINY


def mean_var(f, df, per, slices):
    """-> (mean [B], allowance, var [B], allowance) of f [n, B] held with error df, reduced in slices of `per` particles"""
    xp = _xp(f)
    n = f.shape[0]
    mean = f.mean(0)
    var = ((f - mean) ** 2).mean(0)
    D = _amax(f, xp) - _amin(f, xp) + 2.0 * _amax(df, xp)
    a = gamma(4) + U * (per + 1) / 2.0
    E = a * D / (1.0 - a)
    e64 = gamma64(5 * slices) * (xp.abs(mean) + D)
    allow_mean = df.mean(0) + E + U * xp.abs(mean) + e64
    Ep = E + U * D
    inp = (2.0 / n) * (xp.abs(f - mean) * df).sum(0) + (df * df).mean(0)
    allow_var = (inp + 2.0 * Ep * D + Ep * Ep + gamma(per + 3) * (var + (D + E) ** 2) + 4.0 * D * E + 4.0 * E * E
                 + U * var + gamma64(9 * slices + 1) * var + 4.0 * D * e64 + 4.0 * e64 * e64)
    return mean, allow_mean, var, allow_var


def lpd(l, dl, per, slices):
    """-> (lpd [B], allowance) of the log likelihoods l [n, B] held with error dl"""
    xp = _xp(l)
    n = l.shape[0]
    top = _amax(l, xp)
    val = top + xp.log(xp.exp(l - top).sum(0)) - np.log(n)
    rho = gamma(6 * per)
    return val, (_amax(dl, xp) + rho / (1.0 - rho) + per * TINY + U * xp.abs(val) + gamma64(7 * slices)
                 + U64 * (2.0 * xp.abs(val) + 12.0 * np.log(n)))


# ------------------------------------------------------------------------------------------------
# NumPy float32 after the kernel: the same operations on the same fp32 values, with every slice walked in the kernel's
# order and the slices merged in fp64 one after the other (the finish kernel associates the same merges as a tree).  The dot products are summed sequentially, which is the GLM kernel's order but not the network kernel's
# (four partial sums per chunk of 64 hidden units, chunk totals added), and every multiply-add rounds twice where the
# kernel's fma rounds once: dz / dpred charge one rounding per term whatever the order, so this is one more correct fp32
# evaluation, not a bit-for-bit one.  Used on the CPU to check that the allowance holds before a GPU sees it.
# ------------------------------------------------------------------------------------------------
def link_f32(model, theta, X, **m):
    f = np.float32
    th, X = np.asarray(theta, f), np.asarray(X, f)
    if model != "bnn":
        w = th[:, m["w_col"]:m["w_col"] + m["F"]]
        return sr._seq(w[:, None, :] * X[None, :, :], -1)
    n, F, H = th.shape[0], m["n_in"], m["H"]
    c = dict(zip(sr.BNN_ORDER, m["cols"]))
    w1 = th[:, c["w1"]:c["w1"] + F * H].reshape(n, F, H)
    zh = np.broadcast_to(th[:, None, c["b1"]:c["b1"] + H], (n, X.shape[0], H)).copy()
    for k in range(F):
        zh += X[None, :, k, None] * w1[:, None, k, :]
    return sr._seq(np.maximum(zh, f(0)) * th[:, None, c["w2"]:c["w2"] + H], -1) + th[:, c["b2"], None]


def outputs_f32(z, sigmoid):
    f = np.float32
    with np.errstate(over="ignore"):
        return f(1) / (f(1) + np.exp(-z)) if sigmoid else z


def loglik_f32(model, z, y, noise_precision=1.0, log_gamma=None):
    f = np.float32
    y = np.asarray(y, f)
    if model == "logistic":
        return y * z - (np.maximum(z, f(0)) + np.log1p(np.exp(-np.abs(z))))
    if model == "linear":
        h, c0 = f(0.5 * noise_precision), f(0.5 * np.log(noise_precision) - HALF_LOG_2PI)
    else:
        lg = np.asarray(log_gamma, f)[:, None]
        h, c0 = f(0.5) * np.exp(lg), f(0.5) * lg - f(HALF_LOG_2PI)
    r = y - z
    return c0 - h * (r * r)


def summaries_f32(fv, l, per):
    """the kernel's reduction on float32 values fv [n, B] (and l, or None) -> (mean, var, lpd or None) as float32"""
    f = np.float32
    n, B = fv.shape
    cnt, m, m2 = 0.0, np.zeros(B), np.zeros(B)
    states = []
    for s0 in range(0, n, per):
        blk = fv[s0:s0 + per]
        shift, mean, M2 = blk[0].copy(), np.zeros(B, f), np.zeros(B, f)
        mx, se = (l[s0].copy(), np.ones(B, f)) if l is not None else (None, None)
        for k in range(blk.shape[0]):
            g = blk[k] - shift
            delta = g - mean
            mean = mean + delta * (f(1) / f(k + 1))
            M2 = M2 + delta * (g - mean)
            if l is not None and k:
                lk = l[s0 + k]
                with np.errstate(invalid="ignore"):
                    e = np.where(lk == mx, f(1), np.exp(-np.abs(lk - mx))).astype(f)
                up = lk > mx
                se = np.where(up, se * e + f(1), se + e).astype(f)
                mx = np.where(up, lk, mx)
        assert mean.dtype == f and M2.dtype == f
        cs = float(blk.shape[0])
        ms = shift.astype(np.float64) + mean.astype(np.float64)
        tot, delta = cnt + cs, ms - m
        m = m + delta * (cs / tot)
        m2 = m2 + M2.astype(np.float64) + delta * delta * (cnt * cs / tot)
        cnt = tot
        states.append((mx, se))
    out_lpd = None
    if l is not None:
        top = np.max([s[0].astype(np.float64) for s in states], axis=0)
        tot = sum(s[1].astype(np.float64) * np.exp(s[0].astype(np.float64) - top) for s in states)
        out_lpd = (top + np.log(tot) - np.log(n)).astype(f)
    return m.astype(f), (m2 / n).astype(f), out_lpd
