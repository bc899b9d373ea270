"""fp64 references of the WEIGHTED summaries of the predictive producers (csrc/stein_predict.hip, stein_predict_*_weighted)
with an a-priori fp32 error allowance per element.

TEST INFRASTRUCTURE ONLY.  Written by the rules at the top of tests/score_ref.py and tests/predict_ref.py (u = 2^-24,
gamma(m), expf charged 4 u, gamma64 for the fp64 parts; no safety factors), against the operations NumPy arrays and torch
tensors share.  The forward pass (glm_link, bnn_link, outputs, loglik) is predict_ref's and is imported, not copied.

Weights w [n] >= 0 in fp64, W their sum, v_p = w_p / W.  The lanes hold vh_p = fl32(v_p) = v_p (1 + e_p), |e_p| <= u, or 0
when v_p is below TINY = 2^-126 (the kernel flushes it; "flushed" below).  A particle with w_p = 0 enters nothing: every
max, range and sum below runs over the particles with w_p > 0 only.

    mean_b = sum_p v_p f_pb      var_b = sum_p v_p (f_pb - mean_b)^2      lpd_b = log sum_p v_p exp(l_pb)
    ess    = W^2 / sum_p w_p^2

The kernel cuts the particles into slices of c = `per`; a lane walks its slice in order with West's update and the slices
are merged in fp64 with the weights c_s = W_s / W of the weight pass.  D = max f - min f + 2 max df as in predict_ref.

Effective weights.  In exact arithmetic the kernel's mean is sum_p vt_p f_p with vt_p = c_s vh_p / sum_(q in s) vh_q, a
probability vector.  Against v:  vh_p / v_p = 1 + e_p;  the slice's sum of vh is (c_s - phi_s)(1 + e'), |e'| <= u, phi_s the
flushed mass of the slice;  sum_(p live in s) v_p phi_s / (c_s - phi_s) = phi_s;  a flushed p loses v_p itself.  The fp64
sums W_s and W (n terms) and the quotient move every c_s by gamma64(n + 2) relatively.  With at most n flushed weights,
    eta = sum_p |vt_p - v_p| <= gamma(2) + 3 n TINY + 2 gamma64(n + 2)
and a probability vector moved by eta moves a mean by at most eta D (subtract the midrange first: the weights' changes
sum to zero) and a variance by at most eta D^2 (the variance is the minimum over c of sum v (f - c)^2).

    mean      West on g_k = fl(f_k - f_first) (u D each): m_k = fma(d_k, r_k, m_(k-1)), d_k = fl(g_k - m_(k-1)), r_k =
              fl(vh_k / S_k), S_k = fl(S_(k-1) + vh_k) the running fp32 sum of the weights (gamma(k - 1) relative, every
              term positive).  r_k carries gamma(k - 1) + u =: rho_k, d_k u, the fma u |m_k|.  Against the exact
              vh-weighted running mean, with P_k the exact partial sum of the weights,
                  P_k |e_k| <= P_(k-1) |e_(k-1)| + vh_k (rho_k + u) |g_k - m_(k-1)| + P_k u |m_k|,  both magnitudes <= D + |e|,
              and sum_k P_k <= c P_c (all the weight may come first; 1/n weights gave (c + 1) / 2 here), so
                  |e_c| <= E = a D / (1 - a),   a = gamma(c + 2) + u c        (the u D of g itself is in the c + 2).
              The finish merges as predict_ref describes, with c_s for the counts: e64 = gamma64(5 slices) (|mean| + D).
                  allowance = sum_p v_p df_p + eta D + E + u |mean| + e64.
    var       Input: 2 sum_p v_p |f_p - mean| df_p + sum_p v_p df_p^2.  Weights: the kernel adds sum_p vh_p (f_p - mu_s)^2
              within the slices and sum_s c_s (mu_s - mu)^2 between them; that is the variance under vt plus sum_p (vh_p -
              vt_p)(f_p - mu_s)^2, so 2 eta D^2 for the difference and eta D^2 for vt against v: 3 eta D^2.  West's increment
              vh d_k (g_k - m_k) = vh d_k^2 (1 - r_k): the error rho_k of r_k is rho_k r_k vh d^2 <= gamma(c + 1) (D + E)^2
              summed over the slice's weights; the means off by E and g by u D, the products' three roundings, the c
              additions and Chan's merge are predict_ref's terms with sum vh = 1 in place of 1/n sum 1:
                  allowance = input + 3 eta D^2 + 2 E' D + E'^2 + gamma(c + 3) (var + (D + E)^2) + gamma(c + 1) (D + E)^2
                              + 4 D E + 4 E^2 + u var + v64,     E' = E + u D,  v64 = gamma64(9 slices + 1) var + 4 D e64 + 4 e64^2.
    lpd       max_p dl (1-Lipschitz in the sup norm).  A term is vh_p exp(l_p - max): the weight's rounding is one more
              relative rounding per term beside predict_ref's six per step: rho = gamma(6 c + 1).  The flushed weights'
              terms are lost: charged exactly, lpd - lpd_kept with lpd_kept the value without them.  A product vh e below
              the normal range may be lost: n TINY against the kept sum T = sum_kept v exp(l - top_kept), T >= the weight
              of the likeliest kept particle.  fp64: the merge's seven per slice, the weights' gamma64(n + 2), log (4, of
              |log T|) and the sum with top:
                  allowance = max_p dl + rho / (1 - rho) + (lpd - lpd_kept) + n TINY / T + u |lpd|
                              + gamma64(7 slices + n + 2) + 2^-53 (2 |lpd| + 4 |log T|).
    ess       fp64 throughout: n additions for W, n products and n additions for sum w^2, a product and a quotient:
                  allowance = gamma64(3 n + 4) ess.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as pr  # noqa: E402
from predict_ref import TINY, U64, gamma64, glm_link, bnn_link, outputs, loglik  # noqa: E402,F401
from score_ref import U, gamma  # noqa: E402

FLT_MIN = float(np.finfo(np.float32).tiny)     # = TINY


def _xp(a):
    return pr._xp(a)


def _live_max(a, live, xp):
    fill = xp.zeros_like(a) - float("inf")
    return pr._amax(xp.where(live, a, fill), xp)


def _live_min(a, live, xp):
    return -_live_max(-a, live, xp)


def _clean(a, live, xp):
    """a with the rows of weight zero replaced by 0: they enter no sum, whatever they hold"""
    return xp.where(live, a, xp.zeros_like(a))


def normalised(w):
    """-> (v [n] = w / W, W, live [n, 1]) in fp64"""
    W = w.sum()
    return w / W, W, (w > 0)[:, None]


def eta(n):
    return gamma(2) + 3.0 * n * TINY + 2.0 * gamma64(n + 2)


def mean_var(f, df, w, per, slices):
    """-> (mean [B], allowance, var [B], allowance) of f [n, B] held with error df under the weights w [n]"""
    xp = _xp(f)
    n = f.shape[0]
    v, _, live = normalised(w)
    f, df = _clean(f, live, xp), _clean(df + xp.zeros_like(f), live, xp)
    vc = v[:, None]
    mean = (vc * f).sum(0)
    var = (vc * (f - mean) ** 2).sum(0)
    D = _live_max(f, live, xp) - _live_min(f, live, xp) + 2.0 * _live_max(df, live, xp)
    a = gamma(per + 2) + U * per
    E = a * D / (1.0 - a)
    e64 = gamma64(5 * slices) * (xp.abs(mean) + D)
    et = eta(n)
    allow_mean = (vc * df).sum(0) + et * D + E + U * xp.abs(mean) + e64
    Ep = E + U * D
    inp = 2.0 * (vc * xp.abs(f - mean) * df).sum(0) + (vc * df * df).sum(0)
    allow_var = (inp + 3.0 * et * D * D + 2.0 * Ep * D + Ep * Ep + gamma(per + 3) * (var + (D + E) ** 2)
                 + gamma(per + 1) * (D + E) ** 2 + 4.0 * D * E + 4.0 * E * E + U * var
                 + gamma64(9 * slices + 1) * var + 4.0 * D * e64 + 4.0 * e64 * e64)
    return mean, allow_mean, var, allow_var


def _lse(l, v, keep, xp):
    """-> (log sum_keep v exp(l), T = sum_keep v exp(l - top), top = max_keep l)"""
    top = _live_max(l, keep, xp)
    T = (_clean(v[:, None] * xp.exp(_clean(l - top, keep, xp)), keep, xp)).sum(0)
    return top + xp.log(T), T


def lpd(l, dl, w, per, slices):
    """-> (lpd [B], allowance) of the log likelihoods l [n, B] held with error dl under the weights w [n]"""
    xp = _xp(l)
    n = l.shape[0]
    v, _, live = normalised(w)
    kept = (v >= TINY * (1.0 + 2.0 * U))[:, None]          # certainly not flushed; what the kernel keeps beyond these only helps
    val, _ = _lse(l, v, live, xp)
    val_kept, T = _lse(l, v, kept, xp)
    rho = gamma(6 * per + 1)
    allow = (_live_max(dl + xp.zeros_like(l), live, xp) + rho / (1.0 - rho) + xp.abs(val - val_kept) + n * TINY / T + U * xp.abs(val)
             + gamma64(7 * slices + n + 2) + U64 * (2.0 * xp.abs(val) + 4.0 * xp.abs(xp.log(T))))
    return val, allow


def ess(w):
    """-> (ess, allowance), scalars"""
    n = w.shape[0]
    val = w.sum() ** 2 / (w * w).sum()
    return val, gamma64(3 * n + 4) * val


# ------------------------------------------------------------------------------------------------
# NumPy float32 after the kernel: the weights summed in fp64 and divided by W in fp64, rounded to fp32 and flushed below the
# normal range; every slice walked in the kernel's order with West's update and the running max; the slices merged in fp64
# one after the other with W_s / W, a slice whose weights all round to zero skipped.  One more correct fp32 evaluation in the
# kernel's order (predict_ref.summaries_f32 says what "order" leaves out), used on the CPU before a GPU sees the allowance.
# ------------------------------------------------------------------------------------------------
def lane_weights(w):
    w = np.asarray(w, np.float64)
    with np.errstate(under="ignore"):
        vh = (w / w.sum()).astype(np.float32)
    vh[vh < np.float32(FLT_MIN)] = 0
    return vh


def summaries_f32(fv, l, w, per):
    """the kernel's weighted reduction on float32 values fv [n, B] (and l, or None) -> (mean, var, lpd or None) as float32"""
    f = np.float32
    n, B = fv.shape
    w = np.asarray(w, np.float64)
    W = w.sum()
    vh = lane_weights(w)
    cnt, m, m2, top, tot = 0.0, np.zeros(B), np.zeros(B), None, None
    for s0 in range(0, n, per):
        blk, wb = fv[s0:s0 + per], vh[s0:s0 + per]
        if not (wb > 0).any():
            continue                                       # the weight pass zeroes this slice's W_s: no state is read
        wk, shift, mean, M2, mx, se = f(0), None, np.zeros(B, f), np.zeros(B, f), None, None
        for k in range(blk.shape[0]):
            wp = wb[k]
            if not wp > 0:
                continue
            first = wk == 0
            wk = f(wk + wp)
            if first:
                shift = blk[k].copy()
            g = blk[k] - shift
            delta = g - mean
            mean = mean + delta * f(wp / wk)
            M2 = M2 + f(wp) * delta * (g - mean)
            if l is not None:
                lk = l[s0 + k]
                if first:
                    mx, se = lk.copy(), np.full(B, wp, f)
                else:
                    with np.errstate(invalid="ignore", under="ignore"):
                        e = np.where(lk == mx, f(1), np.exp(-np.abs(lk - mx))).astype(f)
                        up = lk > mx
                        se = np.where(up, se * e + wp, wp * e + se).astype(f)
                    mx = np.where(up, lk, mx)
        assert mean.dtype == f and M2.dtype == f
        cs = float(w[s0:s0 + per].sum() / W)
        ms = shift.astype(np.float64) + mean.astype(np.float64)
        t, delta = cnt + cs, ms - m
        m = m + delta * (cs / t)
        m2 = m2 + M2.astype(np.float64) + delta * delta * (cnt * cs / t)
        cnt = t
        if l is not None:
            mx64, se64 = mx.astype(np.float64), se.astype(np.float64)
            if top is None:
                top, tot = mx64, se64
            else:
                new = np.maximum(top, mx64)
                tot = tot * np.exp(top - new) + se64 * np.exp(mx64 - new)
                top = new
    out_lpd = (top + np.log(tot)).astype(f) if l is not None else None
    return m.astype(f), m2.astype(f), out_lpd
