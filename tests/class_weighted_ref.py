"""fp64 references of the WEIGHTED class summaries (csrc/stein_predict_softmax.hip, csrc/stein_predict_bnn_class.hip:
stein_predict_softmax_weighted, stein_predict_bnn_class_weighted) with an a-priori fp32 error allowance per element.

TEST INFRASTRUCTURE ONLY.  The derivations of tests/softmax_ref.py (summaries, _slice_mean, _lpd) extended to weights, by the
same rules (u = 2^-24, gamma(m) = m u / (1 - m u), expf and logf charged 4 u, division correctly rounded, gamma64 for the
fp64 parts; no safety factor), against the operations NumPy arrays and torch tensors share.  The softmax and the entropy of a
particle (softmax_parts, dp, dH) are softmax_ref's, imported and not copied; the network classifier's logits and their
errors come from netclass_ref.forward.

Weights w [n] >= 0 in fp64, W their sum, v_p = w_p / W.  A particle with w_p = 0 enters nothing, whatever its probabilities
are: every sum and maximum below runs over the particles with w_p > 0 only.

    prob_bc = sum_p v_p p_pbc      lpd_b = log sum_p v_p p_{pb,y_b}      ent_b = sum_p v_p H(p_pb.)      ess = W^2 / sum_p w_p^2

A weighted slice sum.  The kernel cuts the particles into slices of `per`; a lane walks its slice in order, acc = fmaf(vh_p,
q~_p, acc), with q~_p = q_p +- dq_p >= 0 the fp32 term (a probability, the probability of the label, an entropy) and vh_p the
lane weight; the slices' sums are added in slice order in fp64 and rounded to fp32.  Nothing is divided by n.  Per term:
    the weight   vh_p = fl32(v~_p) = v~_p (1 + e), |e| <= u, with v~_p the fp64 quotient of w_p and the fp64 sum W~: n
                 additions and one division move it by gamma64(n + 2) relatively (every term is non-negative), charged twice
                 for the first-order cross term with e:               (u + 2 gamma64(n + 2)) v_p (q_p + dq_p)
    the flush    a weight below 2^-126 W counts as zero: its term is lost, at most 2^-126 max_p (q_p + dq_p) each, and a
                 product or a partial sum below the normal range may lose 2^-126 absolutely:
                                                                      n 2^-126 (max_p (q_p + dq_p) + 1)  over all n terms
    the chain    `per` fmaf roundings, every term non-negative:       gamma(per) (1 + u) sum_p v_p (q_p + dq_p)
    the term     its own error, weighted:                             sum_p v_p dq_p
    the merge    at most 1024 fp64 additions, far below 8 roundings of 2^-53:   2^-50 Q
    the result   rounded to fp32:                                     u (Q + all of the above)
so  Q = sum_p v_p q_p  +-  err + u (Q + err),
    err = sum_p v_p dq_p + (u + 2 gamma64(n + 2) + gamma(per) (1 + u)) sum_p v_p (q_p + dq_p) + n 2^-126 (max (q + dq) + 1) + 2^-50 Q.
prob   q = p_c, dq = dp_c.
ent    q = H, dq = dH of softmax_ref (both terms of H are >= 0).
lpd    S = sum_p v_p p_y with err as above and without the final rounding (the logarithm is taken in fp64 of the fp64 sum):
       |log(S~) - log(S)| <= -log(1 - err / S), then the rounding to fp32, u (|lpd| + that).  A label outside [0, C): NaN.
ess    predict_weighted_ref.ess: fp64 throughout, gamma64(3 n + 4) ess.
tight=True drops dz (the forward sum), as in softmax_ref: the allowance against fp64 statistics of the logits the call itself
returned; summaries_of_probs() is prob and lpd against the returned probabilities, which the kernel sums bit for bit: dq = 0.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_ref as ncr  # noqa: E402
import softmax_ref as smr  # noqa: E402
from predict_ref import TINY, gamma64  # noqa: E402
from predict_weighted_ref import ess, lane_weights  # noqa: E402,F401
from score_ref import EXP_U, U, _xp, gamma  # noqa: E402
from softmax_ref import F64, LOG_U, _onehot, softmax_parts  # noqa: E402


def _max0(xp, a):
    return a.max(0) if xp is np else a.max(0).values


def _clean(xp, a, live):
    """a [n, ...] with the particles of weight zero replaced by 0: they enter no sum, whatever they hold"""
    lv = live.reshape((live.shape[0],) + (1,) * (len(a.shape) - 1))
    return xp.where(lv, a, xp.zeros_like(a))


def _wslice_sum(xp, q, dq, w, per, final=True):
    """sum_p v_p q_p over the particles (axis 0) of the non-negative terms q with errors dq, as the kernels take it"""
    n = q.shape[0]
    live = w > 0
    v = (w / w.sum()).reshape((n,) + (1,) * (len(q.shape) - 1))
    q, dq = _clean(xp, q, live), _clean(xp, dq, live)
    Q = (v * q).sum(0)
    T = (v * (q + dq)).sum(0)
    err = ((v * dq).sum(0) + (U + 2.0 * gamma64(n + 2) + gamma(per) * (1.0 + U)) * T
           + n * TINY * (_max0(xp, q + dq) + 1.0) + F64 * Q)
    return Q, (err + U * (Q + err)) if final else err


def _wlpd(xp, py, dpy, w, per):
    S, dS = _wslice_sum(xp, py, dpy, w, per, final=False)
    val = xp.log(S)
    rel = dS / S
    d = -xp.log1p(-rel) if xp is not np else -np.log1p(-np.minimum(rel, 0.5))
    return val, d + U * (xp.abs(val) + d)


def summaries(z, dz, labels, w, per, tight=False):
    """the weighted summaries from the logits z [n, B, C] with error bounds dz under the weights w [n] -> dict name ->
    (value, allowance): prob [B, C]; ent [B]; lpd [B] when labels is given; ess (scalars).  per: particles per slice"""
    xp = _xp(z)
    C = z.shape[-1]
    if tight:
        dz = xp.zeros_like(z)
    live = w > 0
    z, dz = _clean(xp, z, live), _clean(xp, dz, live)      # (a dead particle's logits may be anything; its terms are dropped)
    sp = softmax_parts(z, dz)
    p, dp, t = sp["p"], sp["dp"], sp["t"]
    out = {"prob": _wslice_sum(xp, p, dp, w, per)}
    pt = -(p * t).sum(-1)
    H = sp["logs"] + pt
    logp = t - sp["logs"][..., None]
    dH = (sp["delta"] * sp["grow"] * (p * xp.abs(logp + H[..., None])).sum(-1)
          + gamma(C) + EXP_U * U + LOG_U * U * sp["logs"]
          + (gamma(C + 2 * EXP_U + 1) + gamma(C)) * pt + U * H)
    out["ent"] = _wslice_sum(xp, H, dH, w, per)
    if labels is not None:
        oh = _onehot(xp, labels, C, z)
        out["lpd"] = _wlpd(xp, (p * oh).sum(-1), (dp * oh).sum(-1), w, per)
    out["ess"] = ess(w)
    return out


def summaries_of_probs(p, labels, w, per):
    """prob and lpd against the probabilities the call itself returned (fp64 copies of its fp32 pred)"""
    xp = _xp(p)
    C = p.shape[-1]
    p = _clean(xp, p, w > 0)
    zero = xp.zeros_like(p)
    out = {"prob": _wslice_sum(xp, p, zero, w, per)}
    if labels is not None:
        oh = _onehot(xp, labels, C, p)
        out["lpd"] = _wlpd(xp, (p * oh).sum(-1), (zero * oh).sum(-1), w, per)
    return out


def softmax_logits(theta, w_col, F, C, X):
    """-> (z, dz) of stein_predict_softmax's forward pass (softmax_ref.predict's)"""
    xp = _xp(theta)
    n = theta.shape[0]
    W = theta[:, w_col:w_col + F * C].reshape(n, F, C)
    return X @ W, gamma(F) * (xp.abs(X) @ xp.abs(W))


def netclass_logits(theta, F, H, C, cols, X):
    """-> (z, dz) of stein_predict_bnn_class's forward pass, through netclass_ref.forward"""
    fw = ncr.forward(theta, F, H, C, cols, X)
    return fw["z"], fw["dz"]


# ------------------------------------------------------------------------------------------------
# NumPy float32 after the kernels: the lane weights of predict_weighted_ref.lane_weights (the fp64 quotient rounded to fp32 and
# flushed below the normal range); every slice walked in order with acc = fmaf(vh, q, acc) -- the product of two floats is
# exact in fp64, so fl32 of the fp64 sum is the fused result but for a double rounding at a tie -- skipping the particles of
# weight zero; the slices added in fp64 in slice order.  One more correct fp32 evaluation in the kernels' order, used on the
# CPU before a GPU sees the allowance.
# ------------------------------------------------------------------------------------------------
def weighted_sums_f32(q, w, per):
    """q [n, ...] float32 -> sum_p vh_p q_p as float64 (the fp64 merge of the fp32 slice sums)"""
    f = np.float32
    n = q.shape[0]
    vh = lane_weights(w)
    tot = np.zeros(q.shape[1:], np.float64)
    for a in range(0, n, per):
        acc = np.zeros(q.shape[1:], f)
        for p in range(a, min(n, a + per)):
            if vh[p] > 0:
                with np.errstate(under="ignore"):
                    acc = (np.float64(vh[p]) * q[p].astype(np.float64) + acc.astype(np.float64)).astype(f)
        tot += acc.astype(np.float64)
    return tot


def summaries_f32(z, labels, w, per):
    """the kernels' softmax tail and weighted reduction on float32 logits z [n, B, C] -> dict(prob, ent, lpd, pred_mean)"""
    f = np.float32
    C = z.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        t, s, p = smr._softmax_f32(z)
        H = (np.log(s).astype(f) - smr._seq(p * t, -1)).astype(f)
    out = {"pred_mean": p, "prob": weighted_sums_f32(p, w, per).astype(f), "ent": weighted_sums_f32(H, w, per).astype(f)}
    if labels is not None:
        oh = _onehot(np, labels, C, p)
        with np.errstate(invalid="ignore"):
            py = (np.where(oh == 1, p, 0) + np.where(np.isnan(oh), np.nan, 0)).sum(-1).astype(f)
            out["lpd"] = np.log(weighted_sums_f32(py, w, per)).astype(f)
    return out


def softmax_f32(theta, w_col, F, C, X, labels, w, per):
    f = np.float32
    th, X = np.asarray(theta, f), np.asarray(X, f)
    W = th[:, w_col:w_col + F * C].reshape(th.shape[0], F, C)
    return summaries_f32(smr._logits_f32(X, W), labels, w, per)


def netclass_f32(theta, F, H, C, cols, X, labels, w, per):
    f = np.float32
    _, _, z = ncr._forward_f32(np.asarray(theta, f), F, H, C, cols, np.asarray(X, f))
    return summaries_f32(z, labels, w, per)
