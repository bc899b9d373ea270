"""fp64 references of the two network-classifier calls (csrc/stein_score_bnn_class.hip, csrc/stein_predict_bnn_class.hip) with
an a-priori fp32 error allowance per element.

TEST INFRASTRUCTURE ONLY.  Written against the operations NumPy arrays and torch tensors share, as tests/score_ref.py and
tests/softmax_ref.py are, so the same code is the CPU reference (NumPy) and the device reference (torch fp64 on the GPU).  The
inputs are fp64 arrays holding fp32-representable values; the scalar parameters are rounded to fp32 first.  `labels` is an
integer array.  cols = first column of (w1, b1, w2, b2, log_lambda), cols[4] < 0 or None: the fixed precision.

The allowance is a derivation by the rules at the head of tests/score_ref.py and tests/softmax_ref.py and carries no safety
factor: u = 2^-24, gamma(m) = m u / (1 - m u); a sum of m rounded terms in any order errs by gamma(m) sum |terms| (an FMA
feeding the sum is one of the m roundings); expf and logf are charged 2 ulp = 4 u relative (EXP_U, LOG_U); division is
correctly rounded.  Errors already present in an operand are propagated to first order explicitly and the cross terms
through |x| + dx in place of |x|.  F = n_in, H, C, B = batch.

Forward, as both kernels take it (a lane sums a pre-activation and a logit alone, in ascending order: no shuffle adds):
    dpre_bh = gamma(F + 1) (|b1_h| + sum_f |x_bf w1_fh|)            b1 and F FMAs (the rule of score_ref.py's network)
    a_bh    = relu(pre_bh), 1-Lipschitz: da_bh = dpre_bh;  A_bh = a_bh + dpre_bh
    dz_bc   = sum_h dpre_bh |w2_hc| + gamma(H + 1) (|b2_c| + sum_h A_bh |w2_hc|)      b2 and H FMAs
    p, dp, delta, ...: softmax_ref.softmax_parts(z, dz), unchanged: the kernels evaluate the softmax as the softmax model's do
Score (r_bc = 1[y_b = c] - p_bc, m_bh = [pre_bh > 0], D_bh = sum_c r_bc w2_hc, delta_bh = m_bh D_bh):
    dr_bc   = dp_bc + u (|r_bc| + dp_bc);  R_bc = |r_bc| + dr_bc     one subtraction
    gb2_c   = sum_b r_bc        +- sum_b dr_bc + gamma(B) sum_b R_bc
    gw2_hc  = sum_b a_bh r_bc   +- sum_b (A_bh R_bc - a_bh |r_bc|) + gamma(B) sum_b A_bh R_bc
    dD_bh   = sum_c dr_bc |w2_hc| + gamma(C) sum_c R_bc |w2_hc|      C FMAs from zero
    gb1_h   = sum_b delta_bh    +- sum_b m_bh dD_bh + gamma(B) sum_b m_bh (|D_bh| + dD_bh) + sum over the AMBIGUOUS b of
                                   (|D_bh| + dD_bh)
    gw1_fh  = sum_b x_bf delta_bh: the same with every term times |x_bf|
    every block  scale G - prec W:  scale E_G (1 + gamma(k)) + gamma(k) (scale |G| + |prec W|), k = 3 (two products and the
              subtraction; adding the +0 of a good label is exact), + EXP_U when the precision is expf(log lambda)
    log_lambda entry  P / 2 - prec (sw2 / 2 + rate):  A = gamma(P + 6 + 3 + EXP_U + 4) prec (sw2 / 2 + rate), allowance
              A + u (|value| + A), as the alpha entry of softmax_ref.py with P in the place of F C
    A label outside [0, C): every entry of the four blocks of the reference is NaN (compare with isnan).
ReLU masks, as score_ref.py treats them: a (b, h) with |pre_bh| <= dpre_bh is ambiguous -- a correct fp32 evaluation may take
either branch, which moves b1_h by the whole term |D_bh| and w1_fh by |D_bh x_bf|.  Those terms are added to the allowance of
exactly the b1_h and w1_.h entries they touch; score() also returns the share of live entries so touched, which the tests cap
at 2 %.  (a_bh itself is continuous in pre_bh, so gw2, gb2 and the predictive call carry no such term.)
Predictive: softmax_ref.summaries(z, dz, labels, per) with the dz above -- pred, prob, lpd and ent by the rules written there;
tight=True and softmax_ref.summaries_of_probs are the allowances against fp64 statistics of the call's own pred.
"""
import numpy as np

from score_ref import EXP_U, LANES, U, _f32, _xp, gamma
from softmax_ref import WAVES, _onehot, _seq, _softmax_f32, softmax_parts, summaries, summaries_of_probs  # noqa: F401

ORDER = ("w1", "b1", "w2", "b2", "log_lambda")


def _blocks(theta, F, H, C, cols):
    n = theta.shape[0]
    w1 = theta[:, cols[0]:cols[0] + F * H].reshape(n, F, H)
    b1 = theta[:, cols[1]:cols[1] + H]
    w2 = theta[:, cols[2]:cols[2] + H * C].reshape(n, H, C)
    b2 = theta[:, cols[3]:cols[3] + C]
    return w1, b1, w2, b2


def _as(xp, like, cond):
    return cond.to(like.dtype) if xp is not np else cond.astype(like.dtype)


def forward(theta, F, H, C, cols, X):
    """-> dict of pre, dpre, a, z, dz (fp64) by the rules of the module docstring"""
    xp = _xp(theta)
    w1, b1, w2, b2 = _blocks(theta, F, H, C, cols)
    aX = xp.abs(X)
    pre = X @ w1 + b1[:, None, :]                          # [n, B, H]
    dpre = gamma(F + 1) * (aX @ xp.abs(w1) + xp.abs(b1)[:, None, :])
    a = xp.maximum(pre, xp.zeros_like(pre))
    z = a @ w2 + b2[:, None, :]                            # [n, B, C]
    aw2 = xp.abs(w2)
    dz = dpre @ aw2 + gamma(H + 1) * ((a + dpre) @ aw2 + xp.abs(b2)[:, None, :])
    return {"pre": pre, "dpre": dpre, "a": a, "z": z, "dz": dz}


def live_count(F, H, C, cols):
    return F * H + H + H * C + C + (1 if cols[4] is not None and cols[4] >= 0 else 0)


def score(theta, F, H, C, cols, X, labels, scale=1.0, prior_precision=1.0, gamma_rate=0.01):
    """-> (score [n, d], allowance [n, d], share) of stein_score_bnn_class.  share: the fraction of the live (model) entries
    whose allowance holds the whole term of an ambiguous ReLU mask."""
    xp = _xp(theta)
    n = theta.shape[0]
    B = X.shape[0]
    s, rate = _f32(scale), _f32(gamma_rate)
    ll = -1 if cols[4] is None else cols[4]
    w1, b1, w2, b2 = _blocks(theta, F, H, C, cols)
    fw = forward(theta, F, H, C, cols, X)
    pre, dpre, a = fw["pre"], fw["dpre"], fw["a"]
    sp = softmax_parts(fw["z"], fw["dz"])
    r = _onehot(xp, labels, C, fw["z"]) - sp["p"]          # [n, B, C]
    dr = sp["dp"] + U * (xp.abs(r) + sp["dp"])
    R = xp.abs(r) + dr
    aX, aw2 = xp.abs(X), xp.abs(w2)
    A = a + dpre
    m = _as(xp, pre, pre > 0)
    amb = _as(xp, pre, xp.abs(pre) <= dpre)
    gB = gamma(B)
    gb2, E_gb2 = r.sum(1), dr.sum(1) + gB * R.sum(1)       # [n, C]
    aT, AT = xp.swapaxes(a, 1, 2), xp.swapaxes(A, 1, 2)
    gw2 = aT @ r                                           # [n, H, C]
    AR = AT @ R
    E_gw2 = AR - aT @ xp.abs(r) + gB * AR
    w2T = xp.swapaxes(w2, 1, 2)
    aw2T = xp.abs(w2T)
    D = r @ w2T                                            # [n, B, H]
    dD = dr @ aw2T + gamma(C) * (R @ aw2T)
    dl = m * D
    Dt = xp.abs(D) + dD
    E = m * dD + gB * m * Dt + amb * Dt
    gb1, E_gb1 = dl.sum(1), E.sum(1)                       # [n, H]
    gw1, E_gw1 = X.T @ dl, aX.T @ E                        # [n, F, H]
    k = 3 + (EXP_U if ll >= 0 else 0)
    prec = xp.exp(theta[:, ll]) if ll >= 0 else _f32(prior_precision) * xp.ones_like(theta[:, 0])
    gk = gamma(k)
    out, allow = xp.zeros_like(theta), xp.zeros_like(theta)

    def put(col, G, EG, W):
        pw = prec.reshape((n,) + (1,) * (len(W.shape) - 1)) * W
        size = int(np.prod(G.shape[1:]))
        out[:, col:col + size] = (s * G - pw).reshape(n, size)
        allow[:, col:col + size] = (s * EG * (1.0 + gk) + gk * (s * xp.abs(G) + xp.abs(pw))).reshape(n, size)
    put(cols[0], gw1, E_gw1, w1)
    put(cols[1], gb1, E_gb1, b1)
    put(cols[2], gw2, E_gw2, w2)
    put(cols[3], gb2, E_gb2, b2)
    P = F * H + H + H * C + C
    if ll >= 0:
        sw2 = (w1 * w1).sum(-1).sum(-1) + (b1 * b1).sum(-1) + (w2 * w2).sum(-1).sum(-1) + (b2 * b2).sum(-1)
        tt = prec * (0.5 * sw2 + rate)
        val = 0.5 * P - tt
        Aa = gamma(P + LANES + WAVES + EXP_U + 4) * tt
        out[:, ll] = val
        allow[:, ll] = Aa + U * (xp.abs(val) + Aa)
    touched = float((amb.sum(1) > 0).sum()) * (1 + F)
    return out, allow, touched / float(n * live_count(F, H, C, cols))


def predict(theta, F, H, C, cols, X, labels, per):
    """-> the dict of softmax_ref.summaries() for stein_predict_bnn_class's arguments"""
    fw = forward(theta, F, H, C, cols, X)
    return summaries(fw["z"], fw["dz"], labels, per)


# ------------------------------------------------------------------------------------------------
# the same formulas in NumPy float32 in the kernels' summation order (features, hidden units, classes, rows ascending;
# particles ascending per slice, the slices merged in fp64): what a correct fp32 implementation gives, used on the CPU to
# check that the allowances hold before a GPU sees them
# ------------------------------------------------------------------------------------------------
def _forward_f32(th, F, H, C, cols, X):
    f = np.float32
    n, B = th.shape[0], X.shape[0]
    w1, b1, w2, b2 = _blocks(th, F, H, C, cols)
    pre = np.broadcast_to(b1[:, None, :], (n, B, H)).astype(f)
    for k in range(F):
        pre = pre + X[None, :, k, None] * w1[:, None, k, :]
    a = np.maximum(pre, f(0))
    z = np.broadcast_to(b2[:, None, :], (n, B, C)).astype(f)
    for h in range(H):
        z = z + a[:, :, h, None] * w2[:, None, h, :]
    assert pre.dtype == f and z.dtype == f
    return pre, a, z


def score_f32(theta, F, H, C, cols, X, labels, scale=1.0, prior_precision=1.0, gamma_rate=0.01):
    f = np.float32
    th, X = np.asarray(theta, f), np.asarray(X, f)
    n = th.shape[0]
    ll = -1 if cols[4] is None else cols[4]
    w1, b1, w2, b2 = _blocks(th, F, H, C, cols)
    pre, a, z = _forward_f32(th, F, H, C, cols, X)
    _, _, p = _softmax_f32(z)
    r = (_onehot(np, labels, C, p) - p).astype(f)          # [n, B, C]
    gb2 = _seq(r, 1)
    gw2 = np.stack([_seq(a[:, :, h, None] * r, 1) for h in range(H)], axis=1)     # [n, H, C]
    D = np.zeros(pre.shape, f)
    for c in range(C):
        D = D + r[:, :, c, None] * w2[:, None, :, c]
    dl = np.where(pre > 0, D, f(0))
    gb1 = _seq(dl, 1)
    gw1 = np.stack([_seq(dl * X[None, :, k, None], 1) for k in range(F)], axis=1)  # [n, F, H]
    prec = np.exp(th[:, ll]) if ll >= 0 else np.full(n, prior_precision, f)
    out = np.zeros_like(th)
    s = f(scale)
    out[:, cols[0]:cols[0] + F * H] = (s * gw1 - prec[:, None, None] * w1).reshape(n, F * H)
    out[:, cols[1]:cols[1] + H] = s * gb1 - prec[:, None] * b1
    out[:, cols[2]:cols[2] + H * C] = (s * gw2 - prec[:, None, None] * w2).reshape(n, H * C)
    out[:, cols[3]:cols[3] + C] = s * gb2 - prec[:, None] * b2
    if ll >= 0:
        sw2 = (_seq((w1 * w1).reshape(n, F * H), -1) + _seq((w2 * w2).reshape(n, H * C), -1)) + _seq(b1 * b1, -1) + _seq(b2 * b2, -1)
        out[:, ll] = f(0.5) * f(F * H + H + H * C + C) - prec * (f(0.5) * sw2 + f(gamma_rate))
    assert out.dtype == f
    return out


def predict_f32(theta, F, H, C, cols, X, labels, per):
    f = np.float32
    th, X = np.asarray(theta, f), np.asarray(X, f)
    n = th.shape[0]
    _, _, z = _forward_f32(th, F, H, C, cols, X)
    t, s, p = _softmax_f32(z)
    Hh = (np.log(s).astype(f) - _seq(p * t, -1)).astype(f)
    out = {"pred_link": z, "pred_mean": p}

    def mean(q):                                           # fp32 per slice, the slices in fp64
        tot = np.zeros(q.shape[1:], np.float64)
        for a0 in range(0, n, per):
            tot += _seq(q[a0:a0 + per], 0).astype(np.float64)
        return tot / n
    out["prob"] = mean(p).astype(f)
    out["ent"] = mean(Hh).astype(f)
    if labels is not None:
        oh = _onehot(np, labels, C, p)
        with np.errstate(invalid="ignore"):
            out["lpd"] = np.log(mean((p * oh).sum(-1).astype(f))).astype(f)
    return out
