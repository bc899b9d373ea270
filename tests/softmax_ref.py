"""fp64 references of the two softmax-regression calls (csrc/stein_score_softmax.hip, csrc/stein_predict_softmax.hip) with an
a-priori fp32 error allowance per element.

TEST INFRASTRUCTURE ONLY.  Written against the operations NumPy arrays and torch tensors share, as tests/score_ref.py is, so
the same code is the CPU reference (NumPy) and the device reference (torch fp64 on the GPU).  The inputs are fp64 arrays
holding fp32-representable values; the scalar parameters are rounded to fp32 first.  `labels` is an integer array.

The allowance is a derivation by the rules at the head of tests/score_ref.py and carries no safety factor: u = 2^-24,
gamma(m) = m u / (1 - m u); a sum of m rounded terms in any order errs by gamma(m) sum |terms| (gamma(m + 6) when it crosses
the lanes of a wave); expf and logf are charged 2 ulp = 4 u relative (EXP_U, LOG_U); division is correctly rounded.

Shared (z_c = sum_f x_f W_fc, m = max_c z_c, t_c = z_c - m, e_c = exp(t_c), s = sum_c e_c, p_c = e_c / s):
    dz_c    = gamma(F + 6) sum_f |x_f W_fc|          the F-term sum; the score kernel may split it over the lanes of a row
                                                     (gamma(F) in the predictive kernel, whose lane sums it alone)
    delta   = max_c (dz_c + u |t_c|)                 what reaches the exponentials: the error of z_c and the rounding of the
                                                     subtraction z_c - m.  The softmax does not see a common shift, so the
                                                     error of m itself costs nothing.
    dp_c    = 2 p_c (1 - p_c) delta exp(4 delta) + gamma(C + 2 EXP_U + 1) p_c
              The first term is the softmax's sensitivity, sum_j |d p_c / d z_j| = 2 p_c (1 - p_c), times the largest
              perturbation; along the path p_c and 1 - p_c = sum_{j != c} p_j each change by a factor of at most
              exp(2 delta), which the factor exp(4 delta) pays for.  The second is the evaluation: expf above and below
              (EXP_U each), the C-term sum of positive terms, the division.

Score (r_c = 1[y = c] - p_c, g_fc = sum_b x_bf r_bc, out_fc = s g_fc - prec W_fc):
    dr_bc   = dp_bc + u (|r_bc| + dp_bc)             one subtraction
    out_fc +- s sum_b dr_bc |x_bf| (1 + gamma(k)) + gamma(k) (s sum_b |r_bc x_bf| + |prec W_fc|),  k = B + 4 (+ EXP_U when the
              precision is expf(log alpha)): the B-term sum and the prior term, exactly as the GLM of tests/score_ref.py
    alpha entry F C / 2 - prec (sw2 / 2 + rate):  A = gamma(F C + 6 + 3 + EXP_U + 4) prec (sw2 / 2 + rate), allowance
              A + u (|value| + A); the 3 are the adds across the four waves of a particle
    A label outside [0, C): the reference's weight entries are NaN (and the allowance there is NaN: compare with isnan).

Predictive (per = particles per slice, n particles):
    pred    LINK: dz_c.  MEAN: dp_c.
    a slice sum of `per` non-negative fp32 terms q_p with errors dq_p, merged in fp64 and divided by n in fp64:
            Q = 1/n sum_p q_p  +-  1/n sum_p dq_p + gamma(per) 1/n sum_p (q_p + dq_p) + 2^-50 Q       (the fp64 merge: at most
            1024 slices, a division: far below 8 roundings of 2^-53) and the final rounding to fp32, u (Q + all of the above)
    prob_c  q = p_c, dq = dp_c
    lpd     S = 1/n sum_p p_y with the bound dS of the line above without the final rounding (the logarithm is taken in fp64
            of the fp64 quotient): |log(S~) - log(S)| <= -log(1 - dS / S), then the rounding to fp32, u (|lpd| + that)
    ent     q = H = log s - sum_c p_c t_c (both terms >= 0), the entropy through logsumexp and sum p z with the maximum
            taken out of both.  As a function of z it is shift invariant with d H / d z_j = -p_j (log p_j + H), so
            dH = delta exp(4 delta) sum_j p_j |log p_j + H|                        the inputs
               + gamma(C) + EXP_U u + LOG_U u log s                               log s: s is a C-term sum of positive terms
                                                                                  each off by EXP_U u; logf on top
               + (gamma(C + 2 EXP_U + 1) + gamma(C)) sum_c p_c |t_c|              sum p t: the evaluation of p_c, the C FMAs
               + u H                                                              the subtraction
`tight=True` drops dz (the forward sum) and keeps the rest: the allowance of the summaries against fp64 statistics of the
logits the call itself returned.  summaries_of_probs() is the same for prob and lpd against the returned probabilities, which
the kernel sums bit for bit: only the slice sums, the merge and the final roundings remain.
"""
import numpy as np

from score_ref import EXP_U, LANES, U, _f32, _xp, gamma

LOG_U = 4     # logf charged 2 ulp = 4 u relative
WAVES = 3     # adds across the four waves of a particle
F64 = 2.0 ** -50


def _max(xp, a):
    return a.max(-1) if xp is np else a.max(-1).values


def _onehot(xp, labels, C, like):
    """[..., C] of 1[y = c]; a label outside [0, C) gives a row of NaN"""
    if xp is np:
        cls = np.arange(C)
        oh = (np.asarray(labels)[..., None] == cls).astype(like.dtype)
        bad = (np.asarray(labels) < 0) | (np.asarray(labels) >= C)
        oh[bad] = np.nan
        return oh
    cls = xp.arange(C, device=like.device)
    oh = (labels[..., None] == cls).to(like.dtype)
    bad = (labels < 0) | (labels >= C)
    oh[bad] = float("nan")
    return oh


def softmax_parts(z, dz):
    """z, dz [..., C] -> dict of p, dp, t, log s, delta (fp64), by the shared rules of the module docstring"""
    xp = _xp(z)
    C = z.shape[-1]
    m = _max(xp, z)[..., None]
    t = z - m
    e = xp.exp(t)
    s = e.sum(-1)
    p = e / s[..., None]
    delta = _max(xp, dz + U * xp.abs(t))
    grow = xp.exp(4.0 * delta)
    dp = 2.0 * p * (1.0 - p) * (delta * grow)[..., None] + gamma(C + 2 * EXP_U + 1) * p
    return {"p": p, "dp": dp, "t": t, "logs": xp.log(s), "delta": delta, "grow": grow}


def score(theta, w_col, F, C, alpha_col, X, labels, scale=1.0, prior_precision=1.0, gamma_rate=0.01):
    """-> (score [n, d], allowance [n, d]) of stein_score_softmax; alpha_col < 0: the fixed precision"""
    xp = _xp(theta)
    n = theta.shape[0]
    s, rate = _f32(scale), _f32(gamma_rate)
    B = X.shape[0]
    W = theta[:, w_col:w_col + F * C].reshape(n, F, C)
    aX = xp.abs(X)
    z = X @ W                                              # [n, B, C]
    dz = gamma(F + LANES) * (aX @ xp.abs(W))
    sp = softmax_parts(z, dz)
    r = _onehot(xp, labels, C, z) - sp["p"]                # [n, B, C] (the one-hot rows broadcast over the particles)
    dr = sp["dp"] + U * (xp.abs(r) + sp["dp"])
    k = B + 4 + (EXP_U if alpha_col >= 0 else 0)
    prec = xp.exp(theta[:, alpha_col])[:, None, None] if alpha_col >= 0 else _f32(prior_precision)
    g = X.T @ r                                            # [n, F, C]
    out, allow = xp.zeros_like(theta), xp.zeros_like(theta)
    out[:, w_col:w_col + F * C] = (s * g - prec * W).reshape(n, F * C)
    al = s * (aX.T @ dr) * (1.0 + gamma(k)) + gamma(k) * (s * (aX.T @ xp.abs(r)) + xp.abs(prec * W))
    allow[:, w_col:w_col + F * C] = al.reshape(n, F * C)
    if alpha_col >= 0:
        tt = prec[:, 0, 0] * (0.5 * (W * W).sum(-1).sum(-1) + rate)
        val = 0.5 * (F * C) - tt
        A = gamma(F * C + LANES + WAVES + EXP_U + 4) * tt
        out[:, alpha_col] = val
        allow[:, alpha_col] = A + U * (xp.abs(val) + A)
    return out, allow


def _slice_mean(xp, q, dq, per, n, final=True):
    """the mean over the particles (axis 0) of the non-negative terms q with errors dq, as the kernels take it"""
    Q = q.sum(0) / n
    err = dq.sum(0) / n + gamma(per) * (q + dq).sum(0) / n + F64 * Q
    return Q, (err + U * (Q + err)) if final else err


def summaries(z, dz, labels, per, tight=False):
    """the summaries of stein_predict_softmax from the logits z [n, B, C] with error bounds dz -> dict name -> (value,
    allowance): pred_link, pred_mean [n, B, C]; prob [B, C]; ent [B]; lpd [B] when labels is given.  per: particles per slice"""
    xp = _xp(z)
    n, B, C = z.shape
    if tight:
        dz = xp.zeros_like(z)
    sp = softmax_parts(z, dz)
    p, dp, t = sp["p"], sp["dp"], sp["t"]
    out = {"pred_link": (z, dz), "pred_mean": (p, dp)}
    out["prob"] = _slice_mean(xp, p, dp, per, n)
    pt = -(p * t).sum(-1)                                  # >= 0
    H = sp["logs"] + pt
    logp = t - sp["logs"][..., None]
    dH = (sp["delta"] * sp["grow"] * (p * xp.abs(logp + H[..., None])).sum(-1)
          + gamma(C) + EXP_U * U + LOG_U * U * sp["logs"]
          + (gamma(C + 2 * EXP_U + 1) + gamma(C)) * pt + U * H)
    out["ent"] = _slice_mean(xp, H, dH, per, n)
    if labels is not None:
        oh = _onehot(xp, labels, C, z)
        out["lpd"] = _lpd(xp, (p * oh).sum(-1), (dp * oh).sum(-1), per, n)
    return out


def _lpd(xp, py, dpy, per, n):
    S, dS = _slice_mean(xp, py, dpy, per, n, final=False)
    val = xp.log(S)
    rel = dS / S
    d = -xp.log1p(-rel) if xp is not np else -np.log1p(-np.minimum(rel, 0.5))
    return val, d + U * (xp.abs(val) + d)


def predict(theta, w_col, F, C, X, labels, per):
    """-> the dict of summaries() for stein_predict_softmax's arguments (fp64 logits, dz = gamma(F) |X| |W|)"""
    xp = _xp(theta)
    n = theta.shape[0]
    W = theta[:, w_col:w_col + F * C].reshape(n, F, C)
    z = X @ W
    dz = gamma(F) * (xp.abs(X) @ xp.abs(W))
    return summaries(z, dz, labels, per)


def summaries_of_probs(p, labels, per):
    """prob and lpd against the probabilities the call itself returned (fp64 copies of its fp32 pred): the kernel sums these
    very floats, so only the slice sums, the merge and the final roundings remain -> {"prob": (v, allow), "lpd": (v, allow)}"""
    xp = _xp(p)
    n, _, C = p.shape
    zero = xp.zeros_like(p)
    out = {"prob": _slice_mean(xp, p, zero, per, n)}
    if labels is not None:
        oh = _onehot(xp, labels, C, p)
        out["lpd"] = _lpd(xp, (p * oh).sum(-1), (zero * oh).sum(-1), per, n)
    return out


# ------------------------------------------------------------------------------------------------
# the same formulas in NumPy float32 in the kernels' summation order (features ascending per lane and the lanes of a row
# summed as a tree; rows ascending; particles ascending per slice, the slices merged in fp64): what a correct fp32
# implementation gives, used on the CPU to check that the allowances hold before a GPU sees them
# ------------------------------------------------------------------------------------------------
def _seq(terms, axis):
    return np.take(np.cumsum(terms, axis=axis, dtype=np.float32), -1, axis=axis)


def _logits_f32(X, W, G=1):
    f = np.float32
    n, F, C = W.shape
    parts = []
    for j in range(G):                                     # lane j: f = j, j + G, ...
        idx = np.arange(j, F, G)
        if len(idx) == 0:
            parts.append(np.zeros((n, X.shape[0], C), f))
            continue
        parts.append(_seq(X[None, :, idx, None] * W[:, None, idx, :], 2))
    while len(parts) > 1:                                  # the xor tree of the shuffles, widest stride first
        half = len(parts) // 2
        parts = [parts[i] + parts[i + half] for i in range(half)]
    return parts[0].astype(f)


def _softmax_f32(z):
    f = np.float32
    t = (z - z.max(-1, keepdims=True)).astype(f)
    e = np.exp(t).astype(f)
    s = _seq(e, -1)
    return t, s, (e / s[..., None]).astype(f)


def score_f32(theta, w_col, F, C, alpha_col, X, labels, scale=1.0, prior_precision=1.0, gamma_rate=0.01, G=1):
    f = np.float32
    th, X = np.asarray(theta, f), np.asarray(X, f)
    n = th.shape[0]
    W = th[:, w_col:w_col + F * C].reshape(n, F, C)
    _, _, p = _softmax_f32(_logits_f32(X, W, G))
    r = (_onehot(np, labels, C, p) - p).astype(f)
    g = _seq(X[None, :, :, None] * r[:, :, None, :], 1)    # [n, F, C]
    prec = np.exp(th[:, alpha_col])[:, None, None] if alpha_col >= 0 else f(prior_precision)
    out = np.zeros_like(th)
    out[:, w_col:w_col + F * C] = (f(scale) * g - prec * W).reshape(n, F * C)
    if alpha_col >= 0:
        out[:, alpha_col] = f(0.5) * f(F * C) - prec[:, 0, 0] * (f(0.5) * _seq((W * W).reshape(n, F * C), -1) + f(gamma_rate))
    assert out.dtype == f
    return out


def predict_f32(theta, w_col, F, C, X, labels, per):
    f = np.float32
    th, X = np.asarray(theta, f), np.asarray(X, f)
    n = th.shape[0]
    W = th[:, w_col:w_col + F * C].reshape(n, F, C)
    z = _logits_f32(X, W)
    t, s, p = _softmax_f32(z)
    H = (np.log(s).astype(f) - _seq(p * t, -1)).astype(f)
    out = {"pred_link": z, "pred_mean": p}

    def mean(q):                                           # fp32 per slice, the slices in fp64
        tot = np.zeros(q.shape[1:], np.float64)
        for a in range(0, n, per):
            tot += _seq(q[a:a + per], 0).astype(np.float64)
        return tot / n
    out["prob"] = mean(p).astype(f)
    out["ent"] = mean(H).astype(f)
    if labels is not None:
        oh = _onehot(np, labels, C, p)
        with np.errstate(invalid="ignore"):
            out["lpd"] = np.log(mean((p * oh).sum(-1).astype(f))).astype(f)
    return out
