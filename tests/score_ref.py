"""fp64 references of the two score producers (csrc/stein_score.hip) with an a-priori fp32 error allowance per element.

TEST INFRASTRUCTURE ONLY.  Every function is vectorised over the particles and written against the operations NumPy
arrays and torch tensors share, so the same code is the CPU reference (NumPy) and the device reference (torch fp64 on
the GPU, where n = 65 545 particles cost nothing).  The inputs are fp64 arrays holding fp32-representable values (what
the kernel reads); the scalar parameters are rounded to fp32 first, because the C ABI evaluates in fp32.

The allowance is a derivation, not a measurement, and carries no safety factor.  Its rules:

  * u = 2^-24 is the unit roundoff of fp32, gamma(m) = m u / (1 - m u).
  * A sum of m rounded terms taken in any order errs by at most gamma(m) * sum |terms| (adding a zero is exact, so
    idle lanes cost nothing; a product feeding the sum counts as one of the m roundings).  A sum that is reduced
    across the lanes of a particle group is charged gamma(m + 6): the six are the shuffle adds of a 64-lane group.
  * expf: the ROCm documents installed with the toolchain state no ulp bound for it, so it is charged 2 ulp, which is
    a relative error of 4 u (EXP_U below).  Division and square root are correctly rounded (u).
  * A product or quotient of k rounded factors carries gamma(k) relative error; errors already present in an operand
    are propagated through the formulas of the header comment of stein_score.hip, first order terms explicitly and
    the cross terms through |x| + dx in place of |x|.

GLM (z_b = x_b . w, r_b the residual, g_c = sum_b r_b x_bc, out_c = s g_c - prec w_c):
    dz_b   = gamma(F + 6) sum_c |w_c x_bc|
    dr_b   = dz_b / 4 + gamma(4) (|y_b| + 1)           logistic: sigmoid is 1/4-Lipschitz; expf (4 u, damped by
                                                       sigma (1 - sigma) <= 1/4 to u), 1 + e, the division and the
                                                       subtraction of a value bounded by |y_b| + 1 are the four
    dr_b   = dz_b + u (|r_b| + dz_b)                   linear: one subtraction; |r_b| is not bounded by |y_b| + 1 here
    out_c +- s sum_b dr_b |x_bc| (1 + gamma(k)) + gamma(k) (s sum_b |r_b x_bc| + |prec w_c|),   k = B + 4 (+ 4 when the
                                                       precision is expf(log alpha))
    alpha entry F/2 - prec (sw2 / 2 + rate):  A = gamma(F + 6 + 4 + 4) prec (sw2 / 2 + rate), allowance A + u (|value| + A)

BNN (z_bh = b1_h + sum_f x_bf w1_fh, a = relu(z), m = [z > 0], e_b = y_b - pred_b; cg = s gamma):
    dz_bh    = gamma(F + 1) (|b1_h| + sum_f |x_bf w1_fh|)
    dpred_b  = sum_h dz_bh |w2_h| + gamma(H + 7) (sum_h |a_bh w2_h| + |b2|)
    de_b     = dpred_b + u (|e_b| + dpred_b);  E_b = |e_b| + de_b,  A_bh = a_bh + dz_bh
    sum_b e_b         +- sum_b de_b + gamma(B) sum_b E_b
    sum_b e_b^2       +- sum_b (E_b^2 - e_b^2) + gamma(B) sum_b E_b^2
    sum_b e_b a_bh    +- sum_b (E_b A_bh - |e_b| a_bh) + gamma(B) sum_b E_b A_bh
    sum_b m e_b w2_h [x_bf]  +- sum_b m de_b |w2_h| [|x_bf|] + gamma(B + 1) sum_b m E_b |w2_h| [|x_bf|]
                             + sum over the AMBIGUOUS b of E_b |w2_h| [|x_bf|]
    every block (cg G - lambda W) / n_train:  (cg (E_G + gamma(10) (|G| + E_G)) + gamma(10) lambda |W|) / n_train
    (cg: the division n_train / B, expf and a product; then a product, the subtraction, 1 / n_train and a product)
    log_gamma and log_lambda entries: the same rules over their four terms, gamma(12) and gamma(P + 6 + 10).

ReLU masks: a (b, h) with |z_bh| <= dz_bh is ambiguous -- a correct fp32 evaluation may take either branch, which
moves the b1_h entry by the whole term cg |e_b w2_h| and the w1_fh entries by cg |e_b w2_h x_bf| (the factor is 1 for
b1 and |x_bf| for w1: both are covered by the issue's max(1, |x_bf|)).  Those terms are added to the allowance of
exactly these entries; bnn_score also returns the share of live entries so touched, which the tests cap at 2 %.
"""
import numpy as np

U = 2.0 ** -24
EXP_U = 4     # expf charged 2 ulp = 4 u relative
LANES = 6     # shuffle adds of a 64-lane group


def gamma(m):
    return m * U / (1.0 - m * U)


def _xp(a):
    if type(a).__module__.split(".")[0] == "torch":
        import torch
        return torch
    return np


def _f32(v):
    return float(np.float32(v))


def glm_score(theta, kind, w_col, F, alpha_col, X, y, scale=1.0, prior_precision=1.0, gamma_rate=0.01, row_weight=None):
    """-> (score [n, d], allowance [n, d]) of stein_score_glm.  kind "linear" | "logistic"; alpha_col < 0: fixed precision.
    row_weight [B] multiplies the rows' contributions to the gradient (0 drops a row); the allowance ignores it."""
    xp = _xp(theta)
    s, rate = _f32(scale), _f32(gamma_rate)
    B = X.shape[0]
    w = theta[:, w_col:w_col + F]
    aX = xp.abs(X)
    z = w @ X.T                                           # [n, B]
    dz = gamma(F + LANES) * (xp.abs(w) @ aX.T)
    if kind == "logistic":
        r = y - 1.0 / (1.0 + xp.exp(-z))
        dr = 0.25 * dz + gamma(4) * (xp.abs(y) + 1.0)
    else:
        r = y - z
        dr = dz + U * (xp.abs(r) + dz)
    if row_weight is not None:
        r = r * row_weight
    k = B + 4 + (EXP_U if alpha_col >= 0 else 0)
    prec = xp.exp(theta[:, alpha_col])[:, None] if alpha_col >= 0 else _f32(prior_precision)
    score, allow = xp.zeros_like(theta), xp.zeros_like(theta)
    score[:, w_col:w_col + F] = s * (r @ X) - prec * w
    allow[:, w_col:w_col + F] = (s * (dr @ aX) * (1.0 + gamma(k)) + gamma(k) * (s * (xp.abs(r) @ aX) + xp.abs(prec * w)))
    if alpha_col >= 0:
        t = prec[:, 0] * (0.5 * (w * w).sum(-1) + rate)
        val = 0.5 * F - t
        A = gamma(F + LANES + EXP_U + 4) * t
        score[:, alpha_col] = val
        allow[:, alpha_col] = A + U * (xp.abs(val) + A)
    return score, allow


BNN_ORDER = ("w1", "b1", "w2", "b2", "log_lambda", "log_gamma")


def bnn_score(theta, n_in, H, cols, X, y, n_train, ga=1.0, gb=0.01, row_weight=None):
    """-> (score [n, d], allowance [n, d], share) of stein_score_bnn; cols = first column of BNN_ORDER's blocks.
    share: the fraction of the live (model) entries whose allowance holds the whole term of an ambiguous ReLU mask."""
    xp = _xp(theta)
    n = theta.shape[0]
    F, B = n_in, X.shape[0]
    c = dict(zip(BNN_ORDER, cols))
    nt, a0, b0 = _f32(n_train), _f32(ga), _f32(gb)
    w1 = theta[:, c["w1"]:c["w1"] + F * H].reshape(n, F, H)
    b1, w2, b2 = theta[:, c["b1"]:c["b1"] + H], theta[:, c["w2"]:c["w2"] + H], theta[:, c["b2"]]
    lam, gam = xp.exp(theta[:, c["log_lambda"]]), xp.exp(theta[:, c["log_gamma"]])
    aX, aw2 = xp.abs(X), xp.abs(w2)[:, None, :]
    z = X @ w1 + b1[:, None, :]                           # [n, B, H]
    dz = gamma(F + 1) * (aX @ xp.abs(w1) + xp.abs(b1)[:, None, :])
    a = xp.maximum(z, xp.zeros_like(z))
    m = (z > 0).to(z.dtype) if xp is not np else (z > 0).astype(z.dtype)
    amb = xp.abs(z) <= dz
    amb = amb.to(z.dtype) if xp is not np else amb.astype(z.dtype)
    pred = (a * w2[:, None, :]).sum(-1) + b2[:, None]     # [n, B]
    dpred = (dz * aw2).sum(-1) + gamma(H + LANES + 1) * ((a * aw2).sum(-1) + xp.abs(b2)[:, None])
    e = y - pred
    de = dpred + U * (xp.abs(e) + dpred)
    E = xp.abs(e) + de
    ew = e if row_weight is None else e * row_weight
    se, E_se = ew.sum(-1), de.sum(-1) + gamma(B) * E.sum(-1)
    se2, E_se2 = (ew * e).sum(-1), (E * E - e * e).sum(-1) + gamma(B) * (E * E).sum(-1)
    A = a + dz
    gw2 = (ew[:, None, :] @ a)[:, 0, :]                   # [n, H]
    EA = (E[:, None, :] @ A)[:, 0, :]
    E_gw2 = EA - (xp.abs(e)[:, None, :] @ a)[:, 0, :] + gamma(B) * EA
    t = m * ew[:, :, None] * w2[:, None, :]               # [n, B, H]
    tb = E[:, :, None] * aw2
    D = m * de[:, :, None] * aw2 + gamma(B + 1) * m * tb + amb * tb
    gb1, E_gb1 = t.sum(1), D.sum(1)
    gw1, E_gw1 = X.T @ t, aX.T @ D                        # [n, F, H]

    s = nt / B
    cg, inv = s * gam, 1.0 / nt
    g10 = gamma(10)

    def block(G, EG, W, cgx, lamx):
        return (cgx * G - lamx * W) * inv, (cgx * (EG + g10 * (xp.abs(G) + EG)) + g10 * lamx * xp.abs(W)) * inv

    score, allow = xp.zeros_like(theta), xp.zeros_like(theta)
    v, al = block(gw1, E_gw1, w1, cg[:, None, None], lam[:, None, None])
    score[:, c["w1"]:c["w1"] + F * H], allow[:, c["w1"]:c["w1"] + F * H] = v.reshape(n, F * H), al.reshape(n, F * H)
    v, al = block(gb1, E_gb1, b1, cg[:, None], lam[:, None])
    score[:, c["b1"]:c["b1"] + H], allow[:, c["b1"]:c["b1"] + H] = v, al
    v, al = block(gw2, E_gw2, w2, cg[:, None], lam[:, None])
    score[:, c["w2"]:c["w2"] + H], allow[:, c["w2"]:c["w2"] + H] = v, al
    v, al = block(se, E_se, b2, cg, lam)
    score[:, c["b2"]], allow[:, c["b2"]] = v, al
    g12 = gamma(12)
    score[:, c["log_gamma"]] = (s * (0.5 * B - 0.5 * gam * se2) + (a0 - 1.0) - b0 * gam) * inv
    allow[:, c["log_gamma"]] = inv * (s * 0.5 * gam * E_se2 * (1.0 + g12)
                                      + g12 * (s * 0.5 * B + s * 0.5 * gam * xp.abs(se2) + abs(a0 - 1.0) + b0 * gam))
    P = F * H + 2 * H + 1
    sw2 = (w1 * w1).sum(-1).sum(-1) + (b1 * b1).sum(-1) + (w2 * w2).sum(-1) + b2 * b2
    score[:, c["log_lambda"]] = (0.5 * P - 0.5 * lam * sw2 + (a0 - 1.0) - b0 * lam) * inv
    allow[:, c["log_lambda"]] = inv * gamma(P + LANES + 10) * (0.5 * P + 0.5 * lam * sw2 + abs(a0 - 1.0) + b0 * lam)
    touched = float((amb.sum(1) > 0).sum()) * (1 + F)
    return score, allow, touched / float(n * (P + 2))


# ------------------------------------------------------------------------------------------------
# the same formulas in NumPy float32 with sequential accumulation (np.cumsum adds left to right in the array's type):
# what a correct fp32 implementation gives, used on the CPU to check that the allowance holds before a GPU sees it
# ------------------------------------------------------------------------------------------------
def _seq(terms, axis):
    return np.take(np.cumsum(terms, axis=axis, dtype=np.float32), -1, axis=axis)


def glm_score_f32(theta, kind, w_col, F, alpha_col, X, y, scale=1.0, prior_precision=1.0, gamma_rate=0.01):
    f = np.float32
    th, X, y = np.asarray(theta, f), np.asarray(X, f), np.asarray(y, f)
    w = th[:, w_col:w_col + F]
    with np.errstate(over="ignore"):
        z = _seq(w[:, None, :] * X[None, :, :], -1)       # [n, B]
        r = y - f(1) / (f(1) + np.exp(-z)) if kind == "logistic" else y - z
        g = _seq(r[:, :, None] * X[None, :, :], 1)        # [n, F]
    prec = np.exp(th[:, alpha_col])[:, None] if alpha_col >= 0 else f(prior_precision)
    out = np.zeros_like(th)
    out[:, w_col:w_col + F] = f(scale) * g - prec * w
    if alpha_col >= 0:
        out[:, alpha_col] = f(0.5) * f(F) - prec[:, 0] * (f(0.5) * _seq(w * w, -1) + f(gamma_rate))
    assert out.dtype == f
    return out


def bnn_score_f32(theta, n_in, H, cols, X, y, n_train, ga=1.0, gb=0.01):
    f = np.float32
    th, X, y = np.asarray(theta, f), np.asarray(X, f), np.asarray(y, f)
    n, F, B = th.shape[0], n_in, X.shape[0]
    c = dict(zip(BNN_ORDER, cols))
    w1 = th[:, c["w1"]:c["w1"] + F * H].reshape(n, F, H)
    b1, w2, b2 = th[:, c["b1"]:c["b1"] + H], th[:, c["w2"]:c["w2"] + H], th[:, c["b2"]]
    lam, gam = np.exp(th[:, c["log_lambda"]]), np.exp(th[:, c["log_gamma"]])
    z = np.broadcast_to(b1[:, None, :], (n, B, H)).copy()
    for k in range(F):
        z += X[None, :, k, None] * w1[:, None, k, :]
    a = np.maximum(z, f(0))
    e = y - (_seq(a * w2[:, None, :], -1) + b2[:, None])
    se, se2 = _seq(e, -1), _seq(e * e, -1)
    gw2 = _seq(e[:, :, None] * a, 1)
    t = np.where(z > 0, e[:, :, None] * w2[:, None, :], f(0))
    gb1 = _seq(t, 1)
    gw1 = np.stack([_seq(t * X[None, :, k, None], 1) for k in range(F)], axis=1)
    s = f(n_train) / f(B)
    cg, inv = s * gam, f(1) / f(n_train)
    out = np.zeros_like(th)
    out[:, c["w1"]:c["w1"] + F * H] = ((cg[:, None, None] * gw1 - lam[:, None, None] * w1) * inv).reshape(n, F * H)
    out[:, c["b1"]:c["b1"] + H] = (cg[:, None] * gb1 - lam[:, None] * b1) * inv
    out[:, c["w2"]:c["w2"] + H] = (cg[:, None] * gw2 - lam[:, None] * w2) * inv
    out[:, c["b2"]] = (cg * se - lam * b2) * inv
    out[:, c["log_gamma"]] = (s * (f(0.5) * f(B) - f(0.5) * gam * se2) + (f(ga) - f(1)) - f(gb) * gam) * inv
    P = f(F * H + 2 * H + 1)
    sw2 = _seq((w1 * w1).reshape(n, F * H), -1) + _seq(b1 * b1, -1) + _seq(w2 * w2, -1) + b2 * b2
    out[:, c["log_lambda"]] = (f(0.5) * P - f(0.5) * lam * sw2 + (f(ga) - f(1)) - f(gb) * lam) * inv
    assert out.dtype == f
    return out
