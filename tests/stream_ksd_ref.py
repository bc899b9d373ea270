"""The row-sum form of the kernelized Stein discrepancy that the streaming step evaluates (a helper of the streaming KSD
tests, not a test; include/steinhip.h, stein_svgd_phi_stream_ksd).

With x = theta, g = score, w = g - x / h2, r_i = |x_i|^2, D_ij = r_i + r_j - 2 x_i.x_j and k_ij = exp(-D_ij / 2 h2):

    u_ij / k_ij = w_i.w_j - D_ij / (2 h2^2) + b_i + b_j + d / h2,      b_i = g_i.x_i / h2 - r_i / (2 h2^2)

and with ow = (K.W)_e, rs_i = sum_j k_ij, rd_i = sum_j k_ij D_ij, per element e = (i, c):

    S      = sum_e [ w_e ow_e + rs_i (g_e^2 - w_e^2 + 1 / h2) ]  -  sum_i rd_i / (2 h2^2)
    S_diag = sum_e [ g_e^2 + 1 / h2 ]

No K.theta.  `rowsum_sums` evaluates it in fp64; round32=True rounds what the library holds in fp32 -- the distances before
they are exponentiated, and the three sums ow, rs, rd -- and keeps the final per-element accumulation in fp64, as
k_stream_finish_ksd does.
"""
import torch

import ksd_ref as R


def _r32(t):
    return t.to(torch.float32).to(torch.float64)


def rowsum_sums(X, G, h2, round32=False):
    """(S, S_diag) by the row-sum form."""
    X, G = R._f64(X, G)
    h2 = float(h2)
    r = (X * X).sum(1)
    D = r[:, None] + r[None, :] - 2.0 * (X @ X.T)
    if round32:
        D = _r32(D)
    K = torch.exp(-D / (2.0 * h2))
    W = G - X / h2
    ow, rs, rd = K @ W, K.sum(1), (K * D).sum(1)
    if round32:
        ow, rs, rd = _r32(ow), _r32(rs), _r32(rd)
    t = X / h2
    w = G - t
    S = (w * ow + rs[:, None] * (t * (2.0 * G - t) + 1.0 / h2)).sum() - rd.sum() / (2.0 * h2 * h2)
    S_diag = (G * G + 1.0 / h2).sum()
    return float(S), float(S_diag)
