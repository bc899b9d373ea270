"""fp64 reference of the SVGD direction and the kernelized Stein discrepancy under the inverse multiquadric kernel (a helper
of the IMQ tests, not a test; include/steinhip.h, stein_svgd_phi_imq / stein_svgd_phi_imq_ksd).

With c2 = 2 h2, D_ij = |x_i - x_j|^2 (clamped at 0 from below) and u_ij = 1 + D_ij / c2:

    k = u^(-1/2),  k3 = k^3,  k5 = k^5,        grad_{x_j} k(x_j, x_i) = k3_ij (x_i - x_j) / c2
    n phi_i = (K G)_i + [ rs3_i x_i - (K3 X)_i ] / c2,                        rs3_i = sum_j k3_ij
    u_p(i,j) = k g_i.g_j + k3 (g_i - g_j).(x_i - x_j) / c2 + d k3 / c2 - 3 k5 D / c2^2
    S      = sum_e g_e (K G)_e + (2 / c2) sum_e g_e [ rs3_i x_e - (K3 X)_e ] + sum_i [ d rs3_i / c2 - 3 rd5_i / c2^2 ]
    S_diag = sum_e g_e^2 + n d / c2,                                          rd5_i = sum_j k5_ij D_ij

`pair_phi` and `pairwise_sums` build everything from the pairs; `rowsum_sums` is the row-sum form the library evaluates,
and with round32=True a model of its arithmetic: D, k, k3, O1 = K.G, O2 = K3.X, rs3 and rd5 rounded to fp32, k and k3
passed through the hi + lo fp16 split at 2^14 before the products.  Everything takes torch tensors (or arrays) on any
device and computes in fp64; h2 is given.
"""
import torch

PEXP = 14


def _f64(*ts):
    return [torch.as_tensor(t).to(torch.float64) for t in ts]


def _r32(t):
    return t.to(torch.float32).to(torch.float64)


def _split16(t):
    """t (fp64, holding fp32 values in (0, 1]) through the two-term fp16 split at 2^PEXP: (hi + lo) / 2^PEXP"""
    s = t * 2.0 ** PEXP
    hi = s.to(torch.float16).to(torch.float64)
    lo = _r32(s - hi).to(torch.float16).to(torch.float64)
    return (hi + lo) / 2.0 ** PEXP


def sq_dists(X, rows=slice(None)):
    """rows `rows` of D = r_i + r_j - 2 x_i.x_j in fp64, clamped at 0"""
    X, = _f64(X)
    r = (X * X).sum(1)
    return (r[rows, None] + r[None, :] - 2.0 * (X[rows] @ X.T)).clamp_min(0.0)


def median_h2(X):
    """the median-heuristic bandwidth^2 in fp64 (median of all n^2 squared distances -- the mean of the middle two for an
    even count -- over ln n): for CPU runs that have no engine to ask"""
    import math
    D = sq_dists(X).reshape(-1).sort().values
    m = D.numel()
    med = float(D[m // 2]) if m % 2 else 0.5 * float(D[m // 2 - 1] + D[m // 2])
    return med / math.log(X.shape[0])


def kernel(D, h2):
    """(k, k3, k5) of the distances D"""
    k = (1.0 + D / (2.0 * h2)) ** -0.5
    k2 = k * k
    return k, k * k2, k * k2 * k2


def pair_phi(X, G, h2):
    """phi from the pairs' differences (small n): (1 / n) sum_j [ k_ij g_j + k3_ij (x_i - x_j) / c2 ]"""
    X, G = _f64(X, G)
    n = X.shape[0]
    diff = X[:, None, :] - X[None, :, :]
    k, k3, _ = kernel((diff ** 2).sum(-1), h2)
    return (k @ G + (k3[:, :, None] * diff).sum(1) / (2.0 * h2)) / n


def pairwise_u(X, G, h2):
    """[n, n] matrix of the Stein kernel u_p (small n), from the differences"""
    X, G = _f64(X, G)
    d, c2 = X.shape[1], 2.0 * h2
    diff = X[:, None, :] - X[None, :, :]
    D = (diff ** 2).sum(-1)
    k, k3, k5 = kernel(D, h2)
    cross = ((G[:, None, :] - G[None, :, :]) * diff).sum(-1)
    return k * (G @ G.T) + k3 * cross / c2 + d * k3 / c2 - 3.0 * k5 * D / c2 ** 2


def pairwise_sums(X, G, h2, block=2048):
    """(sum_ij u_p, sum_i u_p(i,i), scale) by the direct pair sum, `block` rows at a time.  scale = sum_ij of every term of
    u_p taken with its magnitude: what the GPU tests measure the statistic's error against."""
    X, G = _f64(X, G)
    n, d = X.shape
    c2 = 2.0 * h2
    a = (G * X).sum(1)
    S = scale = 0.0
    for i0 in range(0, n, block):
        rows = slice(i0, i0 + block)
        x, g = X[rows], G[rows]
        D = sq_dists(X, rows)
        k, k3, k5 = kernel(D, h2)
        gg = g @ G.T
        cross = (a[rows, None] + a[None, :] - g @ X.T - x @ G.T) / c2
        S += float((k * gg + k3 * cross + d * k3 / c2 - 3.0 * k5 * D / c2 ** 2).sum())
        scale += float((k * gg.abs() + k3 * cross.abs() + d * k3 / c2 + 3.0 * k5 * D / c2 ** 2).sum())
    S_diag = float((G * G).sum() + n * d / c2)
    return S, S_diag, scale


def statistic(S, S_diag, n, statistic="u"):
    if statistic == "v":
        return S / n ** 2
    if statistic == "u":
        return (S - S_diag) / (n * (n - 1))
    raise ValueError("statistic must be 'u' or 'v'")


def rowsum_sums(X, G, h2, round32=False, block=2048):
    """(S, S_diag, phi, rs3) by the row-sum form, `block` rows at a time.  round32: the model of the library's arithmetic
    described at the top (the per-element accumulation of S stays in fp64, as in k_imq_finish_ksd; phi is rounded to
    fp32 at the end)."""
    X, G = _f64(X, G)
    n, d = X.shape
    c2 = 2.0 * h2
    phi = torch.empty_like(X)
    rs3_all = torch.empty(n, dtype=torch.float64, device=X.device)
    S = 0.0
    for i0 in range(0, n, block):
        rows = slice(i0, i0 + block)
        D = sq_dists(X, rows)
        if round32:
            D = _r32(D)
        k, k3, k5 = kernel(D, h2)
        if round32:
            k = _r32(k)
            k3 = _r32(k * k * k)
            k5 = _r32(k3 * k * k)
            ka, k3a = _split16(k), _split16(k3)
        else:
            ka, k3a = k, k3
        o1, o2, rs3, rd5 = ka @ G, k3a @ X, k3.sum(1), (k5 * D).sum(1)
        if round32:
            o1, o2, rs3, rd5 = _r32(o1), _r32(o2), _r32(rs3), _r32(rd5)
        x, g = X[rows], G[rows]
        dk = rs3[:, None] * x - o2
        phi[rows] = (o1 + dk / c2) / n
        rs3_all[rows] = rs3
        S += float((g * (o1 + 2.0 * dk / c2)).sum() + (d * rs3 / c2 - 3.0 * rd5 / c2 ** 2).sum())
    if round32:
        phi = _r32(phi)
    S_diag = float((G * G).sum() + n * d / c2)
    return S, S_diag, phi, rs3_all


def phi_allowance(phi_ref, rs3, X, h2, tol):
    """per column: tol (|phi_ref_c| + |rs3 o x_c| / (c2 n)) -- the streaming tests' allowance carried over to the two-term
    form rs3 x - K3 X"""
    X, = _f64(X)
    n = X.shape[0]
    return tol * (phi_ref.norm(dim=0) + (rs3[:, None] * X).norm(dim=0) / (2.0 * h2 * n))
