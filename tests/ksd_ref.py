"""fp64 reference of the kernelized Stein discrepancy under SVGD's RBF kernel (a helper of the KSD tests, not a test).

    u_ij = k_ij [ g_i.g_j + (g_i - g_j).(x_i - x_j)/h2 + d/h2 - D_ij/h2^2 ],   k_ij = exp(-D_ij / 2 h2)
    KSD^2_V = sum_ij u_ij / n^2,    KSD^2_U = sum_{i != j} u_ij / (n (n - 1))

`pairwise_u` / `pairwise_sums` build u from the pairs (O(n^2 d)); `elementwise_sums` is the per-element form the library
evaluates (include/steinhip.h, STEIN_FLAG_KSD) from K.G, K.theta and rowsum(K).  Everything takes torch tensors (or
arrays) on any device and computes in fp64; h2 is given (the GPU tests pass the engine's own bandwidth).
"""
import torch


def _f64(*ts):
    return [torch.as_tensor(t).to(torch.float64) for t in ts]


def pairwise_u(X, G, h2):
    """[n, n] matrix of u_ij (fp64), from the differences x_i - x_j."""
    X, G = _f64(X, G)
    d = X.shape[1]
    diff = X[:, None, :] - X[None, :, :]
    D = (diff ** 2).sum(-1)
    K = torch.exp(-D / (2.0 * h2))
    cross = ((G[:, None, :] - G[None, :, :]) * diff).sum(-1)
    return K * (G @ G.T + cross / h2 + d / h2 - D / h2 ** 2)


def statistic(S, S_diag, n, statistic="u"):
    """KSD^2 from the two sums: "v" (all pairs) or "u" (off-diagonal pairs)."""
    if statistic == "v":
        return S / n ** 2
    if statistic == "u":
        return (S - S_diag) / (n * (n - 1))
    raise ValueError("statistic must be 'u' or 'v'")


def pairwise_sums(X, G, h2, block=2048):
    """(sum_ij u_ij, sum_i u_ii, scale) by the direct pair sum, `block` rows at a time (fits C3 on a device).  scale =
    sum_ij of every term of u_ij taken with its magnitude: what the GPU tests measure the statistic's error against."""
    X, G = _f64(X, G)
    n, d = X.shape
    r = (X * X).sum(1)
    a = (G * X).sum(1)
    S = scale = 0.0
    for i0 in range(0, n, block):
        x, g = X[i0:i0 + block], G[i0:i0 + block]
        D = (r[i0:i0 + block, None] + r[None, :] - 2.0 * (x @ X.T)).clamp_min(0.0)
        K = torch.exp(-D / (2.0 * h2))
        gg = g @ G.T
        cross = (a[i0:i0 + block, None] + a[None, :] - g @ X.T - x @ G.T) / h2
        S += float((K * (gg + cross + d / h2 - D / h2 ** 2)).sum())
        scale += float((K * (gg.abs() + cross.abs() + d / h2 + D / h2 ** 2)).sum())
    S_diag = float(((G * G).sum(1) + d / h2).sum())
    return S, S_diag, scale


def elementwise_sums(X, G, h2, rows=None):
    """The per-element form: with og = (K.G)_e, ot = (K.X)_e, rs = rowsum(K)_i, th = x_e, dk = (rs th - ot) / h2,
        S      = sum_e [ g_e og + 2 (g_e - th / h2) dk + rs / h2 ]
        S_diag = sum_e [ g_e^2 + 1 / h2 ]
    over the elements e = (i, c) of the rows `rows` (a slice; None = all): a row block's share.  The shares of a
    partition of the rows sum to the total; one share alone is not sum_{i in rows, j} u_ij."""
    X, G = _f64(X, G)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = torch.exp(-D / (2.0 * h2))
    sl = rows if rows is not None else slice(None)
    k = K[sl]
    og, ot, rs = k @ G, k @ X, k.sum(1, keepdim=True)
    th, g = X[sl], G[sl]
    dk = (rs * th - ot) / h2
    S = (g * og + 2.0 * (g - th / h2) * dk + rs / h2).sum()
    S_diag = (g * g + 1.0 / h2).sum()
    return float(S), float(S_diag)


def median_h2(X):
    """The median-heuristic bandwidth^2 in fp64 (median of all n^2 squared distances, mean of the middle two for an even
    count, over ln n): for CPU runs that have no engine to ask."""
    import math
    X, = _f64(X)
    n = X.shape[0]
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).reshape(-1).sort().values
    m = D.numel()
    med = float(D[m // 2]) if m % 2 else 0.5 * float(D[m // 2 - 1] + D[m // 2])
    return med / math.log(n)
