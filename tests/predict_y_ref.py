"""fp64 reference of the predictive distribution of y (csrc/stein_predict_y.hip: stein_predict_*_ycdf and
stein_predict_*_yquantiles) with an a-priori fp32 error allowance per output, and a NumPy float32 emulation of the kernels'
arithmetic and of the 8-ary search.

TEST INFRASTRUCTURE ONLY.  The reference is written against the operations NumPy arrays and torch tensors share, like
tests/predict_ref.py: on the CPU Phi is scipy.special.ndtr (and Phi^-1 scipy.special.ndtri), on the device torch.special.ndtr
in fp64.

    F_b(t) = sum_p w_p Phi((t - z_pb) s_p) / W,   s_p = sqrt(tau_p)

The allowance a_F of one output follows the rules at the top of tests/score_ref.py (u = 2^-24, gamma(m), no safety factor)
and charges, for the kernel's  Phi = 0.5f * erfcf(fl(-fl(1/sqrt 2) * fl(fl(t - z) * s))):
  * the argument: the subtraction, the product with s, the product with the rounded 1/sqrt 2 and that constant's own rounding
    are gamma(4) relative; s itself is u for the linear model (the host's fp64 square root rounded to fp32 once) and
    (EXP_U / 2 + 1) u for the network (sqrt of expf: half of expf's relative error, then sqrt's own rounding; the doubling
    of 1/2 e^lg is exact).  A relative error rho of the argument x moves Phi by at most |x| phi(x) rho <= 0.242 rho;
  * an error dz of z (the forward pass; zero when z is taken from the library's own pred) moves Phi by at most
    dz s phi_max, phi_max = 1 / sqrt(2 pi);
  * erfcf at ERFC_U: the device library's bound is not documented on this platform, so it is charged 16 ulp = 32 u, the OpenCL
    full-profile bound, absolutely (as against Phi <= 1; the halving is exact);
  * fl32(w / W): u on every weight, so u F; nothing for an unweighted call, whose lanes add Phi itself;
  * the running sum of a slice: `per` fma of non-negative terms, gamma(per) F (Phi's own rounding is one of them);
  * the fp64 merge of the slices, the division by n (unweighted) and the rounding of the result to fp32:
    gamma64(slices + 2) F + u F, as tests/predict_ref.py charges its sums;
  * TINY for what underflows (a normalised weight below 2^-126 counts as zero; erfcf's tail).
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as pr  # noqa: E402
import score_ref as sr  # noqa: E402

U, EXP_U, gamma, gamma64, TINY = sr.U, sr.EXP_U, sr.gamma, pr.gamma64, pr.TINY
ERFC_U = 32                      # erfcf charged 16 ulp = 32 u
XPHI_MAX = 0.242                 # max |x| phi(x) = phi(1) = 0.24197...
PHI_MAX = 1.0 / math.sqrt(2.0 * math.pi)
K = 7                            # PY_K of stein_predict_y.hip: interior points per refinement pass
WIDEN = 2.0 ** -21               # PY_WIDEN
POINTS_MAX = LEVELS_MAX = 8
PASSES_MAX = 12
PART_FLOATS = 1 << 23            # PY_PART_FLOATS
ROUND_WGS = 512                  # PY_ROUND_WGS


def _xp(a):
    return sr._xp(a)


def ndtr(x):
    if _xp(x) is np:
        from scipy.special import ndtr as f
        return f(x)
    import torch
    return torch.special.ndtr(x)


def ndtri(q):
    from scipy.special import ndtri as f
    return f(q)


def s_rel(model):
    """relative error of the kernel's s = sqrt(tau) in units of u"""
    return 1.0 if model != "bnn" else EXP_U / 2.0 + 1.0


def norm_weights(w, n, xp=np):
    """-> (w / W in fp64, weighted?) ; w = None: 1 / n each"""
    if w is None:
        return None
    return w / w.sum()


def cdf(t, z, dz, s, w, model, per, slices):
    """-> (F [A, B], a_F [A, B]).  t [A, B]; z, dz [n, B] (dz = 0: z exact); s [n] = sqrt(tau) in fp64; w [n] >= 0 or None."""
    xp = _xp(z)
    n = z.shape[0]
    rho = gamma(4) + s_rel(model) * U
    F, A = [], []
    for i in range(t.shape[0]):
        ph = ndtr((t[i][None, :] - z) * s[:, None])                    # [n, B]
        term = XPHI_MAX * rho + PHI_MAX * s[:, None] * dz
        if w is None:
            Fi, Ti = ph.sum(0) / n, term.sum(0) / n
            wu = 0.0
        else:
            wn = (w / w.sum())[:, None]
            live = (wn > 0)
            Fi = xp.where(live, wn * xp.where(live, ph, xp.zeros_like(ph)), xp.zeros_like(ph)).sum(0)
            Ti = xp.where(live, wn * xp.where(live, term, xp.zeros_like(term)), xp.zeros_like(term)).sum(0)
            wu = U
        F.append(Fi)
        A.append(Ti + ERFC_U * U + (wu + gamma(per) + gamma64(slices + 2) + U) * Fi + n * TINY)
    return xp.stack(F), xp.stack(A)


def component_quantiles(z, s, c):
    """z + c / s, [n, B] in fp64"""
    return z + (c / s)[:, None]


def quantile64(level, z, s, w, iters=64):
    """fp64 bisection of F(t) = level per row -> (t_lo, t_hi) [B] with F(t_lo) < level <= F(t_hi), one fp64 step apart at most
    after `iters` halvings of the span of the component quantiles; level [B] in (0, 1).  -inf / +inf where level <= 0 / >= 1."""
    xp = _xp(z)
    n = z.shape[0]
    wn = None if w is None else (w / w.sum())[:, None]
    live = None if w is None else (wn > 0)
    zz = z if w is None else xp.where(live, z, xp.zeros_like(z))

    def F(t):
        ph = ndtr((t[None, :] - zz) * s[:, None])
        return ph.sum(0) / n if w is None else xp.where(live, wn * ph, xp.zeros_like(ph)).sum(0)
    big = 40.0 / float(s.min())                      # Phi(-40) = 0 and Phi(40) = 1 in fp64
    if w is None:
        lo, hi = pr._amin(z, xp) - big, pr._amax(z, xp) + big
    else:
        inf = xp.full_like(z, float("inf"))
        lo, hi = pr._amin(xp.where(live, z, inf), xp) - big, pr._amax(xp.where(live, z, -inf), xp) + big
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        below = F(mid) < level
        lo, hi = xp.where(below, mid, lo), xp.where(below, hi, mid)
    ninf, pinf = xp.full_like(lo, -float("inf")), xp.full_like(lo, float("inf"))
    lo = xp.where(level <= 0, ninf, xp.where(level >= 1, pinf, lo))
    hi = xp.where(level <= 0, ninf, xp.where(level >= 1, pinf, hi))
    return lo, hi


# ---- the kernels' arithmetic in NumPy float32 ----------------------------------------------------------------------------
f32 = np.float32


def erfc_f32(x):
    from scipy.special import erfc
    return erfc(x.astype(np.float64)).astype(f32)   # a correctly rounded erfcf: the emulation's stand-in for the device's


def s_f32(model, tau=None, lg=None):
    """-> (s, 1 / s) as the kernels hold them"""
    if model != "bnn":
        return f32(math.sqrt(tau)), f32(1.0 / math.sqrt(tau))
    with np.errstate(over="ignore", under="ignore"):
        s = np.sqrt(f32(2.0) * (f32(0.5) * np.exp(lg.astype(f32))).astype(f32)).astype(f32)
        return s, (f32(1.0) / s).astype(f32)


def norm_weights_f32(w):
    """pred_norm_weight: fl32(w / W), flushed below the normal range; W as the weight pass sums it is fp64 (any order: the
    emulation is checked against the allowance, not bit for bit)"""
    q = (np.asarray(w, np.float64) / np.asarray(w, np.float64).sum()).astype(f32)
    return np.where(q >= np.finfo(f32).tiny, q, f32(0.0)).astype(f32)


def phi_f32(x):
    return (f32(0.5) * erfc_f32((f32(-0.70710678118654752440) * x).astype(f32))).astype(f32)


def cdf_f32(t, z, s, w32, per):
    """t [A, B] f32, z [n, B] f32, s [n] or scalar f32, w32 [n] f32 normalised or None -> F-hat [A, B] float64 (the finish
    kernel's fp64 value before the final rounding is rounded here to f32 and returned as such)"""
    n = z.shape[0]
    s = np.broadcast_to(np.asarray(s, f32), (n,))
    tot = np.zeros(t.shape, np.float64)
    for a in range(0, n, per):
        acc = np.zeros(t.shape, f32)
        for p in range(a, min(n, a + per)):
            if w32 is not None and not w32[p] > 0:
                continue
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                ph = phi_f32(((t - z[p][None, :]).astype(f32) * s[p]).astype(f32))
                if w32 is None:
                    acc = (acc + ph).astype(f32)
                else:
                    acc = (acc.astype(np.float64) + w32[p].astype(np.float64) * ph.astype(np.float64)).astype(f32)  # one rounding: fma
        tot += acc
    return tot if w32 is not None else tot / n


def point_f32(lo, hi, j):
    """py_point: one rounding of lo + (hi - lo) j / 8, then min with hi (the fma in fp64: exact product and sum of f32 values
    fit 53 bits unless the exponents are far apart, where the double rounding cannot matter to any assertion made here)"""
    d = (hi - lo).astype(f32)
    p = (lo.astype(np.float64) + d.astype(np.float64) * (0.125 * j)).astype(f32)
    return np.minimum(p, hi)


def bracket_f32(z, s, rs, w32, c):
    """the bracket pass for one level: c = fl32(Phi^-1(level)) -> (lo0, hi0) [B]"""
    n = z.shape[0]
    rs = np.broadcast_to(np.asarray(rs, f32), (n,))
    lo = np.full(z.shape[1], np.inf, f32)
    hi = np.full(z.shape[1], -np.inf, f32)
    for p in range(n):
        if w32 is not None and not w32[p] > 0:
            continue
        o = f32(c) * rs[p]
        cq = (z[p] + o).astype(f32)
        m = (f32(WIDEN) * (np.abs(z[p]) + np.abs(o)).astype(f32)).astype(f32)
        lo = np.fmin(lo, (cq - m).astype(f32))
        hi = np.fmax(hi, (cq + m).astype(f32))
    return lo, hi


def refine_f32(lo, hi, level, z, s, w32, per):
    """one refinement pass of one level -> (lo, hi) [B]"""
    pts = np.stack([point_f32(lo, hi, j) for j in range(1, K + 1)])
    F = cdf_f32(pts, z, s, w32, per)
    nlo, nhi = pts[K - 1].copy(), hi.copy()
    below = lo.copy()
    found = np.zeros(lo.shape, bool)
    for k in range(K):
        take = ~found & (F[k] >= level)
        nlo = np.where(take, below, nlo)
        nhi = np.where(take, pts[k], nhi)
        found |= take
        below = pts[k]
    return nlo.astype(f32), nhi.astype(f32)


def yquantiles_f32(levels, passes, z, s, rs, w32, per):
    """-> (lo [L, B], hi [L, B], lo0, hi0) of the emulated call"""
    lo, hi, lo0, hi0 = [], [], [], []
    for q in levels:
        a, b = bracket_f32(z, s, rs, w32, f32(ndtri(q)))
        lo0.append(a)
        hi0.append(b)
        for _ in range(passes):
            a, b = refine_f32(a, b, q, z, s, w32, per)
        lo.append(a)
        hi.append(b)
    return np.stack(lo), np.stack(hi), np.stack(lo0), np.stack(hi0)


def width_bound(lo1, hi1, passes):
    """the contract hi - lo <= (hi0 - lo0) / 8^passes plus one ulp, with hi0 - lo0 taken as eight times the width after the
    first refinement pass (what a caller can see: a passes=1 call) and the ulp that of the larger end of that bracket"""
    lo1, hi1 = np.asarray(lo1, f32), np.asarray(hi1, f32)
    ulp = np.spacing(np.maximum(np.abs(lo1), np.abs(hi1))).astype(np.float64)
    return 8.0 * (hi1.astype(np.float64) - lo1.astype(np.float64)) / 8.0 ** passes + ulp
