"""The KSD goodness-of-fit test (Chwialkowski et al. 2016; Liu et al. 2016; Gorham & Mackey 2017 for the IMQ kernel): the
V-statistic of the Stein kernel against its wild-bootstrap replicates, without the n x n matrix (include/steinhip.h,
stein_ksd_boot)."""
import torch

from .. import _lib
from .._checks import bandwidth_to_h2, check_kernel_name

_KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}


def _check_particles(theta, score):
    for name, t in (("theta", theta), ("score", score)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a torch tensor" % name)
        if not t.is_cuda:
            raise ValueError("%s must be a device (cuda/HIP) tensor, got %s: the test has no CPU path" % (name, t.device))
        if t.dim() != 2:
            raise ValueError("%s must be [n, d], got %s" % (name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    if theta.shape != score.shape or theta.device != score.device:
        raise ValueError("theta and score must have the same shape and device: %s %s vs %s %s" %
                         (tuple(theta.shape), theta.device, tuple(score.shape), score.device))
    n, d = theta.shape
    if n < 2 or d < 1:
        raise ValueError("need n >= 2 and d >= 1, got n = %d, d = %d" % (n, d))
    return n, d


def _check_weights(weights, rows, n, dev):
    if not isinstance(weights, torch.Tensor) or not weights.is_cuda or weights.dtype != torch.float32 or weights.dim() != 2 \
            or weights.shape[1] != n or (rows is not None and weights.shape[0] != rows) or weights.shape[0] < 1 \
            or weights.device != dev:
        got = (tuple(weights.shape), weights.dtype, weights.device) if isinstance(weights, torch.Tensor) else (weights,)
        raise ValueError("weights must be a float32 tensor [%s, %d] on %s, got %s" %
                         ("reps" if rows is None else rows, n, dev, " ".join(str(g) for g in got)))


def ksd_quadratic_forms(theta, score, weights, bandwidth="median", kernel="imq"):
    """(Q, diag): Q[b] = sum_ij weights[b, i] weights[b, j] u_p(x_i, x_j), a float64 device tensor [reps], for every row of
    the float32 device tensor `weights` [reps, n], and diag = sum_i u_p(x_i, x_i), a 1-element float64 device tensor; u_p is
    the Stein kernel of `kernel` ("imq", the default, or "rbf") for the particles `theta` with scores `score` =
    d log p / d theta, both [n, d] float32 device tensors.  A row of ones gives n^2 KSD^2_V; any finite weights are taken
    (signs, centred multinomial counts).  bandwidth: as in stein_thinning ("median", a positive float h, or a 1-element
    float32 device tensor holding h^2).  One call on the current stream, no host synchronisation; an O(n d + n reps)
    workspace is allocated for the call, the n x n matrix never exists."""
    from ..engine import HipStages
    check_kernel_name(kernel)
    if isinstance(bandwidth, torch.Tensor):
        h2 = bandwidth
    else:
        h2 = bandwidth_to_h2(bandwidth, "a positive finite float, a 1-element float32 device tensor (h^2) or \"median\"")
    n, d = _check_particles(theta, score)
    dev = theta.device
    _check_weights(weights, None, n, dev)
    if isinstance(h2, torch.Tensor) and (h2.numel() != 1 or h2.dtype != torch.float32 or h2.device != dev):
        raise ValueError("bandwidth: a tensor must be a 1-element float32 tensor on %s (the squared bandwidth), got %s %s "
                         "on %s" % (dev, tuple(h2.shape), h2.dtype, h2.device))
    theta, score, weights = theta.contiguous(), score.contiguous(), weights.contiguous()
    reps = weights.shape[0]
    stages = HipStages()
    with torch.cuda.device(dev):
        if isinstance(h2, str):      # "median"
            from ..stream_engine import StreamEngine
            eng = StreamEngine(n, d, device=dev, h2="median", stages=stages)
            h2 = eng.refresh_bandwidth(theta)
        elif not isinstance(h2, torch.Tensor):
            h2 = torch.full((1,), h2, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.ksd_boot_workspace_bytes(n, d, reps), dtype=torch.uint8, device=dev)
        q = torch.empty(reps, dtype=torch.float64, device=dev)
        diag = torch.empty(1, dtype=torch.float64, device=dev)
        stages.ksd_boot(theta, score, n, d, h2, _KERNEL_IDS[kernel], weights, reps, q, diag, ws)
    return q, diag


def sign_processes(n_boot, n, flip_prob, device, generator=None):
    """[n_boot, n] float32 rows of +-1: the first entry is +-1 with equal probability and every next one is the previous
    times -1 with probability flip_prob (0.5: independent Rademacher signs)"""
    first = torch.randint(0, 2, (n_boot, 1), device=device, generator=generator, dtype=torch.int32)
    flips = (torch.rand((n_boot, n - 1), device=device, generator=generator) < flip_prob).to(torch.int32)
    parity = torch.cat([first, flips], dim=1).cumsum(dim=1) & 1
    return (1 - 2 * parity).to(torch.float32)


def stein_goodness_of_fit(theta, score, n_boot=511, bandwidth="median", kernel="imq", statistic="v", flip_prob=0.5,
                          weights=None, generator=None, return_samples=False):
    """(KSD^2, p_value) of the hypothesis that the particles `theta` are draws from the density whose scores at them are
    `score` (both [n, d] float32 device tensors); with return_samples=True also the n_boot bootstrap replicates of the
    statistic (a float64 device tensor).  The replicates are sum_ij w_i w_j u_p(x_i, x_j) under n_boot sign processes w
    (built on the device, `generator` a device torch.Generator for reproducibility): flip_prob = 0.5 gives independent
    Rademacher signs (independent draws); a smaller flip_prob keeps neighbouring signs equal for about 1 / flip_prob draws,
    Chwialkowski et al.'s wild bootstrap for correlated MCMC output.  weights: your own [n_boot, n] float32 device rows
    instead (statistic "v" only).  p = (1 + #{b : Q_b >= Q_0}) / (n_boot + 1); the statistic Q_0 is computed as one more
    row, all ones, of the same call, so both sides of the comparison come out of the same arithmetic.
    statistic: "v" (default) or "u" (the diagonal sum_i u_p(x_i, x_i) removed from the statistic and every replicate).
    bandwidth, kernel: as in ksd_quadratic_forms.  One host read, at the end.  A NaN or infinity in theta or score makes the
    statistic and the p-value NaN."""
    if isinstance(n_boot, bool) or not isinstance(n_boot, int) or n_boot < 1:
        raise ValueError("n_boot must be an integer >= 1, got %r" % (n_boot,))
    if isinstance(flip_prob, bool) or not isinstance(flip_prob, (int, float)) or not 0.0 < float(flip_prob) < 1.0:
        raise ValueError("flip_prob must be a float in (0, 1), got %r" % (flip_prob,))
    if statistic not in ("u", "v"):
        raise ValueError("statistic must be 'u' or 'v'")
    check_kernel_name(kernel)
    n, d = _check_particles(theta, score)
    dev = theta.device
    if weights is not None:
        _check_weights(weights, n_boot, n, dev)
        if statistic == "u":
            raise ValueError("statistic='u' removes sum_i w_i^2 u_p(x_i, x_i), which is the diagonal sum only for sign "
                             "weights; with weights= use statistic='v'")
    with torch.cuda.device(dev):
        if weights is None:
            weights = sign_processes(n_boot, n, float(flip_prob), dev, generator)
        rows = torch.cat([torch.ones((1, n), dtype=torch.float32, device=dev), weights], dim=0)
        q, diag = ksd_quadratic_forms(theta, score, rows, bandwidth=bandwidth, kernel=kernel)
        vals = q / float(n) ** 2 if statistic == "v" else (q - diag) / (float(n) * (n - 1.0))
        count = (vals[1:] >= vals[0]).sum().to(torch.float64)
        stat, hits = torch.stack([vals[0], count]).tolist()
    # a NaN or Inf in theta or score, or a zero bandwidth, makes every form NaN (include/steinhip.h): no comparison counts,
    # which would read as p = 1 / (n_boot + 1) -- a rejection.  A statistic that is not a number has no p-value.
    p = (1.0 + hits) / (n_boot + 1.0) if stat == stat else float("nan")
    return (stat, p, vals[1:]) if return_samples else (stat, p)
