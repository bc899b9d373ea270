"""Stein thinning (Riabiz et al. 2022): the m particles that best represent all n (include/steinhip.h, stein_thin)."""
import torch

from .. import _lib
from .._checks import bandwidth_to_h2, check_kernel_name

_KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}


def stein_thinning(theta, score, m, bandwidth="median", kernel="imq", return_ksd=False):
    """Indices (an int64 device tensor [m]) of the m greedy picks among the particles `theta` with scores `score` =
    d log p / d theta, both [n, d] float32 device tensors: pick t is the particle that most lowers the kernelized Stein
    discrepancy of the first t picks, the lowest index on equal value.  Selection is with replacement -- an index may
    repeat, so m > n is meaningful -- and works on any sample with scores, MCMC output included.  `theta[idx]` is the
    thinned sample, in pick order: every prefix of it is the greedy choice of its own length.
    bandwidth: "median" (default): the library's median-heuristic bandwidth of `theta`, taken without the n x n image
    (stein_stream_median; needs n >= 2).  A positive finite float h (h^2 rounded to float32).  A 1-element float32
    device tensor: the SQUARED bandwidth h2, as the streaming engine's `h2` -- read on the device, never checked.
    kernel: "imq" (default), (1 + D / (2 h^2))^(-1/2), the kernel whose discrepancy controls convergence, or "rbf".
    return_ksd=True: also a float64 device tensor [m], KSD^2 (V-statistic) of the first t picks after each pick.
    m + 1 launches on the current stream, no host synchronisation; an O(n) workspace is allocated for the call."""
    from ..engine import HipStages
    check_kernel_name(kernel)
    if isinstance(bandwidth, torch.Tensor):
        h2 = bandwidth
    else:
        h2 = bandwidth_to_h2(bandwidth, "a positive finite float, a 1-element float32 device tensor (h^2) or \"median\"")
    for name, t in (("theta", theta), ("score", score)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a torch tensor" % name)
        if not t.is_cuda:
            raise ValueError("%s must be a device (cuda/HIP) tensor, got %s: thinning has no CPU path" % (name, t.device))
        if t.dim() != 2:
            raise ValueError("%s must be [n, d], got %s" % (name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    if theta.shape != score.shape or theta.device != score.device:
        raise ValueError("theta and score must have the same shape and device: %s %s vs %s %s" %
                         (tuple(theta.shape), theta.device, tuple(score.shape), score.device))
    n, d = theta.shape
    if n < 1 or d < 1:
        raise ValueError("need n >= 1 and d >= 1, got n = %d, d = %d" % (n, d))
    if isinstance(m, bool) or not isinstance(m, int) or m < 1:
        raise ValueError("m must be an integer >= 1, got %r" % (m,))
    dev = theta.device
    if isinstance(h2, torch.Tensor) and (h2.numel() != 1 or h2.dtype != torch.float32 or h2.device != dev):
        raise ValueError("bandwidth: a tensor must be a 1-element float32 tensor on %s (the squared bandwidth), got %s %s "
                         "on %s" % (dev, tuple(h2.shape), h2.dtype, h2.device))
    theta, score = theta.contiguous(), score.contiguous()
    stages = HipStages()
    with torch.cuda.device(dev):
        if isinstance(h2, str):      # "median"
            if n < 2:
                raise ValueError("n = %d: the median-heuristic bandwidth divides by ln(n); need n >= 2 (or pass a bandwidth)" % n)
            from ..stream_engine import StreamEngine
            eng = StreamEngine(n, d, device=dev, h2="median", stages=stages)
            h2 = eng.refresh_bandwidth(theta)
        elif not isinstance(h2, torch.Tensor):
            h2 = torch.full((1,), h2, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.thin_workspace_bytes(n, d), dtype=torch.uint8, device=dev)
        idx = torch.empty(m, dtype=torch.int64, device=dev)
        ksd2 = torch.empty(m, dtype=torch.float64, device=dev) if return_ksd else None
        stages.thin(theta, score, n, d, h2, _KERNEL_IDS[kernel], m, idx, ksd2, ws)
    return (idx, ksd2) if return_ksd else idx
