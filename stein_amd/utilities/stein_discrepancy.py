"""Kernelized Stein discrepancy of any particle set, by the step's own fused call (include/steinhip.h, STEIN_FLAG_KSD)."""
import torch

from .._checks import bandwidth_to_h2, check_kernel_name


def kernelized_stein_discrepancy(theta, score, statistic="u", bandwidth=None, kernel="rbf"):
    """KSD^2 (a float) of the particles `theta` with scores `score` = d log p / d theta, both [n, d] float32 or bfloat16
    device tensors, under the RBF kernel with the median-heuristic bandwidth SVGD uses: statistic "u" (U-statistic,
    unbiased, the default) or "v" (V-statistic).  Runs the fused phi call with the statistic on a transient engine (its
    workspace is allocated for the call: about 4 n^2 bytes for large n) and applies nothing.
    bandwidth: None (default) is the above.  A positive finite float h (K = exp(-D / (2 h^2)), h^2 rounded to float32) or
    "median" (the exact median heuristic, taken without the n x n image) runs the streaming step's statistic instead
    (stein_svgd_phi_stream_ksd with phi = NULL) in an O(n d) workspace: float32 inputs only.
    kernel: "rbf" (default) or "imq": the statistic under the inverse multiquadric kernel (1 + D / (2 h^2))^(-1/2) at the
    same bandwidth (stein_svgd_phi_imq_ksd with phi = NULL) -- the kernel whose discrepancy detects non-convergence for
    d >= 3.  It runs on the streaming path only: bandwidth=None then means "median"."""
    from ..engine import SvgdEngine
    check_kernel_name(kernel)
    if kernel == "imq" and bandwidth is None:
        bandwidth = "median"
    h2 = bandwidth_to_h2(bandwidth, "None, a positive finite float or \"median\"") if bandwidth is not None else None
    if h2 is not None:
        for name, t in (("theta", theta), ("score", score)):
            if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16:
                raise ValueError("bandwidth=: the streaming statistic takes float32 inputs; %s is bfloat16 (bf16 inputs "
                                 "are only supported with bandwidth=None)" % name)
    for name, t in (("theta", theta), ("score", score)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a torch tensor" % name)
        if not t.is_cuda:
            raise ValueError("%s must be a device (cuda/HIP) tensor, got %s: the statistic has no CPU path" % (name, t.device))
        if t.dim() != 2:
            raise ValueError("%s must be [n, d], got %s" % (name, tuple(t.shape)))
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("%s must be float32 or bfloat16, got %s" % (name, t.dtype))
    if theta.shape != score.shape or theta.dtype != score.dtype or theta.device != score.device:
        raise ValueError("theta and score must have the same shape, dtype and device: %s %s %s vs %s %s %s" %
                         (tuple(theta.shape), theta.dtype, theta.device, tuple(score.shape), score.dtype, score.device))
    n, d = theta.shape
    if n < 2:
        raise ValueError("n = %d: the statistic needs at least two particles" % n)
    if statistic not in ("u", "v"):
        raise ValueError("statistic must be 'u' or 'v'")
    if h2 is not None:
        eng = SvgdEngine(n, d, device=theta.device, h2=h2, kernel=kernel)
        with torch.cuda.device(theta.device):
            eng.stream_discrepancy_sums(theta.contiguous(), score.contiguous())
            return float(eng.stein_discrepancy(statistic).item())
    eng = SvgdEngine(n, d, device=theta.device, dtype=theta.dtype, ksd=True)
    with torch.cuda.device(theta.device):
        eng.compute_phi(theta.contiguous(), score.contiguous())
        return float(eng.stein_discrepancy(statistic).item())
