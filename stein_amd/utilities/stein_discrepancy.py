"""Kernelized Stein discrepancy of any particle set, by the step's own fused call (include/steinhip.h, STEIN_FLAG_KSD)."""
import torch


def kernelized_stein_discrepancy(theta, score, statistic="u"):
    """KSD^2 (a float) of the particles `theta` with scores `score` = d log p / d theta, both [n, d] float32 or bfloat16
    device tensors, under the RBF kernel with the median-heuristic bandwidth SVGD uses: statistic "u" (U-statistic,
    unbiased, the default) or "v" (V-statistic).  Runs the fused phi call with the statistic on a transient engine (its
    workspace is allocated for the call: about 4 n^2 bytes for large n) and applies nothing."""
    from ..engine import SvgdEngine
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
    eng = SvgdEngine(n, d, device=theta.device, dtype=theta.dtype, ksd=True)
    with torch.cuda.device(theta.device):
        eng.compute_phi(theta.contiguous(), score.contiguous())
        return float(eng.stein_discrepancy(statistic).item())
