"""Stein importance weights (black-box importance sampling, Liu & Lee 2017) and the Stein-kernel products they are built
from, without the n x n matrix (include/steinhip.h, stein_weights and stein_ksd_matmul)."""
import torch

from .. import _lib
from .._checks import bandwidth_to_h2, check_kernel_name
from .stein_test import _check_particles, _check_weights

_KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}


# the bandwidth forms of ksd_quadratic_forms, in the three places both functions below need them
def _parse_bandwidth(bandwidth):
    """a tensor as it is (_check_h2_tensor looks at it once the device is known), else bandwidth_to_h2's float or 'median'"""
    if isinstance(bandwidth, torch.Tensor):
        return bandwidth
    return bandwidth_to_h2(bandwidth, "a positive finite float, a 1-element float32 device tensor (h^2) or \"median\"")


def _check_h2_tensor(h2, dev):
    if isinstance(h2, torch.Tensor) and (h2.numel() != 1 or h2.dtype != torch.float32 or h2.device != dev):
        raise ValueError("bandwidth: a tensor must be a 1-element float32 tensor on %s (the squared bandwidth), got %s %s "
                         "on %s" % (dev, tuple(h2.shape), h2.dtype, h2.device))


def _device_h2(h2, theta, stages):
    """the 1-element float32 device tensor of the squared bandwidth from _parse_bandwidth's result (inside the device
    context): "median" is the library's median heuristic of `theta`, taken without the n x n image"""
    n, d = theta.shape
    if isinstance(h2, str):      # "median"
        from ..stream_engine import StreamEngine
        return StreamEngine(n, d, device=theta.device, h2="median", stages=stages).refresh_bandwidth(theta)
    if not isinstance(h2, torch.Tensor):
        return torch.full((1,), h2, dtype=torch.float32, device=theta.device)
    return h2


def stein_kernel_products(theta, score, V, bandwidth="median", kernel="imq"):
    """out[b, i] = sum_j u_p(x_i, x_j) V[b, j], a float32 device tensor [reps, n], for every row of the float32 device
    tensor `V` [reps, n]; u_p is the Stein kernel of `kernel` ("imq", the default, or "rbf") for the particles `theta` with
    scores `score` = d log p / d theta, both [n, d] float32 device tensors.  The rows U v that importance weights and
    control variates need: with a row w, (out * w).sum() is w^T U w; the control-variate coefficients are a solve of your
    own on these products.  bandwidth, and everything about the call, as in ksd_quadratic_forms; the rows are contracted
    as given (out(-V) may differ from -out(V) in a last bit)."""
    from ..engine import HipStages
    check_kernel_name(kernel)
    h2 = _parse_bandwidth(bandwidth)
    n, d = _check_particles(theta, score)
    dev = theta.device
    _check_weights(V, None, n, dev)
    _check_h2_tensor(h2, dev)
    theta, score, V = theta.contiguous(), score.contiguous(), V.contiguous()
    reps = V.shape[0]
    stages = HipStages()
    with torch.cuda.device(dev):
        h2 = _device_h2(h2, theta, stages)
        ws = torch.empty(_lib.ksd_matmul_workspace_bytes(n, d, reps), dtype=torch.uint8, device=dev)
        out = torch.empty((reps, n), dtype=torch.float32, device=dev)
        stages.ksd_matmul(theta, score, n, d, h2, _KERNEL_IDS[kernel], V, reps, out, ws)
    return out


def stein_importance_weights(theta, score, iters=None, bandwidth="median", kernel="imq", return_path=False):
    """(w, info): the weights w, a float64 device tensor [n] on the simplex, that `iters` Frank-Wolfe steps with an exact
    line search from the uniform weights give for  min_w w^T U w,  the KSD^2 of the weighted sample (U the Stein-kernel
    matrix of the particles `theta` with scores `score`, both [n, d] float32 device tensors).  Use them as
    (w[:, None] * f(theta)).sum(0): they correct a biased or unconverged sample -- SVGD particles stopped early, MCMC output,
    a warm start from another posterior -- and keep every particle.
    info: {"ksd2": w^T U w, "ksd2_uniform": the same for w = 1 / n, "gap": w^T g - min g with g = U w}, Python floats read
    from the device once, at the end; ksd2 - (the least KSD^2 any weights reach) <= 2 gap.  Plain Frank-Wolfe converges as
    O(1 / t): the gap says where you stand.  return_path=True adds "idx" (int64 [iters]) and "gamma" (float64 [iters]), the
    vertex and the length of every step, as device tensors.
    iters: None (default) means 4 n; 0 returns the uniform weights.  bandwidth, kernel: as in stein_thinning.
    iters + 1 launches and two Stein-kernel products on the current stream; an O(n d) workspace is allocated for the call."""
    from ..engine import HipStages
    check_kernel_name(kernel)
    h2 = _parse_bandwidth(bandwidth)
    n, d = _check_particles(theta, score)
    if iters is None:
        iters = 4 * n
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError("iters must be None or an integer >= 0, got %r" % (iters,))
    dev = theta.device
    _check_h2_tensor(h2, dev)
    theta, score = theta.contiguous(), score.contiguous()
    stages = HipStages()
    with torch.cuda.device(dev):
        h2 = _device_h2(h2, theta, stages)
        ws = torch.empty(_lib.weights_workspace_bytes(n, d), dtype=torch.uint8, device=dev)
        w = torch.empty(n, dtype=torch.float64, device=dev)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        idx = torch.empty(iters, dtype=torch.int64, device=dev) if return_path else None
        gamma = torch.empty(iters, dtype=torch.float64, device=dev) if return_path else None
        stages.weights(theta, score, n, d, h2, _KERNEL_IDS[kernel], iters, w, stats, idx, gamma, ws)
        ksd2, gap, uniform = stats.tolist()
    info = {"ksd2": ksd2, "ksd2_uniform": uniform, "gap": gap}
    if return_path:
        info["idx"], info["gamma"] = idx, gamma
    return w, info
