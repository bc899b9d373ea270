"""Stein importance weights of an SVGD run stopped early: a better estimate from the same particles.

    python examples/stein_importance_weights/main.py [--particles 1024] [--iters 60] [--fw-iters K]

runs the sampler of examples/logistic_regression (synthetic data of Covertype's shape, HIP score producer) for a few steps
only, then asks SteinSampler.importance_weights (stein_amd.utilities.stein_importance_weights: Frank-Wolfe with an exact line
search on w^T U w under the IMQ kernel at the median bandwidth, full-data score) for the weights and prints KSD^2 of the
uniform and of the weighted particles with the duality gap, the effective sample size 1 / sum w^2, and the held-out
accuracy and mean log predictive density of the weighted against the unweighted ensemble.
"""
import argparse
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from stein_amd.optimizers import AdamGradientDescent  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import GlmScore  # noqa: E402


def logistic_example():
    spec = importlib.util.spec_from_file_location("logistic_main", os.path.join(HERE, "..", "logistic_regression", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=60, help="SVGD steps before the run is stopped")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--fw-iters", type=int, default=None, help="Frank-Wolfe steps (default: 4 x particles)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    dev = "cuda"
    (Xtr, ytr), (Xte, yte) = logistic_example().make_data()
    Xtr_t, ytr_t = torch.tensor(Xtr, dtype=torch.float32, device=dev), torch.tensor(ytr, dtype=torch.float32, device=dev)
    Xte_t, yte_t = torch.tensor(Xte, dtype=torch.float32, device=dev), torch.tensor(yte, dtype=torch.float32, device=dev)
    score = GlmScore("logistic", Xtr.shape[1], w_col=1, alpha_col=0, n_train=len(Xtr))
    sampler = SteinSampler(args.particles, None, AdamGradientDescent(learning_rate=1e-1), score=score,
                           model_vars={"model/w:0": [Xtr.shape[1], 1], "model/log_alpha:0": []})
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(args.iters):
        idx = torch.randint(0, len(Xtr), (args.batch,), device=dev, generator=gen)
        sampler.train_on_batch({"X": Xtr_t[idx], "y": ytr_t[idx]})

    n = args.particles
    w, info = sampler.importance_weights({"X": Xtr_t, "y": ytr_t}, iters=args.fw_iters)
    print("%d particles after %d SVGD steps; %d Frank-Wolfe steps" % (n, args.iters, args.fw_iters or 4 * n))
    print("  KSD^2 (IMQ, median bandwidth): uniform %.4e   weighted %.4e   gap %.3e (weighted - optimum <= 2 gap)" %
          (info["ksd2_uniform"], info["ksd2"], info["gap"]))
    print("  effective sample size 1 / sum w^2 = %.1f of %d; %d particles carry weight" %
          (1.0 / float((w * w).sum()), n, int((w > 0).sum())))
    logits = Xte_t.double() @ sampler.theta_matrix[:, 1:].double().T                      # [test, n]
    uniform = torch.full_like(w, 1.0 / n)
    for name, ww in (("unweighted", uniform), ("weighted", w)):
        mean_logit = logits @ ww
        acc = float(((mean_logit > 0).double() == yte_t.double()).double().mean())
        log_l = yte_t.double()[:, None] * logits - torch.nn.functional.softplus(logits)   # [test, n]
        lpd = float(torch.logsumexp(log_l + ww.clamp_min(1e-300).log()[None, :], 1).mean())
        print("  %-10s ensemble: held-out accuracy %.4f, mean log predictive density %.4f" % (name, acc, lpd))


if __name__ == "__main__":
    main()
