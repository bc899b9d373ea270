"""Weighted posterior predictive of an SVGD run stopped early: Stein importance weights and thinning counts in the summaries.

    python examples/weighted_predictive/main.py [--particles 1024] [--iters 60] [--long-iters 2000] [--thin 128]

runs the sampler of examples/logistic_regression (synthetic data of Covertype's shape, HIP score producer) for a few steps
only, and reads the held-out predictions out four ways through ``sampler.posterior_predictive`` (the HIP predictive
producer; the [particles, test points] matrix is never formed):

    uniform    the plain ensemble, 1/n per particle
    weighted   weights=sampler.importance_weights(...)             (Stein importance weights, float64 on the simplex)
    counts     weights=torch.bincount(sampler.thin(m), minlength=n)  (the thinned multiset as integer weights)
    gathered   the thinned particles theta[idx] gathered into their own [m, d] matrix, then unweighted

and prints, for each, the mean held-out log predictive density and the mean absolute error of the ensemble-mean logit
against a long run of the same sampler, with the effective sample size of the weights.  `counts` and `gathered` describe the
same multiset, so they agree to rounding.  It prints only: no thresholds.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from stein_amd.optimizers import AdamGradientDescent  # noqa: E402
from stein_amd.predict import GlmPredict  # noqa: E402
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
    ap.add_argument("--long-iters", type=int, default=2000, help="SVGD steps of the long run the estimates are compared with")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--thin", type=int, default=128, help="particles Stein thinning picks (with replacement)")
    ap.add_argument("--fw-iters", type=int, default=None, help="Frank-Wolfe steps of the weights (default: 4 x particles)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    dev = "cuda"
    (Xtr, ytr), (Xte, yte) = logistic_example().make_data()
    Xtr_t, ytr_t = torch.tensor(Xtr, dtype=torch.float32, device=dev), torch.tensor(ytr, dtype=torch.float32, device=dev)
    test = {"X": torch.tensor(Xte, dtype=torch.float32, device=dev), "y": torch.tensor(yte, dtype=torch.float32, device=dev)}
    full = {"X": Xtr_t, "y": ytr_t}
    n, feats = args.particles, Xtr.shape[1]
    predictive = GlmPredict("logistic", feats, w_col=1)           # output "link": the logits

    def run(iters):
        torch.manual_seed(0)
        score = GlmScore("logistic", feats, w_col=1, alpha_col=0, n_train=len(Xtr))
        s = SteinSampler(n, None, AdamGradientDescent(learning_rate=1e-1), score=score,
                         model_vars={"model/w:0": [feats, 1], "model/log_alpha:0": []})
        gen = torch.Generator(device=dev).manual_seed(0)
        for _ in range(iters):
            idx = torch.randint(0, len(Xtr), (args.batch,), device=dev, generator=gen)
            s.train_on_batch({"X": Xtr_t[idx], "y": ytr_t[idx]})
        return s

    long_run = run(args.long_iters).posterior_predictive(predictive, test)
    sampler = run(args.iters)
    w, info = sampler.importance_weights(full, iters=args.fw_iters)
    idx = sampler.thin(args.thin, full)
    counts = torch.bincount(idx, minlength=n)

    rows = [("uniform", sampler.posterior_predictive(predictive, test)),
            ("weighted", sampler.posterior_predictive(predictive, test, weights=w)),
            ("counts", sampler.posterior_predictive(predictive, test, weights=counts))]
    mean, var, lpd = predictive.summary(sampler._matrix_f32()[idx].contiguous(), test)
    rows.append(("gathered", {"mean": mean.cpu().numpy(), "var": var.cpu().numpy(), "lpd": lpd.cpu().numpy()}))

    print("%d particles after %d SVGD steps, against %d steps; KSD^2 uniform %.3e, weighted %.3e; %d of %d picks distinct"
          % (n, args.iters, args.long_iters, info["ksd2_uniform"], info["ksd2"], int((counts > 0).sum()), args.thin))
    print("  long run : held-out mean lpd %.4f" % float(np.mean(long_run["lpd"])))
    for name, out in rows:
        ess = "ess %7.1f" % out["ess"] if "ess" in out else "(unweighted over %d particles)" % (n if name == "uniform" else args.thin)
        print("  %-9s: held-out mean lpd %.4f   mean |logit - long run| %.4f   %s"
              % (name, float(np.mean(out["lpd"])), float(np.mean(np.abs(out["mean"] - long_run["mean"]))), ess))


if __name__ == "__main__":
    main()
