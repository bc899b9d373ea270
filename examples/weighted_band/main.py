"""Credible bands of an SVGD run stopped early, under Stein importance weights and of the thinned multiset.

    python examples/weighted_band/main.py [--particles 1024] [--iters 60] [--long-iters 2000] [--thin 128]

runs the sampler of examples/logistic_regression (synthetic data of Covertype's shape, HIP score producer) for a few steps
only, and reads the 90 % band and the median of the held-out class probabilities out three ways through
``sampler.predictive_quantiles`` (the HIP predictive producer; the [particles, test points] matrix is never formed):

    unweighted   the plain ensemble: exact order statistics, NumPy's linear interpolation
    weighted     weights=sampler.importance_weights(...)               (float64 on the simplex)
    counts       weights=torch.bincount(sampler.thin(m), minlength=n)  (the thinned multiset as integer counts)

The two weighted bands follow the inverted weighted distribution function: each value is an output of one particle, the
smallest at which the cumulative weight reaches q -- no interpolation, unlike the unweighted band.  It prints, for each, the
mean width of the band, the mean absolute distance of its median and of its two ends from the band of a long run of the
same sampler, and how often the held-out label's side of 1/2 agrees with the median.  It prints only: no thresholds.
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

QS = (0.05, 0.5, 0.95)


def logistic_example():
    spec = importlib.util.spec_from_file_location("logistic_main", os.path.join(HERE, "..", "logistic_regression", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=60, help="SVGD steps before the run is stopped")
    ap.add_argument("--long-iters", type=int, default=2000, help="SVGD steps of the long run the bands are compared with")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--thin", type=int, default=128, help="particles Stein thinning picks (with replacement)")
    ap.add_argument("--fw-iters", type=int, default=None, help="Frank-Wolfe steps of the weights (default: 4 x particles)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    dev = "cuda"
    (Xtr, ytr), (Xte, yte) = logistic_example().make_data()
    Xtr_t, ytr_t = torch.tensor(Xtr, dtype=torch.float32, device=dev), torch.tensor(ytr, dtype=torch.float32, device=dev)
    test = {"X": torch.tensor(Xte, dtype=torch.float32, device=dev)}
    full = {"X": Xtr_t, "y": ytr_t}
    n, feats = args.particles, Xtr.shape[1]
    predictive = GlmPredict("logistic", feats, w_col=1, output="mean")       # the class probabilities sigmoid(x . w)

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

    long_band = run(args.long_iters).predictive_quantiles(predictive, test, QS)
    sampler = run(args.iters)
    w, info = sampler.importance_weights(full, iters=args.fw_iters)
    counts = torch.bincount(sampler.thin(args.thin, full), minlength=n)

    rows = [("unweighted", sampler.predictive_quantiles(predictive, test, QS)),
            ("weighted", sampler.predictive_quantiles(predictive, test, QS, weights=w)),
            ("counts", sampler.predictive_quantiles(predictive, test, QS, weights=counts))]
    print("%d particles after %d SVGD steps, against %d steps; KSD^2 uniform %.3e, weighted %.3e; %d of %d picks distinct"
          % (n, args.iters, args.long_iters, info["ksd2_uniform"], info["ksd2"], int((counts > 0).sum()), args.thin))
    print("  long run  : mean width of the 90 %% band %.4f" % float(np.mean(long_band[2] - long_band[0])))
    for name, band in rows:
        agree = float(np.mean((band[1] > 0.5) == (np.asarray(yte) > 0.5)))
        print("  %-10s: mean width %.4f   mean |median - long run| %.4f   mean |ends - long run| %.4f   median on the label's side %.3f"
              % (name, float(np.mean(band[2] - band[0])), float(np.mean(np.abs(band[1] - long_band[1]))),
                 float(np.mean(np.abs(band[[0, 2]] - long_band[[0, 2]]))), agree))


if __name__ == "__main__":
    main()
