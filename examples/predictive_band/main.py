"""Credible band of the network example: the ensemble median and the 90 % band per grid point, next to mean +- 1.645 sqrt(var).

    python examples/predictive_band/main.py [--particles 200] [--iters 1500] [--grid 200]

trains the sampler of examples/regression_neural_network (one hidden layer of 100 ReLU units on 20 synthetic points, HIP
score producer) and reads the ensemble out on the reference example's 200-point grid over [0, 1.5] -- the last third of it
lies outside the data -- with ONE call,

    sampler.posterior_predictive(predictive, grid, quantiles=(0.05, 0.5, 0.95))

which gives the mean and the variance of the network outputs over the particles and their exact 5 %, 50 % and 95 %
quantiles per grid point (order statistics found by a radix select that recomputes the forward pass: the [particles, grid]
matrix that the reference's example plots curve by curve is never formed).  It prints the two bands side by side at a few
grid points, and how far the Gaussian band mean +- 1.645 sqrt(var) is from the ensemble's own quantiles, inside the data
and beyond it, as a fraction of the band's width.  It prints only: no thresholds.
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
from stein_amd.predict import BnnPredict  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import BnnScore  # noqa: E402


def network_example():
    spec = importlib.util.spec_from_file_location("network_main", os.path.join(HERE, "..", "regression_neural_network", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--grid", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    net = network_example()
    H, dev = net.H, "cuda"
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(20, 1))
    y = rng.normal(np.cos(10 * X) * (5 * X), 0.1)[:, 0]
    feed = {"X": torch.tensor(X, dtype=torch.float32, device=dev), "y": torch.tensor(y, dtype=torch.float32, device=dev)}
    shapes = {"model/w_1:0": [1, H], "model/b_1:0": [H], "model/w_2:0": [H, 1], "model/b_2:0": [],
              "model/log_lambda:0": [], "model/log_gamma:0": []}
    scale = {"model/w_1:0": 10.0, "model/b_1:0": 1.0, "model/w_2:0": 1.0, "model/b_2:0": 1.0,
             "model/log_lambda:0": 0.0, "model/log_gamma:0": 0.0}        # as the network example starts its particles
    init = {k: rng.normal(size=[args.particles] + s) * scale[k] for k, s in shapes.items()}
    sampler = SteinSampler(args.particles, net.make_log_posterior(len(X), len(X)),
                           AdamGradientDescent(learning_rate=5e-2, decay=0.999), theta=init, model_vars=shapes)
    cols = BnnScore.columns(sampler._access)
    sampler.score = BnnScore(1, H, cols, n_train=len(X))
    for _ in range(args.iters):
        sampler.train_on_batch(feed)

    predictive = BnnPredict(1, H, cols)
    xs = np.linspace(0.0, 1.5, args.grid)
    grid = {"X": torch.tensor(xs[:, None], dtype=torch.float32, device=dev)}
    out = sampler.posterior_predictive(predictive, grid, quantiles=(0.05, 0.5, 0.95))      # one call
    lo, med, hi = out["quantiles"]
    sd = np.sqrt(out["var"])
    g_lo, g_hi = out["mean"] - 1.645 * sd, out["mean"] + 1.645 * sd

    print("%d particles, %d grid points on [0, 1.5]; the data lie in [%.2f, %.2f]" % (args.particles, args.grid, X.min(), X.max()))
    print("      x   |  5 %       median   95 %     (ensemble quantiles) |  mean-1.645sd  mean   mean+1.645sd (Gaussian band)")
    for i in np.linspace(0, args.grid - 1, 11).astype(int):
        print("  %6.3f  | %7.3f  %7.3f  %7.3f                       | %7.3f  %7.3f  %7.3f"
              % (xs[i], lo[i], med[i], hi[i], g_lo[i], out["mean"][i], g_hi[i]))
    inside = xs <= X.max()
    width = np.maximum(hi - lo, 1e-12)
    for name, m in (("inside the data", inside), ("extrapolation", ~inside)):
        if m.any():
            print("%-16s |median - mean| / band width: max %.3f;  Gaussian band ends off by (of the band width): lower max %.3f, "
                  "upper max %.3f" % (name + ":", float((np.abs(med - out["mean"]) / width)[m].max()),
                                      float((np.abs(g_lo - lo) / width)[m].max()), float((np.abs(g_hi - hi) / width)[m].max())))


if __name__ == "__main__":
    main()
