"""Bayesian neural-network regression on tabular data with SVGD: the benchmark of the method (Liu & Wang 2016) -- one
hidden layer of 50 ReLU units, Gamma(1, 0.1) priors on the weight precision lambda and the noise precision gamma (both
sampled in log space), 20 particles, mini-batches of 100, Adam -- on synthetic data with 13 input features (the width of the
Boston housing set), made here: nothing is read from disk.  d = 13 * 50 + 2 * 50 + 3 = 753 parameters per particle.

    python examples/wide_network/main.py [--particles 20] [--iters 2000] [--autograd]

More than four input features: the score comes from the wide HIP score producer (stein_amd.scores.BnnScore ->
stein_score_bnn_wide) and the test readout -- the RMSE of the ensemble mean and the mean log predictive density -- from the
wide predictive producer (stein_amd.predict.BnnPredict -> stein_predict_bnn_wide) through sampler.posterior_predictive, with
no [n, batch] matrix.  --autograd differentiates the same log posterior with torch instead, for comparison; the readout stays.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from stein_amd.optimizers import AdamGradientDescent  # noqa: E402
from stein_amd.predict import BnnPredict  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import BnnScore  # noqa: E402

F, H, BATCH = 13, 50, 100
GAMMA_A, GAMMA_B = 1.0, 0.1


def make_data(rng, n_points=1000):
    """a smooth nonlinear function of 13 standardised features plus noise of standard deviation 0.1"""
    X = rng.normal(size=(n_points, F))
    a, b = rng.normal(size=F) / math.sqrt(F), rng.normal(size=F) / math.sqrt(F)
    y = np.sin(X @ a * 2.0) + 0.5 * (X @ b) ** 2 - 0.5 + rng.normal(scale=0.1, size=n_points)
    return X.astype(np.float32), y.astype(np.float32)


def predict(theta, X):
    """[n_particles, n_points] network outputs for every particle."""
    w1, b1 = theta["model/w_1:0"], theta["model/b_1:0"]         # [n, F, H], [n, H]
    w2, b2 = theta["model/w_2:0"], theta["model/b_2:0"]         # [n, H, 1], [n]
    hidden = torch.relu(torch.einsum("pf,nfh->nph", X, w1) + b1[:, None, :])
    return torch.einsum("nph,nh->np", hidden, w2[:, :, 0]) + b2[:, None]


def make_log_posterior(n_train, a=GAMMA_A, b=GAMMA_B):
    def normal_logpdf(x, log_prec):
        return 0.5 * log_prec - 0.5 * log_prec.exp() * x ** 2 - 0.5 * math.log(2 * math.pi)

    def gamma_logpdf_of_exp(log_x):   # Gamma(a, b) density evaluated at x = exp(log_x)
        return a * math.log(b) - math.lgamma(a) + (a - 1) * log_x - b * log_x.exp()

    def log_posterior(theta, feed):
        log_lam, log_gam = theta["model/log_lambda:0"], theta["model/log_gamma:0"]   # [n]
        pred = predict(theta, feed["X"])
        log_l = normal_logpdf(pred - feed["y"][None, :], log_gam[:, None]).sum(1)
        prior = gamma_logpdf_of_exp(log_lam) + gamma_logpdf_of_exp(log_gam)
        for name in ("model/w_1:0", "model/b_1:0", "model/w_2:0"):
            v = theta[name].reshape(theta[name].shape[0], -1)
            prior = prior + normal_logpdf(v, log_lam[:, None]).sum(1)
        prior = prior + normal_logpdf(theta["model/b_2:0"], log_lam)
        return (log_l * n_train / feed["X"].shape[0] + prior) / n_train
    return log_posterior


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--autograd", action="store_true", help="differentiate log_posterior with torch instead of the HIP score producer")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    X, y = make_data(rng)
    n_train = 900                                                # train / test split: 900 / 100
    dev = "cuda"
    Xtr, ytr = torch.tensor(X[:n_train], device=dev), torch.tensor(y[:n_train], device=dev)
    test = {"X": torch.tensor(X[n_train:], device=dev), "y": torch.tensor(y[n_train:], device=dev)}
    shapes = {"model/w_1:0": [F, H], "model/b_1:0": [H], "model/w_2:0": [H, 1], "model/b_2:0": [],
              "model/log_lambda:0": [], "model/log_gamma:0": []}
    scale = {"model/w_1:0": 1.0 / math.sqrt(F + 1), "model/b_1:0": 1.0 / math.sqrt(F + 1), "model/w_2:0": 1.0 / math.sqrt(H + 1),
             "model/b_2:0": 1.0 / math.sqrt(H + 1), "model/log_lambda:0": 0.1, "model/log_gamma:0": 0.1}
    init = {k: rng.normal(size=[args.particles] + s) * scale[k] for k, s in shapes.items()}
    sampler = SteinSampler(args.particles, make_log_posterior(n_train), AdamGradientDescent(learning_rate=1e-2, decay=1.0),
                           theta=init, model_vars=shapes)
    assert sampler.n_params == F * H + 2 * H + 3
    cols = BnnScore.columns(sampler._access)
    if not args.autograd:   # closed-form backprop of the same log posterior in one HIP launch (stein_amd/scores.py)
        sampler.score = BnnScore(F, H, cols, n_train=n_train, gamma_a=GAMMA_A, gamma_b=GAMMA_B)
    predictive = BnnPredict(F, H, cols)

    def readout():
        """-> (RMSE of the ensemble mean, mean log predictive density) on the held-out points"""
        out = sampler.posterior_predictive(predictive, test)
        return float(np.sqrt(np.mean((y[n_train:] - out["mean"]) ** 2))), float(np.mean(out["lpd"]))

    order = torch.randperm(n_train, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.iters):
        at = (i * BATCH) % n_train
        idx = order[at:at + BATCH]
        sampler.train_on_batch({"X": Xtr[idx].contiguous(), "y": ytr[idx].contiguous()})
        if i % 250 == 0 or i == args.iters - 1:
            print("iteration %5d: test RMSE %.4f, mean log predictive density %.4f" % ((i,) + readout()))
    torch.cuda.synchronize()
    print("%d iterations with the %s score: %.2f s (readouts included)" % (args.iters, "autograd" if args.autograd else "HIP", time.perf_counter() - t0))


if __name__ == "__main__":
    main()
