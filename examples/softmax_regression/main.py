"""Bayesian softmax (multi-class logistic) regression with SVGD on synthetic data made here -- four Gaussian classes in three
dimensions and a column of ones for the bias; nothing is read from disk.  W ~ N(0, 1/alpha), alpha ~ Gamma(1, 0.01) sampled
in log space: d = 4 * 4 + 1 = 17 parameters per particle.

    python examples/softmax_regression/main.py [--particles 100] [--iters 1000] [--autograd]

The score comes from the HIP score producer (stein_amd.scores.SoftmaxScore -> stein_score_softmax) and the test readout --
accuracy, the mean log predictive density, and the mutual information between the label and the particle on held-out
points near the training data and far from it -- from sampler.predictive_classes (stein_amd.predict.SoftmaxPredict ->
stein_predict_softmax), with no [n, batch, C] tensor.  --autograd differentiates the same log posterior with torch instead,
for comparison; the readout stays.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from stein_amd.optimizers import AdagradGradientDescent  # noqa: E402
from stein_amd.predict import SoftmaxPredict  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import SoftmaxScore  # noqa: E402

DIM, C, BATCH = 3, 4, 100
F = DIM + 1                      # the features and a column of ones
GAMMA_RATE = 0.01


def make_data(rng, n_points, spread=1.0):
    """four classes with means on a tetrahedron of radius 2.5 and unit covariance; spread scales the points away from the
    origin (spread = 6: far from anything the model saw)"""
    means = 2.5 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / math.sqrt(3)
    y = rng.integers(0, C, size=n_points)
    X = spread * (means[y] + rng.normal(size=(n_points, DIM)))
    return np.concatenate([X, np.ones((n_points, 1))], axis=1).astype(np.float32), y.astype(np.int64)


def make_log_posterior(n_train):
    def log_posterior(theta, feed):
        W, log_alpha = theta["W:0"], theta["log_alpha:0"]        # [n, F, C], [n]
        logp = torch.log_softmax(torch.einsum("bf,nfc->nbc", feed["X"], W), dim=-1)
        lik = logp[:, torch.arange(feed["X"].shape[0], device=W.device), feed["y"]].sum(-1)
        alpha = log_alpha.exp()
        prior = (0.5 * log_alpha[:, None] - 0.5 * alpha[:, None] * W.reshape(W.shape[0], -1) ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
        prior = prior + math.log(GAMMA_RATE) - GAMMA_RATE * alpha      # Gamma(1, rate) density at alpha, no Jacobian
        return lik * n_train / feed["X"].shape[0] + prior
    return log_posterior


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--autograd", action="store_true", help="differentiate log_posterior with torch instead of the HIP score producer")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n_train = 2000
    X, y = make_data(rng, n_train + 500)
    Xfar, _ = make_data(rng, 500, spread=6.0)
    dev = "cuda"
    Xtr, ytr = torch.tensor(X[:n_train], device=dev), torch.tensor(y[:n_train], device=dev)
    near = {"X": torch.tensor(X[n_train:], device=dev), "y": torch.tensor(y[n_train:], device=dev)}
    far = {"X": torch.tensor(Xfar, device=dev)}
    shapes = {"W:0": [F, C], "log_alpha:0": []}                  # packed in sorted order: W at column 0, log alpha behind it
    init = {"W:0": 0.1 * rng.normal(size=(args.particles, F, C)), "log_alpha:0": 0.1 * rng.normal(size=args.particles)}
    sampler = SteinSampler(args.particles, make_log_posterior(n_train), AdagradGradientDescent(learning_rate=5e-2), theta=init,
                           model_vars=shapes)
    w_col, alpha_col = sampler._access["W:0"][0], sampler._access["log_alpha:0"][0]
    assert sampler.n_params == F * C + 1
    if not args.autograd:   # the closed form of the same log posterior's gradient in one HIP launch (stein_amd/scores.py)
        sampler.score = SoftmaxScore(F, C, w_col=w_col, alpha_col=alpha_col, n_train=n_train, gamma_rate=GAMMA_RATE)
    predictive = SoftmaxPredict(F, C, w_col=w_col)

    def readout():
        out, away = sampler.predictive_classes(predictive, near), sampler.predictive_classes(predictive, far)
        return (float((out["label"] == y[n_train:]).mean()), float(out["lpd"].mean()), float(out["mutual_information"].mean()),
                float(away["mutual_information"].mean()))

    order = torch.randperm(n_train, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.iters):
        at = (i * BATCH) % n_train
        idx = order[at:at + BATCH]
        sampler.train_on_batch({"X": Xtr[idx].contiguous(), "y": ytr[idx].contiguous()})
        if i % 250 == 0 or i == args.iters - 1:
            print("iteration %5d: test accuracy %.3f, mean log predictive density %.4f, mutual information near %.4f / far %.4f"
                  % ((i,) + readout()))
    torch.cuda.synchronize()
    print("%d iterations with the %s score: %.2f s (readouts included)" % (args.iters, "autograd" if args.autograd else "HIP", time.perf_counter() - t0))


if __name__ == "__main__":
    main()
