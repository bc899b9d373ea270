"""The network classifier of examples/network_classifier continued: after the run, shrink or correct the particle set and read
the held-out class summaries under per-particle weights, with no [n, batch, C] tensor and without gathering particles.

    python examples/weighted_classes/main.py [--particles 100] [--iters 1000] [--keep 16]

Four ensembles are compared on the held-out points, by accuracy and by the mean log predictive density:
  full                 all n particles, every one counting alike            sampler.predictive_classes(producer, feed)
  theta[:keep]         the first `keep` particles: what a naive cut gives   (a sampler-free producer.summary on the slice)
  thinning counts      sampler.thin(keep): the greedy Stein picks, with repeats, as the integer weights
                       torch.bincount(idx, minlength=n)                     sampler.predictive_classes(..., weights=counts)
  importance weights   sampler.importance_weights(): Frank-Wolfe weights on the simplex that lower the Stein discrepancy of
                       the weighted particles; the particles do not move    sampler.predictive_classes(..., weights=w)
The weighted calls (stein_predict_bnn_class_weighted) do not compute particles of weight zero: the thinned readout costs about
what its distinct particles cost.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from stein_amd.optimizers import AdagradGradientDescent  # noqa: E402
from stein_amd.predict import BnnClassPredict  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import BnnClassScore  # noqa: E402

N_IN, HIDDEN, C, BATCH = 3, 20, 3, 100
GAMMA_RATE = 0.01
W1, B1, W2, B2, LOG_LAMBDA = BnnClassScore.NAMES


def make_data(rng, n_points):
    """class k: the arc r = 0.4 + 0.9 s at the angle s + 2 pi k / 3, s in [0, 2.5], with a little noise"""
    y = rng.integers(0, C, size=n_points)
    s = rng.uniform(0.0, 2.5, size=n_points)
    angle, r = s + 2.0 * math.pi * y / C, 0.4 + 0.9 * s
    X = np.stack([r * np.cos(angle), r * np.sin(angle)], axis=1) + 0.06 * rng.normal(size=(n_points, 2))
    return np.concatenate([X, np.ones((n_points, 1))], axis=1).astype(np.float32), y.astype(np.int64)


def make_log_posterior(n_train):
    """the model's log posterior, as examples/network_classifier writes it (the HIP score producer is its gradient)"""
    def log_posterior(theta, feed):
        w1, b1, w2, b2, log_lambda = theta[W1], theta[B1], theta[W2], theta[B2], theta[LOG_LAMBDA]
        hid = torch.relu(torch.einsum("bf,nfh->nbh", feed["X"], w1) + b1[:, None, :])
        logp = torch.log_softmax(torch.einsum("nbh,nhc->nbc", hid, w2) + b2[:, None, :], dim=-1)
        lik = logp[:, torch.arange(feed["X"].shape[0], device=w1.device), feed["y"]].sum(-1)
        lam = log_lambda.exp()
        every = torch.cat([w1.reshape(w1.shape[0], -1), b1, w2.reshape(w2.shape[0], -1), b2], dim=1)
        prior = (0.5 * log_lambda[:, None] - 0.5 * lam[:, None] * every ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
        prior = prior + math.log(GAMMA_RATE) - GAMMA_RATE * lam      # Gamma(1, rate) density at lambda, no Jacobian
        return lik * n_train / feed["X"].shape[0] + prior
    return log_posterior


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--keep", type=int, default=16, help="particles the thinned set keeps (with repeats)")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n_train = 2000
    X, y = make_data(rng, n_train + 500)
    dev = "cuda"
    Xtr, ytr = torch.tensor(X[:n_train], device=dev), torch.tensor(y[:n_train], device=dev)
    held_out = {"X": torch.tensor(X[n_train:], device=dev), "y": torch.tensor(y[n_train:], device=dev)}
    shapes = {W1: [N_IN, HIDDEN], B1: [HIDDEN], W2: [HIDDEN, C], B2: [C], LOG_LAMBDA: []}
    n = args.particles
    init = {W1: rng.normal(size=(n, N_IN, HIDDEN)), B1: rng.normal(size=(n, HIDDEN)),
            W2: rng.normal(size=(n, HIDDEN, C)) / math.sqrt(HIDDEN), B2: 0.1 * rng.normal(size=(n, C)), LOG_LAMBDA: 0.1 * rng.normal(size=n)}
    sampler = SteinSampler(n, make_log_posterior(n_train), AdagradGradientDescent(learning_rate=5e-2), theta=init, model_vars=shapes)
    cols = BnnClassScore.columns(sampler._access)
    sampler.score = BnnClassScore(N_IN, HIDDEN, C, cols, n_train=n_train, gamma_rate=GAMMA_RATE)
    predictive = BnnClassPredict(N_IN, HIDDEN, C, cols)
    order = torch.randperm(n_train, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    for i in range(args.iters):
        at = (i * BATCH) % n_train
        idx = order[at:at + BATCH]
        sampler.train_on_batch({"X": Xtr[idx].contiguous(), "y": ytr[idx].contiguous()})

    # the scores that thinning and the importance weights go by: those of the whole training set
    train = {"X": Xtr, "y": ytr}
    picks = sampler.thin(args.keep, train)
    counts = torch.bincount(picks, minlength=n)
    w, info = sampler.importance_weights(train)

    def show(name, out, extra=""):
        print("%-20s held-out accuracy %.3f, mean log predictive density %.4f%s"
              % (name, float((out["label"] == y[n_train:]).mean()), float(out["lpd"].mean()), extra))

    show("full (%d)" % n, sampler.predictive_classes(predictive, held_out))
    first = predictive.summary(sampler.theta_matrix[:args.keep].contiguous(), held_out)
    show("theta[:%d]" % args.keep, {k: v.cpu().numpy() for k, v in first.items()})
    out = sampler.predictive_classes(predictive, held_out, weights=counts)
    show("thinning counts", out, "   (%d distinct particles, ess %.1f)" % (int((counts > 0).sum()), out["ess"]))
    out = sampler.predictive_classes(predictive, held_out, weights=w)
    show("importance weights", out, "   (ess %.1f; KSD^2 %.3e against %.3e under uniform weights)"
         % (out["ess"], float(info["ksd2"]), float(info["ksd2_uniform"])))


if __name__ == "__main__":
    main()
