"""Is the sampler calibrated?  The predictive distribution of y, observation noise included, on held-out rows.

    python examples/predictive_calibration/main.py [--particles 64] [--iters 1500] [--train 200] [--test 400]

trains the network of examples/regression_neural_network (one hidden layer, per-particle noise precision log_gamma, HIP score
producer) on synthetic data and asks of held-out rows what a regression user asks when validating a sampler:

    PIT histogram     sampler.predictive_cdf(producer, held_out): F_b(y_b), the probability integral transform of the
                      mixture over the particles of N(z_pb, 1 / gamma_p); flat for a calibrated sampler
    coverage of y     how many held-out y_b fall inside the 90 % interval of sampler.predictive_interval (the quantiles of that
                      mixture), beside the 90 % credible band of f from sampler.predictive_quantiles, which leaves the noise out
                      and under-covers by construction
    the same under    weights=sampler.importance_weights(...)

The [particles, rows] matrix is never formed.  It prints only: no thresholds.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from stein_amd.optimizers import AdamGradientDescent  # noqa: E402
from stein_amd.predict import BnnPredict  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import BnnScore  # noqa: E402

QS = (0.05, 0.95)


def make_data(rng, count, noise=0.3):
    X = rng.uniform(size=(count, 1))
    return X, rng.normal(np.cos(10 * X) * (5 * X), noise)[:, 0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--test", type=int, default=400)
    ap.add_argument("--fw-iters", type=int, default=None, help="Frank-Wolfe steps of the weights (default: 4 x particles)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    dev = "cuda"
    rng = np.random.default_rng(0)
    (Xtr, ytr), (Xte, yte) = make_data(rng, args.train), make_data(rng, args.test)
    as_feed = lambda X, y: {"X": torch.tensor(X, dtype=torch.float32, device=dev),   # noqa: E731
                            "y": torch.tensor(y, dtype=torch.float32, device=dev)}
    train, held_out = as_feed(Xtr, ytr), as_feed(Xte, yte)
    H, n = args.hidden, args.particles
    shapes = {"model/w_1:0": [1, H], "model/b_1:0": [H], "model/w_2:0": [H, 1], "model/b_2:0": [],
              "model/log_lambda:0": [], "model/log_gamma:0": []}
    scale = {"model/w_1:0": 10.0, "model/b_1:0": 1.0, "model/w_2:0": 1.0, "model/b_2:0": 1.0,
             "model/log_lambda:0": 0.0, "model/log_gamma:0": 0.0}
    init = {k: rng.normal(size=[n] + s) * scale[k] for k, s in shapes.items()}
    sampler = SteinSampler(n, None, AdamGradientDescent(learning_rate=5e-2, decay=0.999), theta=init, model_vars=shapes)
    cols = BnnScore.columns(sampler._access)
    sampler.score = BnnScore(1, H, cols, n_train=args.train)
    producer = BnnPredict(1, H, cols)
    for _ in range(args.iters):
        sampler.train_on_batch(train)
    w, info = sampler.importance_weights(train, iters=args.fw_iters)

    report = {}
    for name, weights in (("unweighted", None), ("importance weights", w)):
        pit = sampler.predictive_cdf(producer, held_out, weights=weights)
        y_band = sampler.predictive_interval(producer, held_out, QS, weights=weights)
        f_band = sampler.predictive_quantiles(producer, held_out, QS, weights=weights)
        hist = np.histogram(pit, bins=10, range=(0.0, 1.0))[0] / len(pit)
        cover_y = float(np.mean((yte >= y_band[0]) & (yte <= y_band[1])))
        cover_f = float(np.mean((yte >= f_band[0]) & (yte <= f_band[1])))
        report[name] = dict(pit=pit, hist=hist, cover_y=cover_y, cover_f=cover_f, y_band=y_band, f_band=f_band)
        print("%s (%d particles, %d held-out rows%s)" % (name, n, args.test,
              "" if weights is None else "; KSD^2 uniform %.3e, weighted %.3e" % (info["ksd2_uniform"], info["ksd2"])))
        print("  PIT histogram, ten bins (0.10 each when calibrated): " + " ".join("%.2f" % h for h in hist))
        print("  90 %% interval of y : covers %.3f of the held-out y, mean width %.3f" % (cover_y, float(np.mean(y_band[1] - y_band[0]))))
        print("  90 %% band of f     : covers %.3f of the held-out y, mean width %.3f  (no noise: under-covers by construction)"
              % (cover_f, float(np.mean(f_band[1] - f_band[0]))))
    return report


if __name__ == "__main__":
    main()
