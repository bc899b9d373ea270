"""GPU: the network classifier through the public API -- BnnClassScore inside SteinSampler on a 3-class toy set no linear model
separates (its score against score_matrix's autograd of the same log posterior in fp64, inside the reference's allowance;
twenty train_on_batch steps), function_posterior(BnnClassPredict), predictive_classes, the ValueErrors that send a
BnnClassPredict away from the scalar-output methods, and the label dtypes."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.optimizers import AdagradGradientDescent
from stein_amd.predict import BnnClassPredict, GlmPredict
from stein_amd.samplers import SteinSampler
from stein_amd.scores import BnnClassScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_ref as ncr  # noqa: E402

pytestmark = pytest.mark.gpu
N, F, H, C, B = 33, 3, 10, 3, 60
N_TRAIN, RATE = 600, 0.01
SHAPES = {"model/w_1:0": [F, H], "model/b_1:0": [H], "model/w_2:0": [H, C], "model/b_2:0": [C], "model/log_lambda:0": []}


def _toy(cuda):
    """three interleaved arcs and a column of ones"""
    rng = np.random.default_rng(4)
    y = rng.integers(0, C, size=B)
    t = rng.uniform(0.0, 2.0, size=B) + 2.0 * math.pi * y / C
    r = 0.5 + 0.8 * (t - 2.0 * math.pi * y / C)
    X = np.stack([r * np.cos(t), r * np.sin(t), np.ones(B)], axis=1) + 0.05 * rng.normal(size=(B, 3)) * [1, 1, 0]
    return torch.tensor(X, dtype=torch.float32, device=cuda), torch.tensor(y, device=cuda)          # int64 labels


def _log_posterior(theta, feed):
    w1, b1, w2, b2, ll = (theta[k] for k in BnnClassScore.NAMES)
    X = feed["X"].to(w1.dtype)
    hid = torch.relu(torch.einsum("bf,nfh->nbh", X, w1) + b1[:, None, :])
    logp = torch.log_softmax(torch.einsum("nbh,nhc->nbc", hid, w2) + b2[:, None, :], dim=-1)
    lik = logp[:, torch.arange(X.shape[0], device=X.device), feed["y"].long()].sum(-1)
    lam = ll.exp()
    every = torch.cat([w1.reshape(w1.shape[0], -1), b1, w2.reshape(w2.shape[0], -1), b2], dim=1)
    prior = (0.5 * ll[:, None] - 0.5 * lam[:, None] * every ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
    prior = prior + math.log(RATE) - RATE * lam                    # Gamma(1, rate) density at lambda, no Jacobian
    return lik * (N_TRAIN / X.shape[0]) + prior


def _sampler(cuda, dtype=torch.float32):
    rng = np.random.default_rng(5)
    init = {k: (0.5 * rng.normal(size=[N] + v)).astype(np.float32).astype(np.float64) for k, v in sorted(SHAPES.items())}
    s = SteinSampler(N, _log_posterior, AdagradGradientDescent(learning_rate=5e-2), theta=init, model_vars=SHAPES, device=cuda,
                     dtype=dtype)
    cols = BnnClassScore.columns(s._access)
    return s, cols


def test_training_predictions_and_the_refusals(cuda):
    X, y = _toy(cuda)
    feed = {"X": X, "y": y}
    s, cols = _sampler(cuda)
    assert s.n_params == F * H + H + H * C + C + 1 and None not in cols
    # the device score against autograd of the same log posterior, taken in fp64 from the same particles
    s64, cols64 = _sampler(cuda, torch.float64)
    assert cols64 == cols and torch.equal(s64.theta_matrix.float(), s.theta_matrix)
    auto = s64.score_matrix(feed)
    s.score = BnnClassScore(F, H, C, cols, n_train=N_TRAIN, gamma_rate=RATE)
    dev = s.score_matrix(feed)
    torch.cuda.synchronize()
    ref, allow, share = ncr.score(s.theta_matrix.double(), F, H, C, list(cols), X.double(), y, N_TRAIN / B, 1.0, RATE)
    assert share <= 0.02
    # the reference is that gradient (score_matrix hands the fp64 gradient back rounded to fp32: half an ulp)
    assert bool(((ref - auto.double()).abs() <= ncr.U * ref.abs() + 1e-9 * ref.abs().max()).all())
    err = (dev.double() - auto.double()).abs()
    print("device score against fp64 autograd: max |err| / allowance = %.3f" % float((err / allow).max()))
    assert bool((err <= allow).all())
    th = s.theta_matrix.clone()
    for _ in range(20):
        s.train_on_batch(feed)
    assert bool(torch.isfinite(s.theta_matrix).all()) and not torch.equal(s.theta_matrix, th)
    # function_posterior: [n, batch, C] from the producer, flattened per particle by the sampler as for any callable
    prod = BnnClassPredict(F, H, C, cols)
    out = prod(s.theta_matrix, {"X": X})
    assert out.shape == (N, B, C) and out.dtype == torch.float32
    fp = s.function_posterior(prod, {"X": X})
    assert fp.shape == (N, B * C) and np.array_equal(fp.reshape(N, B, C), out.cpu().numpy())
    # predictive_classes: the documented keys, shapes and dtypes; prob sums to 1 within its allowance
    pc = s.predictive_classes(prod, feed)
    assert set(pc) == {"prob", "label", "entropy", "mutual_information", "lpd"}
    assert pc["prob"].shape == (B, C) and pc["prob"].dtype == np.float32 and pc["label"].shape == (B,) and pc["label"].dtype == np.int32
    for k in ("entropy", "mutual_information", "lpd"):
        assert pc[k].shape == (B,) and pc[k].dtype == np.float32 and np.isfinite(pc[k]).all(), k
    assert (pc["mutual_information"] >= 0).all()
    a_prob = ncr.predict(s.theta_matrix.double(), F, H, C, list(cols), X.double(), y, per=N)["prob"][1].cpu().numpy()
    assert (np.abs(pc["prob"].astype(np.float64).sum(-1) - 1.0) <= a_prob.sum(-1)).all()
    assert np.array_equal(pc["label"], pc["prob"].argmax(-1))
    assert set(s.predictive_classes(prod, {"X": X})) == {"prob", "label", "entropy", "mutual_information"}
    # the scalar-output methods refuse the producer and name predictive_classes
    for call in (lambda: s.posterior_predictive(prod, feed), lambda: s.posterior_predictive(prod, feed, weights=np.ones(N)),
                 lambda: s.posterior_predictive(prod, feed, quantiles=(0.5,)), lambda: s.predictive_quantiles(prod, feed, (0.5,)),
                 lambda: s.predictive_quantiles(prod, feed, (0.5,), weights=np.ones(N)), lambda: s.predictive_cdf(prod, feed),
                 lambda: s.predictive_interval(prod, feed, (0.1, 0.9)), lambda: prod.order_statistics(s.theta_matrix, feed, [0]),
                 lambda: prod.y_quantiles(s.theta_matrix, feed, (0.5,)), lambda: prod.y_cdf(s.theta_matrix, feed, None)):
        with pytest.raises(ValueError, match="predictive_classes"):
            call()
    with pytest.raises(ValueError, match="posterior_predictive"):
        s.predictive_classes(GlmPredict("logistic", F), feed)


def test_label_dtypes(cuda):
    X, y = _toy(cuda)
    s, cols = _sampler(cuda)
    score = BnnClassScore(F, H, C, cols, n_train=N_TRAIN, gamma_rate=RATE)
    th = s.theta_matrix
    base = score(th, {"X": X, "y": y})
    for dt in (torch.int32, torch.int16, torch.uint8):
        assert torch.equal(score(th, {"X": X, "y": y.to(dt)}), base), dt
    assert torch.equal(score(th, {"X": X, "y": y.cpu()}), base)                   # moved to the device
    prod = BnnClassPredict(F, H, C, cols)
    lpd = prod.summary(th, {"X": X, "y": y})["lpd"]
    assert torch.equal(prod.summary(th, {"X": X, "y": y.to(torch.int16)})["lpd"], lpd)
    for bad in (y.float(), y.double(), y > 0):
        with pytest.raises(ValueError, match="integer"):
            score(th, {"X": X, "y": bad})
        with pytest.raises(ValueError, match="integer"):
            prod.summary(th, {"X": X, "y": bad})
    with pytest.raises(ValueError):
        score(th, {"X": X, "y": y[:-1]})
