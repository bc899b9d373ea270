"""GPU: the weighted class summaries through the public API -- SoftmaxPredict / BnnClassPredict.weighted_summary and
SteinSampler.predictive_classes(producer, feed, weights=) -- with float64 importance weights from sampler.importance_weights
and int64 thinning counts from torch.bincount(sampler.thin(m), minlength=n), passed as NumPy, as a CPU tensor and as a device
tensor.  Counts agree with the unweighted summary of the gathered, repeated particles theta[idx] inside the sum of both
calls' allowances; a wrong length or a complex dtype raises; without weights predictive_classes returns what it did."""
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.optimizers import AdagradGradientDescent
from stein_amd.predict import BnnClassPredict, SoftmaxPredict
from stein_amd.samplers import SteinSampler
from stein_amd.scores import BnnClassScore, SoftmaxScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_weighted_ref as cwr  # noqa: E402
import netclass_ref as ncr  # noqa: E402
import predict_cases as pc  # noqa: E402
import softmax_ref as smr  # noqa: E402

pytestmark = pytest.mark.gpu
N, F, H, C, B, M = 48, 3, 20, 3, 60, 12
KEYS = ("prob", "label", "ent", "lpd")


def _toy(cuda):
    rng = np.random.default_rng(4)
    centres = np.array([[2.0, 0.0], [-1.0, 1.7], [-1.0, -1.7]])
    y = rng.integers(0, C, size=B)
    X = np.concatenate([centres[y] + 0.6 * rng.normal(size=(B, 2)), np.ones((B, 1))], axis=1)      # a column of ones: the bias
    return torch.tensor(X, dtype=torch.float32, device=cuda), torch.tensor(y, device=cuda)          # int64 labels


def _setup(model, cuda):
    """-> (sampler after a few steps, producer, logits(theta fp64, X fp64) -> (z, dz))"""
    rng = np.random.default_rng(5)
    opt = AdagradGradientDescent(learning_rate=5e-2)
    if model == "softmax":
        d = F * C + 1
        theta = (0.1 * rng.normal(size=(N, d))).astype(np.float32)
        s = SteinSampler(N, None, opt, theta=theta, score=SoftmaxScore(F, C, w_col=0, alpha_col=F * C, n_train=10 * B), device=cuda)
        return s, SoftmaxPredict(F, C), lambda th, X: cwr.softmax_logits(th, 0, F, C, X)
    cols = [0, F * H, F * H + H, F * H + H + H * C, F * H + H + H * C + C]
    theta = (0.5 * rng.normal(size=(N, cols[4] + 1))).astype(np.float32)
    s = SteinSampler(N, None, opt, theta=theta, score=BnnClassScore(F, H, C, cols, n_train=10 * B), device=cuda)
    return s, BnnClassPredict(F, H, C, cols[:4]), lambda th, X: cwr.netclass_logits(th, F, H, C, cols, X)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("model", ("softmax", "netclass"))
def test_importance_weights_and_thinning_counts_through_both_surfaces(cuda, model):
    X, y = _toy(cuda)
    feed = {"X": X, "y": y}
    s, prod, logits = _setup(model, cuda)
    for _ in range(5):
        s.train_on_batch(feed)
    th = s.theta_matrix
    w, _ = s.importance_weights(feed)
    idx = s.thin(M, feed)
    counts = torch.bincount(idx, minlength=N)
    assert w.dtype == torch.float64 and w.is_cuda and counts.dtype == torch.int64 and int(counts.sum()) == M
    z, dz = logits(th.double(), X.double())
    per = pc.plan(N, B)[2]
    for weights in (w, counts):
        dev = prod.weighted_summary(th, feed, weights)
        torch.cuda.synchronize()
        assert set(dev) == set(KEYS) | {"ess"} and all(v.is_cuda for v in dev.values())
        assert dev["label"].dtype == torch.int32 and dev["ess"].dtype == torch.float64 and dev["ess"].shape == (1,)
        assert set(prod.weighted_summary(th, {"X": X}, weights)) == {"prob", "label", "ent", "ess"}
        ref = cwr.summaries(z, dz, y, weights.double(), per)
        for k in ("prob", "ent", "lpd"):
            assert bool(((dev[k].double() - ref[k][0]).abs() <= ref[k][1]).all()), k
        assert abs(float(dev["ess"]) - float(ref["ess"][0])) <= float(ref["ess"][1])
        assert torch.equal(dev["label"].long(), dev["prob"].argmax(-1))
        # NumPy, a CPU tensor and a device tensor are one call
        for form in (weights.cpu().numpy(), weights.cpu(), weights):
            again = prod.weighted_summary(th, feed, form)
            for k in KEYS:
                assert _same(again[k], dev[k]), k
            assert float(again["ess"]) == float(dev["ess"])
            pcw = s.predictive_classes(prod, feed, weights=form)
            assert set(pcw) == {"prob", "label", "entropy", "mutual_information", "lpd", "ess"} and isinstance(pcw["ess"], float)
            assert np.array_equal(pcw["prob"], dev["prob"].cpu().numpy()) and np.array_equal(pcw["label"], dev["label"].cpu().numpy())
            assert np.array_equal(pcw["lpd"], dev["lpd"].cpu().numpy()) and pcw["ess"] == float(dev["ess"])
            p64 = pcw["prob"].astype(np.float64)
            assert np.allclose(pcw["entropy"], -(p64 * np.log(np.where(p64 > 0, p64, 1.0))).sum(-1), rtol=1e-6, atol=1e-7)
            assert np.array_equal(pcw["mutual_information"], np.maximum(pcw["entropy"] - dev["ent"].cpu().numpy(), np.float32(0)))
        assert set(s.predictive_classes(prod, {"X": X}, weights=weights)) == {"prob", "label", "entropy", "mutual_information", "ess"}
    # an integer dtype is taken as counts: the same call as their float64 copy
    as_int, as_f64 = prod.weighted_summary(th, feed, counts), prod.weighted_summary(th, feed, counts.double())
    assert all(_same(as_int[k], as_f64[k]) for k in KEYS)
    # counts against the unweighted summary of the gathered, repeated particles: inside the sum of both allowances
    gathered = th[idx].contiguous()
    plain = prod.summary(gathered, feed)
    zg, dzg = logits(gathered.double(), X.double())
    ref_u = (smr if model == "softmax" else ncr).summaries(zg, dzg, y, pc.plan(M, B)[2])
    ref_w = cwr.summaries(z, dz, y, counts.double(), per)
    assert 1.0 <= float(as_int["ess"]) <= M
    for k in ("prob", "ent", "lpd"):
        assert bool(((ref_u[k][0] - ref_w[k][0]).abs() <= 1e-12).all()), k      # the two references are one quantity
        assert bool(((as_int[k].double() - plain[k].double()).abs() <= ref_u[k][1] + ref_w[k][1]).all()), k
    # what is refused
    for bad in (np.ones(N - 1), torch.ones(N + 1), torch.ones(N, 1), torch.ones(N, dtype=torch.complex64), torch.ones(N, dtype=torch.bool)):
        with pytest.raises(ValueError, match="weights"):
            prod.weighted_summary(th, feed, bad)
        with pytest.raises(ValueError, match="weights"):
            s.predictive_classes(prod, feed, weights=bad)
    # without weights: exactly what it returned before
    pcu = s.predictive_classes(prod, feed)
    assert set(pcu) == {"prob", "label", "entropy", "mutual_information", "lpd"}
    assert set(s.predictive_classes(prod, {"X": X})) == {"prob", "label", "entropy", "mutual_information"}
    assert np.array_equal(pcu["prob"], prod.summary(th, feed)["prob"].cpu().numpy())
