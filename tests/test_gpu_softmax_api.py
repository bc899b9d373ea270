"""GPU: softmax regression through the public API -- SoftmaxScore inside SteinSampler.train_on_batch on a 3-class toy set (the
score it feeds is the C ABI's, bit for bit), function_posterior(SoftmaxPredict), predictive_classes, the ValueErrors that send
a SoftmaxPredict away from the scalar-output methods, and the label dtypes."""
import numpy as np
import pytest
import torch

from stein_amd import _lib
from stein_amd.optimizers import AdagradGradientDescent
from stein_amd.predict import GlmPredict, SoftmaxPredict
from stein_amd.samplers import SteinSampler
from stein_amd.scores import SoftmaxScore

pytestmark = pytest.mark.gpu
N, F, C, B = 33, 3, 3, 60


def _toy(cuda):
    rng = np.random.default_rng(4)
    centres = np.array([[2.0, 0.0], [-1.0, 1.7], [-1.0, -1.7]])
    y = rng.integers(0, C, size=B)
    X = np.concatenate([centres[y] + 0.6 * rng.normal(size=(B, 2)), np.ones((B, 1))], axis=1)      # a column of ones: the bias
    return torch.tensor(X, dtype=torch.float32, device=cuda), torch.tensor(y, device=cuda)          # int64 labels


def _sampler(cuda):
    rng = np.random.default_rng(5)
    d = F * C + 1
    theta = (0.1 * rng.normal(size=(N, d))).astype(np.float32)
    score = SoftmaxScore(F, C, w_col=0, alpha_col=F * C, n_train=10 * B)
    return SteinSampler(N, None, AdagradGradientDescent(learning_rate=5e-2), theta=theta, score=score, device=cuda), score


def test_training_predictions_and_the_refusals(cuda):
    X, y = _toy(cuda)
    s, score = _sampler(cuda)
    feed = {"X": X, "y": y}
    assert y.dtype == torch.int64
    # the score the sampler feeds is the C ABI's, bit for bit
    th = s.theta_matrix.clone()
    fed = s.score_matrix(feed)
    raw = torch.full_like(th, float("nan"))
    _lib.call("stein_score_softmax", th.data_ptr(), N, th.shape[1], 0, F, C, F * C, X.data_ptr(), y.to(torch.int32).data_ptr(), B,
              10.0, 1.0, 0.01, raw.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(raw).all()) and torch.equal(fed.view(torch.int32), raw.view(torch.int32))
    for _ in range(5):
        s.train_on_batch(feed)
    assert bool(torch.isfinite(s.theta_matrix).all()) and not torch.equal(s.theta_matrix, th)
    # function_posterior: [n, batch, C] from the producer, flattened per particle by the sampler as for any callable
    prod = SoftmaxPredict(F, C)
    out = prod(s.theta_matrix, {"X": X})
    assert out.shape == (N, B, C) and out.dtype == torch.float32
    fp = s.function_posterior(prod, {"X": X})
    assert fp.shape == (N, B * C) and np.array_equal(fp.reshape(N, B, C), out.cpu().numpy())
    assert np.allclose(fp.reshape(N, B, C).sum(-1), 1.0, atol=1e-5)
    # predictive_classes: keys, shapes, dtypes and what they are
    pc = s.predictive_classes(prod, feed)
    assert set(pc) == {"prob", "label", "entropy", "mutual_information", "lpd"}
    assert pc["prob"].shape == (B, C) and pc["prob"].dtype == np.float32 and pc["label"].shape == (B,) and pc["label"].dtype == np.int32
    for k in ("entropy", "mutual_information", "lpd"):
        assert pc[k].shape == (B,) and pc[k].dtype == np.float32 and np.isfinite(pc[k]).all(), k
    assert (pc["mutual_information"] >= 0).all()
    p64 = pc["prob"].astype(np.float64)
    assert np.allclose(pc["entropy"], -(p64 * np.log(p64)).sum(-1), rtol=1e-6, atol=1e-7)
    assert np.array_equal(pc["label"], pc["prob"].argmax(-1))
    assert np.allclose(pc["prob"], fp.reshape(N, B, C).mean(0), atol=1e-6)
    assert np.allclose(pc["lpd"], np.log(fp.reshape(N, B, C)[:, np.arange(B), y.cpu().numpy()].astype(np.float64).mean(0)), atol=1e-5)
    assert set(s.predictive_classes(prod, {"X": X})) == {"prob", "label", "entropy", "mutual_information"}
    # the scalar-output methods refuse a SoftmaxPredict and name predictive_classes
    for call in (lambda: s.posterior_predictive(prod, feed), lambda: s.posterior_predictive(prod, feed, weights=np.ones(N)),
                 lambda: s.posterior_predictive(prod, feed, quantiles=(0.5,)), lambda: s.predictive_quantiles(prod, feed, (0.5,)),
                 lambda: s.predictive_quantiles(prod, feed, (0.5,), weights=np.ones(N)), lambda: s.predictive_cdf(prod, feed),
                 lambda: s.predictive_interval(prod, feed, (0.1, 0.9)), lambda: prod.order_statistics(s.theta_matrix, feed, [0])):
        with pytest.raises(ValueError, match="predictive_classes"):
            call()
    with pytest.raises(ValueError, match="posterior_predictive"):
        s.predictive_classes(GlmPredict("logistic", F), feed)


def test_label_dtypes(cuda):
    X, y = _toy(cuda)
    s, score = _sampler(cuda)
    th = s.theta_matrix
    base = score(th, {"X": X, "y": y})
    for dt in (torch.int32, torch.int16, torch.uint8):
        assert torch.equal(score(th, {"X": X, "y": y.to(dt)}), base), dt
    assert torch.equal(score(th, {"X": X, "y": y.cpu()}), base)                   # moved to the device
    prod = SoftmaxPredict(F, C)
    lpd = prod.summary(th, {"X": X, "y": y})["lpd"]
    assert torch.equal(prod.summary(th, {"X": X, "y": y.to(torch.int16)})["lpd"], lpd)
    for bad in (y.float(), y.double(), y > 0):
        with pytest.raises(ValueError, match="integer"):
            score(th, {"X": X, "y": bad})
        with pytest.raises(ValueError, match="integer"):
            prod.summary(th, {"X": X, "y": bad})
    with pytest.raises(ValueError):
        score(th, {"X": X, "y": y[:-1]})
