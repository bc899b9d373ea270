"""GPU: the Python side of the weighted predictive quantiles -- ``producer.weighted_quantiles`` (stein_amd/predict.py) and
``sampler.predictive_quantiles`` -- against the definition of tests/wquantile_cases.py applied to the producer's OWN pred,
exactly: float weights through the masses rint(w / W 2^31) the library reports, integer weights as counts against
np.repeat; more than eight levels; weights from sampler.thin against the band of the gathered multiset; weights=None is
``producer.quantiles`` to the bit; argument errors are ValueErrors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import quantile_cases as qc  # noqa: E402
import wquantile_cases as wq  # noqa: E402

pytestmark = pytest.mark.gpu
QS = (0.0, 1.0, 0.5, 0.05, 0.95, 0.3337, 0.9, 0.013, 0.25, 0.75, 0.5)       # eleven levels: two calls of the library


def _producer(case, a):
    from stein_amd.predict import BnnPredict, GlmPredict
    if case["model"] == "bnn":
        return BnnPredict(case["n_in"], case["H"], a["cols"], output=case["output"])
    return GlmPredict(case["model"], case["F"], w_col=a["w_col"], output=case["output"])


def _setup(case, dev):
    a = pc.args(case)
    theta = torch.tensor(a["theta"], dtype=torch.float32, device=dev)
    feed = {"X": torch.tensor(a["X"], dtype=torch.float32, device=dev)}
    return a, _producer(case, a), theta, feed


def _by_definition(pred, masses, qs):
    M = int(np.asarray(masses, np.uint64).astype(object).sum())
    targets = [wq.target(q, M) for q in qs]
    return np.stack([wq.by_definition(pred[:, b], masses, targets) for b in range(pred.shape[1])], axis=1)


@pytest.mark.parametrize("case", [qc.CASES[1], qc.CASES[4]], ids=lambda c: c["name"])     # a GLM and a network producer
def test_weighted_quantiles_against_the_definition_on_the_own_pred(cuda, case):
    a, prod, theta, feed = _setup(case, cuda)
    n = case["n"]
    pred = prod(theta, feed).cpu().numpy()
    rng = np.random.default_rng(5)
    # float weights, as a NumPy array and as a float32 device tensor: the masses the producer keeps are the library's
    w = rng.exponential(size=n)
    w[::6] = 0.0
    for weights in (w, torch.tensor(w, dtype=torch.float32, device=cuda)):
        got = prod.weighted_quantiles(theta, feed, weights, QS)
        assert got.shape == (len(QS), case["B"]) and got.dtype == torch.float32 and got.device == theta.device
        masses = prod._masses[:n].cpu().numpy().view(np.uint32).astype(np.uint64)
        w64 = torch.as_tensor(weights).double().cpu().numpy()
        assert np.abs(masses.astype(np.float64) - w64 / w64.sum() * 2.0 ** 31).max() <= 0.5 + n * 2.0 ** -21
        assert np.array_equal(got.cpu().numpy(), _by_definition(pred, masses, QS))
    # integer counts: exactly np.repeat
    c = rng.integers(0, 4, size=n)
    c[3] = 2
    for counts in (c, torch.tensor(c, dtype=torch.int64, device=cuda), c.astype(np.int32)):
        got = prod.weighted_quantiles(theta, feed, counts, QS).cpu().numpy()
        rep = np.sort(np.repeat(pred, c, axis=0), axis=0)
        want = rep[[wq.target(q, int(c.sum())) for q in QS]]
        assert np.array_equal(got, want)
    # uniform integer weights at the half-step levels are the order statistics
    ranks = [0, 1, n // 2, n - 1]
    got = prod.weighted_quantiles(theta, feed, np.ones(n, np.int64), [wq.half_step(r, n) for r in ranks])
    assert torch.equal(got, prod.order_statistics(theta, feed, ranks))
    # bad weights: NaN rows, no exception
    bad = w.copy()
    bad[1] = -1.0
    assert bool(torch.isnan(prod.weighted_quantiles(theta, feed, bad, (0.5,))).all())
    assert bool(torch.isnan(prod.weighted_quantiles(theta, feed, np.zeros(n, np.int64), (0.5,))).all())
    assert not bool(torch.isnan(prod.weighted_quantiles(theta, feed, np.full(n, 1.5), (0.5,))).any())   # floats are normalised


def test_value_errors(cuda):
    case = qc.CASES[0]
    a, prod, theta, feed = _setup(case, cuda)
    n = case["n"]
    w = np.ones(n)
    for bad in ((-0.1,), (1.0001,), (0.5, float("nan")), ()):
        with pytest.raises(ValueError):
            prod.weighted_quantiles(theta, feed, w, bad)
    for bad in (np.ones(n - 1), np.ones((n, 1)), np.ones(n, bool), np.ones(n, np.complex128)):
        with pytest.raises(ValueError):
            prod.weighted_quantiles(theta, feed, bad, (0.5,))
    with pytest.raises(ValueError):
        prod.weighted_quantiles(theta.double(), feed, w, (0.5,))
    with pytest.raises(ValueError):
        prod.weighted_quantiles(theta, {"X": feed["X"][:, :1].contiguous()}, w, (0.5,))


def test_predictive_quantiles_of_a_sampler(cuda):
    from stein_amd.optimizers import AdamGradientDescent
    from stein_amd.predict import GlmPredict
    from stein_amd.samplers import SteinSampler
    from stein_amd.scores import GlmScore
    n, F, B, ntr = 64, 9, 50, 400
    rng = np.random.default_rng(0)
    Xtr = rng.normal(size=(ntr, F))
    ytr = (rng.uniform(size=ntr) < 1.0 / (1.0 + np.exp(-Xtr @ rng.normal(size=F)))).astype(np.float64)
    full = {"X": torch.tensor(Xtr, dtype=torch.float32, device=cuda), "y": torch.tensor(ytr, dtype=torch.float32, device=cuda)}
    init = {"model/w:0": rng.normal(size=(n, F, 1)) * 0.6, "model/log_alpha:0": rng.normal(size=(n,)) * 0.6}
    s = SteinSampler(n, None, AdamGradientDescent(learning_rate=1e-2), theta=init, device=cuda,
                     score=GlmScore("logistic", F, w_col=1, alpha_col=0, n_train=ntr))
    for _ in range(3):
        s.train_on_batch(full)
    feed = {"X": torch.tensor(rng.normal(size=(B, F)), dtype=torch.float32, device=cuda)}
    prod = GlmPredict("logistic", F, w_col=1, output="mean")
    qs = (0.05, 0.5, 0.95)
    theta = s._matrix_f32()
    # without weights: producer.quantiles, to the bit
    plain = s.predictive_quantiles(prod, feed, qs)
    assert isinstance(plain, np.ndarray) and plain.shape == (3, B) and plain.dtype == np.float32
    assert np.array_equal(plain, prod.quantiles(theta, feed, qs).cpu().numpy())
    assert np.array_equal(plain, s.posterior_predictive(prod, feed, quantiles=qs)["quantiles"])
    # importance weights
    w, _ = s.importance_weights(full, iters=40)
    band = s.predictive_quantiles(prod, feed, qs, weights=w)
    assert isinstance(band, np.ndarray) and band.shape == (3, B) and band.dtype == np.float32
    assert np.array_equal(band, prod.weighted_quantiles(theta, feed, w, qs).cpu().numpy())
    pred = prod(theta, feed).cpu().numpy()
    masses = prod._masses[:n].cpu().numpy().view(np.uint32).astype(np.uint64)
    assert np.array_equal(band, _by_definition(pred, masses, qs))
    assert (band[0] <= band[1]).all() and (band[1] <= band[2]).all()
    # thinning counts: the band of the thinned multiset, without gathering it
    idx = s.thin(16, full)
    counts = torch.bincount(idx, minlength=n)
    band = s.predictive_quantiles(prod, feed, qs, weights=counts)
    gathered = prod.order_statistics(theta[idx].contiguous(), feed, [wq.target(q, 16) for q in qs]).cpu().numpy()
    assert np.array_equal(band, gathered)
    # posterior_predictive keeps refusing the combination and now says where to go
    with pytest.raises(ValueError, match="weighted quantiles.*predictive_quantiles"):
        s.posterior_predictive(prod, feed, weights=w, quantiles=qs)
    with pytest.raises(ValueError):
        s.predictive_quantiles(lambda th, fd: None, feed, qs)
    with pytest.raises(ValueError):
        s.predictive_quantiles(prod, feed, (1.5,), weights=w)
