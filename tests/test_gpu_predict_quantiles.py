"""GPU: the Python side of the predictive order statistics -- ``producer.order_statistics`` / ``producer.quantiles``
(stein_amd/predict.py) and ``sampler.posterior_predictive(..., quantiles=...)``.

quantiles are held against np.quantile (fp64) of the producer's OWN pred: "lower" / "higher" exactly; "linear" inside
3 * 2^-23 * max(|lo|, |hi|) -- lo + (hi - lo) * frac in fp32 is three roundings (the difference, the product, the sum) on a
difference of at most 2 max -- and exactly where the position q (n - 1) is an integer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import quantile_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
QS = (0.0, 1.0, 0.5, 0.05, 0.95, 0.3337, 0.9, 0.013)       # ten ranks under "linear": more than one call of the library


def _producer(case, a):
    from stein_amd.predict import BnnPredict, GlmPredict
    if case["model"] == "bnn":
        return BnnPredict(case["n_in"], case["H"], a["cols"], output=case["output"])
    return GlmPredict(case["model"], case["F"], w_col=a["w_col"], output=case["output"])


def _setup(case, dev):
    a = pc.args(case)
    theta = torch.tensor(a["theta"], dtype=torch.float32, device=dev)
    feed = {"X": torch.tensor(a["X"], dtype=torch.float32, device=dev), "y": torch.tensor(a["y"], dtype=torch.float32, device=dev)}
    return a, _producer(case, a), theta, feed


@pytest.mark.parametrize("case", [qc.CASES[1], qc.CASES[4]], ids=lambda c: c["name"])   # n = 45 (odd: q = 0.5 is a rank), 40
def test_quantiles_against_numpy_of_the_own_pred(cuda, case):
    a, prod, theta, feed = _setup(case, cuda)
    n = case["n"]
    pred = prod(theta, feed).cpu().numpy().astype(np.float64)
    srt = np.sort(pred, axis=0)
    for mode in ("lower", "higher"):
        got = prod.quantiles(theta, feed, QS, interpolation=mode).cpu().numpy()
        want = np.quantile(pred, QS, axis=0, method=mode)
        assert got.shape == (len(QS), case["B"]) and got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), want), mode
    got = prod.quantiles(theta, feed, QS).cpu().numpy().astype(np.float64)
    want = np.quantile(pred, QS, axis=0)
    far = 0
    for i, q in enumerate(QS):
        pos = q * (n - 1)
        lo, hi = srt[int(np.floor(pos))], srt[int(np.ceil(pos))]
        if pos == np.floor(pos):
            assert np.array_equal(got[i], lo), q                    # an order statistic itself
        else:
            far += min(pos - np.floor(pos), np.ceil(pos) - pos) > 0.1
            bound = 3.0 * 2.0 ** -23 * np.maximum(np.abs(lo), np.abs(hi))
            err = np.abs(got[i] - want[i])
            print("%-14s q=%.4f max |err| / bound = %.3f" % (case["name"], q, float((err / bound).max())))
            assert (err <= bound).all(), q
    assert far >= 3                                                  # positions far from an integer are among them
    stats = prod.order_statistics(theta, feed, range(n)).cpu().numpy()        # every rank: n / 8 calls of the library
    assert np.array_equal(stats.astype(np.float64), srt)
    again = prod.order_statistics(theta, feed, [n - 1, 0, 0])
    assert np.array_equal(again.cpu().numpy(), stats[[n - 1, 0, 0]])


def test_value_errors(cuda):
    case = qc.CASES[0]
    a, prod, theta, feed = _setup(case, cuda)
    for bad in ((-0.1,), (1.0001,), (0.5, float("nan")), ()):
        with pytest.raises(ValueError):
            prod.quantiles(theta, feed, bad)
    with pytest.raises(ValueError):
        prod.quantiles(theta, feed, (0.5,), interpolation="nearest")
    for bad in ((), (case["n"],), (-1,)):
        with pytest.raises(ValueError):
            prod.order_statistics(theta, feed, bad)


def test_posterior_predictive_quantiles_key(cuda):
    from stein_amd.optimizers import AdamGradientDescent
    from stein_amd.predict import GlmPredict
    from stein_amd.samplers import SteinSampler
    n, F, B = 41, 9, 50
    rng = np.random.default_rng(0)
    init = {"model/w:0": rng.normal(size=(n, F, 1)) * 0.6, "model/log_alpha:0": rng.normal(size=(n,)) * 0.6}
    s = SteinSampler(n, lambda th, feed: None, AdamGradientDescent(learning_rate=1e-2), theta=init, device=cuda)
    feed = {"X": torch.tensor(rng.normal(size=(B, F)), dtype=torch.float32, device=cuda),
            "y": torch.tensor((rng.uniform(size=B) < 0.5).astype(np.float64), dtype=torch.float32, device=cuda)}
    prod = GlmPredict("logistic", F, w_col=1, output="mean")       # packed by sorted name: log_alpha, then the weights
    plain = s.posterior_predictive(prod, feed)
    assert set(plain) == {"mean", "var", "lpd"}
    qs = (0.05, 0.5, 0.95)
    out = s.posterior_predictive(prod, feed, quantiles=qs)
    assert set(out) == {"mean", "var", "lpd", "quantiles"}
    for k in plain:
        assert np.array_equal(out[k], plain[k]), k                   # the other keys are what they were
    band = out["quantiles"]
    assert isinstance(band, np.ndarray) and band.shape == (3, B) and band.dtype == np.float32
    assert np.array_equal(band, prod.quantiles(s._matrix_f32(), feed, qs).cpu().numpy())
    pred = prod(s._matrix_f32(), feed).cpu().numpy().astype(np.float64)
    assert np.array_equal(band[1].astype(np.float64), np.sort(pred, axis=0)[n // 2])      # the median of an odd n: an element
    assert np.abs(band - np.quantile(pred, qs, axis=0)).max() <= 3.0 * 2.0 ** -23         # outputs in (0, 1)
    assert (band[0] <= band[1]).all() and (band[1] <= band[2]).all()
    with pytest.raises(ValueError, match="weighted quantiles"):
        s.posterior_predictive(prod, feed, weights=np.ones(n), quantiles=qs)
