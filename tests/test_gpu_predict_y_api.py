"""GPU: the Python side of the predictive distribution of y -- ``producer.y_cdf`` / ``producer.y_quantiles``
(stein_amd/predict.py) and ``sampler.predictive_cdf`` / ``sampler.predictive_interval`` -- shapes and dtypes, t=None is t=y,
more than eight points and levels are split to the bit, integer counts are taken as weights, the methods agree with the C ABI
to the bit, the ValueErrors, and the example's main() at a reduced size."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_y_cases as yc  # noqa: E402

pytestmark = pytest.mark.gpu


def _producer(case, a):
    from stein_amd.predict import BnnPredict, GlmPredict
    if case["model"] == "bnn":
        return BnnPredict(case["n_in"], case["H"], a["cols"])
    return GlmPredict(case["model"], case["F"], w_col=a["w_col"], noise_precision=case["tau"])


def _setup(case, dev):
    a = pc.args(case)
    theta = torch.tensor(a["theta"], dtype=torch.float32, device=dev)
    feed = {"X": torch.tensor(a["X"], dtype=torch.float32, device=dev), "y": torch.tensor(a["y"], dtype=torch.float32, device=dev)}
    return a, _producer(case, a), theta, feed


@pytest.mark.parametrize("case", [yc.SINGLE[3], yc.SINGLE[8]], ids=lambda c: c["name"])     # a GLM and a network producer
def test_methods_against_the_c_abi(cuda, case):
    a, prod, theta, feed = _setup(case, cuda)
    n, B = case["n"], case["B"]
    rng = np.random.default_rng(3)
    t = torch.tensor(rng.normal(size=(11, B)), dtype=torch.float32, device=cuda)       # eleven points: two calls of the library
    w = rng.exponential(size=n)
    w[::5] = 0.0
    for weights in (None, w):
        got = prod.y_cdf(theta, feed, t, weights=weights)
        assert got.shape == (11, B) and got.dtype == torch.float32 and got.device == theta.device
        assert yc.same_bits(got[:8], yc.call_ycdf(case, a, t[:8].contiguous(), weights, cuda)[0])
        assert yc.same_bits(got[8:], yc.call_ycdf(case, a, t[8:].contiguous(), weights, cuda)[0])
        pit = prod.y_cdf(theta, feed, weights=weights)
        assert pit.shape == (B,) and yc.same_bits(pit, prod.y_cdf(theta, feed, feed["y"], weights=weights)[0])
        assert yc.same_bits(prod.y_cdf(theta, feed, t[0], weights=weights), got[:1])               # [batch] -> [1, batch]
        qs = (0.05, 0.95, 0.5, 0.025, 0.975, 0.25, 0.75, 0.1, 0.9, 0.3)                 # ten levels: two calls
        hi = prod.y_quantiles(theta, feed, qs, weights=weights)
        lo2, hi2 = prod.y_quantiles(theta, feed, qs, weights=weights, return_bracket=True)
        assert hi.shape == (10, B) and hi.dtype == torch.float32 and yc.same_bits(hi, hi2) and bool((lo2 <= hi2).all())
        ref_lo, ref_hi = yc.call_yquantiles(case, a, qs[:8], 8, weights, cuda)
        assert yc.same_bits(hi[:8], ref_hi) and yc.same_bits(lo2[:8], ref_lo)
        assert yc.same_bits(hi[8:], yc.call_yquantiles(case, a, qs[8:], 8, weights, cuda)[1])
        order = np.argsort(qs)
        assert bool((hi[order][:-1] <= hi[order][1:]).all())                               # (levels far apart: ordered results)
        wide = prod.y_quantiles(theta, feed, qs[:2], weights=weights, passes=2, return_bracket=True)
        assert bool((wide[0] <= lo2[:2]).all()) and bool((hi2[:2] <= wide[1]).all())
    # float32 device weights and integer counts are taken as they are
    c = rng.integers(0, 4, size=n)
    c[1] = 3
    for counts in (c, torch.tensor(c, dtype=torch.int64, device=cuda), c.astype(np.int32)):
        assert yc.same_bits(prod.y_cdf(theta, feed, t[:3].contiguous(), weights=counts),
                            yc.call_ycdf(case, a, t[:3].contiguous(), c.astype(np.float64), cuda)[0])
        assert yc.same_bits(prod.y_quantiles(theta, feed, (0.5,), weights=counts),
                            yc.call_yquantiles(case, a, (0.5,), 8, c.astype(np.float64), cuda)[1])
    bad = w.copy()
    bad[1] = -1.0
    assert bool(torch.isnan(prod.y_cdf(theta, feed, weights=bad)).all())
    assert bool(torch.isnan(prod.y_quantiles(theta, feed, (0.5,), weights=bad)).all())


def test_value_errors(cuda):
    from stein_amd.predict import GlmPredict
    case = yc.SINGLE[0]
    a, prod, theta, feed = _setup(case, cuda)
    n, B = case["n"], case["B"]
    for bad in ((0.0,), (1.0,), (0.5, float("nan")), (-0.1,), ()):
        with pytest.raises(ValueError):
            prod.y_quantiles(theta, feed, bad)
    for passes in (0, 13):
        with pytest.raises(ValueError):
            prod.y_quantiles(theta, feed, (0.5,), passes=passes)
    for bad in (np.ones(n - 1), np.ones((n, 1)), np.ones(n, bool)):
        with pytest.raises(ValueError):
            prod.y_cdf(theta, feed, weights=bad)
        with pytest.raises(ValueError):
            prod.y_quantiles(theta, feed, (0.5,), weights=bad)
    with pytest.raises(ValueError):
        prod.y_cdf(theta, {"X": feed["X"]})                                     # t=None needs feed["y"]
    for bad_t in (torch.zeros(2, B + 1, device=cuda), torch.zeros(2, B, dtype=torch.float64, device=cuda), torch.zeros(2, B),
                  torch.zeros(0, B, device=cuda)):
        with pytest.raises(ValueError):
            prod.y_cdf(theta, feed, bad_t)
    logistic = GlmPredict("logistic", case["F"], w_col=a["w_col"], output="mean")
    with pytest.raises(ValueError, match="Bernoulli"):
        logistic.y_cdf(theta, feed)
    with pytest.raises(ValueError, match="Bernoulli"):
        logistic.y_quantiles(theta, feed, (0.5,))


def test_sampler_methods(cuda):
    from stein_amd.optimizers import AdamGradientDescent
    from stein_amd.predict import GlmPredict
    from stein_amd.samplers import SteinSampler
    from stein_amd.scores import GlmScore
    n, F, B, ntr = 64, 5, 50, 300
    rng = np.random.default_rng(0)
    Xtr = rng.normal(size=(ntr, F))
    ytr = Xtr @ rng.normal(size=F) + 0.5 * rng.normal(size=ntr)
    full = {"X": torch.tensor(Xtr, dtype=torch.float32, device=cuda), "y": torch.tensor(ytr, dtype=torch.float32, device=cuda)}
    init = {"model/w:0": rng.normal(size=(n, F, 1)) * 0.6, "model/log_alpha:0": rng.normal(size=(n,)) * 0.6}
    s = SteinSampler(n, None, AdamGradientDescent(learning_rate=1e-2), theta=init, device=cuda,
                     score=GlmScore("linear", F, w_col=1, alpha_col=0, n_train=ntr))
    for _ in range(3):
        s.train_on_batch(full)
    Xte = rng.normal(size=(B, F))
    feed = {"X": torch.tensor(Xte, dtype=torch.float32, device=cuda),
            "y": torch.tensor(rng.normal(size=B), dtype=torch.float32, device=cuda)}
    prod = GlmPredict("linear", F, w_col=1, noise_precision=4.0)
    theta = s._matrix_f32()
    pit = s.predictive_cdf(prod, feed)
    assert isinstance(pit, np.ndarray) and pit.shape == (B,) and pit.dtype == np.float32
    assert np.array_equal(pit, prod.y_cdf(theta, feed).cpu().numpy()) and (pit >= 0).all() and (pit <= 1).all()
    t = rng.normal(size=(3, B))                                                   # NumPy float64 points are converted
    got = s.predictive_cdf(prod, feed, t)
    assert got.shape == (3, B) and got.dtype == np.float32
    assert np.array_equal(got, prod.y_cdf(theta, feed, torch.tensor(t, dtype=torch.float32, device=cuda)).cpu().numpy())
    band = s.predictive_interval(prod, feed, (0.05, 0.95))
    assert isinstance(band, np.ndarray) and band.shape == (2, B) and band.dtype == np.float32 and (band[0] < band[1]).all()
    assert np.array_equal(band, prod.y_quantiles(theta, feed, (0.05, 0.95)).cpu().numpy())
    # the interval holds the noise: no narrower than the 90 % interval of one component, and F at its ends is the level
    assert (band[1] - band[0] >= 2 * 1.6448 / 2.0).all()
    ends = s.predictive_cdf(prod, feed, band)
    assert np.abs(ends[0] - 0.05).max() < 1e-4 and np.abs(ends[1] - 0.95).max() < 1e-4
    w, _ = s.importance_weights(full, iters=40)
    counts = torch.bincount(s.thin(16, full), minlength=n)
    for weights in (w, counts):
        got = s.predictive_interval(prod, feed, (0.05, 0.95), weights=weights, passes=6)
        assert np.array_equal(got, prod.y_quantiles(theta, feed, (0.05, 0.95), weights=weights, passes=6).cpu().numpy())
        assert np.array_equal(s.predictive_cdf(prod, feed, weights=weights), prod.y_cdf(theta, feed, weights=weights).cpu().numpy())
    gathered = prod.y_cdf(theta[s.thin(16, full)].contiguous(), feed).cpu().numpy()      # counts = the gathered multiset
    assert np.abs(s.predictive_cdf(prod, feed, weights=counts) - gathered).max() < 1e-5
    with pytest.raises(ValueError):
        s.predictive_cdf(lambda th, fd: None, feed)
    with pytest.raises(ValueError):
        s.predictive_interval(lambda th, fd: None, feed, (0.5,))
    with pytest.raises(ValueError):
        s.predictive_interval(prod, feed, (1.0,))
    s._group = object()                                                           # a sharded sampler: one rank only
    with pytest.raises(ValueError, match="one rank only"):
        s.predictive_cdf(prod, feed)
    with pytest.raises(ValueError, match="one rank only"):
        s.predictive_interval(prod, feed, (0.5,))


def test_example_runs_at_a_reduced_size(cuda, capsys):
    spec = importlib.util.spec_from_file_location("predictive_calibration_main",
                                                  os.path.join(ROOT, "examples", "predictive_calibration", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.main(["--particles", "16", "--iters", "30", "--hidden", "8", "--train", "40", "--test", "64", "--fw-iters", "16"])
    out = capsys.readouterr().out
    assert "PIT histogram" in out and "interval of y" in out and "importance weights" in out
    for name in ("unweighted", "importance weights"):
        r = report[name]
        assert r["pit"].shape == (64,) and np.isfinite(r["pit"]).all() and abs(r["hist"].sum() - 1.0) < 1e-6
        assert (r["y_band"][0] < r["y_band"][1]).all() and 0.0 <= r["cover_f"] <= 1.0 and 0.0 <= r["cover_y"] <= 1.0
