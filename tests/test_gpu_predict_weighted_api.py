"""GPU: the weighted predictive summaries behind the public interface -- GlmPredict / BnnPredict.weighted_summary and
SteinSampler.posterior_predictive(weights=) against NumPy fp64 statistics of the producer's own [n, batch] outputs, with
weights from sampler.importance_weights and from torch.bincount(sampler.thin(...)); weights=None is what it was, to the
bit; argument errors are ValueErrors."""
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.optimizers import AdamGradientDescent
from stein_amd.predict import BnnPredict, GlmPredict
from stein_amd.samplers import SteinSampler
from stein_amd.scores import GlmScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_ref as pr  # noqa: E402
import predict_weighted_ref as pwr  # noqa: E402

pytestmark = pytest.mark.gpu
F, H = 9, 12
GLM_VARS = {"model/w:0": [F, 1], "model/log_alpha:0": []}     # packed by sorted name: log_alpha, then the weights
BNN_VARS = {"model/w_1:0": [1, H], "model/b_1:0": [H], "model/w_2:0": [H, 1], "model/b_2:0": [], "model/log_lambda:0": [],
            "model/log_gamma:0": []}
BNN_COLS = (H + 3, 0, 2 * H + 3, H, H + 2, H + 1)              # as tests/test_gpu_predict_api.py


def _sampler(n, shapes, dev, score=None, seed=0):
    rng = np.random.default_rng(seed)
    init = {k: rng.normal(size=[n] + s) * 0.6 for k, s in shapes.items()}
    return SteinSampler(n, None if score is not None else (lambda th, feed: None), AdamGradientDescent(learning_rate=1e-2),
                        theta=init, score=score, device=dev)


def _feed(B, width, dev, binary, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(B, width)) if width == 1 else rng.normal(size=(B, width))
    y = (rng.uniform(size=B) < 0.5).astype(np.float64) if binary else rng.normal(size=B)
    return {"X": torch.tensor(X, dtype=torch.float32, device=dev), "y": torch.tensor(y, dtype=torch.float32, device=dev)}


def _numpy_fp64(s, prod, feed, w):
    """weighted statistics in NumPy fp64 of the producer's own outputs, and the allowance of their reduction alone"""
    f = prod(s._matrix_f32(), feed).double().cpu().numpy()                    # [n, B]: what the summaries are of
    z = f
    if isinstance(prod, GlmPredict) and prod.output == 1 and prod.kind == 1:   # sigmoid outputs: the logits from a link call
        z = GlmPredict("logistic", prod.n_feats, w_col=prod.w_col)(s._matrix_f32(), feed).double().cpu().numpy()
    y = feed["y"].double().cpu().numpy()
    th = s._matrix_f32().double().cpu().numpy()
    if isinstance(prod, BnnPredict):
        l, dl = pwr.loglik("bnn", z, np.zeros_like(z), y, log_gamma=th[:, prod._cols[5]])
    else:
        l, dl = pwr.loglik("logistic" if prod.kind == 1 else "linear", z, np.zeros_like(z), y, prod.noise_precision)
    w = np.asarray(w, np.float64)
    keep = w > 0
    mean = np.average(f[keep], axis=0, weights=w[keep])
    var = np.average((f[keep] - mean) ** 2, axis=0, weights=w[keep])
    lpd = np.log((w[keep, None] * np.exp(l[keep])).sum(0) / w.sum())
    _, slices, per = pc.plan(f.shape[0], f.shape[1])
    _, a_mean, _, a_var = pwr.mean_var(f, np.zeros_like(f), w, per, slices)
    _, a_lpd = pwr.lpd(l, dl, w, per, slices)
    return dict(mean=(mean, a_mean), var=(var, a_var), lpd=(lpd, a_lpd), ess=(w.sum() ** 2 / (w * w).sum(), None))


def _check(tag, got, ref):
    for k in ("mean", "var", "lpd"):
        val, allow = ref[k]
        err = np.abs(np.asarray(got[k], np.float64) - val)
        print("%-34s %-4s max |err| / allowance = %.3f" % (tag, k, (err / allow).max()))
        assert (err <= allow).all(), (tag, k, (err / allow).max())
    assert float(got["ess"]) == pytest.approx(ref["ess"][0], rel=1e-12)


@pytest.mark.parametrize("which", ["logistic_mean", "linear", "network"])
def test_weighted_summary_and_posterior_predictive_against_numpy(cuda, which):
    n, B = 83, 70
    if which == "network":
        s, prod, feed = _sampler(n, BNN_VARS, cuda), BnnPredict(1, H, BNN_COLS), _feed(B, 1, cuda, False)
    elif which == "linear":
        s, prod, feed = _sampler(n, GLM_VARS, cuda), GlmPredict("linear", F, w_col=1, noise_precision=0.7), _feed(B, F, cuda, False)
    else:
        s, prod, feed = _sampler(n, GLM_VARS, cuda), GlmPredict("logistic", F, w_col=1, output="mean"), _feed(B, F, cuda, True)
    rng = np.random.default_rng(2)
    w = rng.exponential(size=n)
    w[rng.integers(0, n, size=20)] = 0.0
    ref = _numpy_fp64(s, prod, feed, w)
    for form, weights in (("float64 device tensor", torch.tensor(w, device=cuda)), ("NumPy array", w),
                          ("float32 host tensor", torch.tensor(w, dtype=torch.float32)),
                          ("strided view", torch.tensor(np.stack([w, w], 1), device=cuda)[:, 0])):
        mean, var, lpd, ess = prod.weighted_summary(s._matrix_f32(), feed, weights)
        assert ess.dtype == torch.float64 and ess.shape == (1,) and ess.device == s.theta_matrix.device
        assert all(t.dtype == torch.float32 and t.shape == (B,) for t in (mean, var, lpd))
        r = ref if "float32" not in form else _numpy_fp64(s, prod, feed, np.asarray(w, np.float32))
        _check("%s %s" % (which, form), dict(mean=mean.cpu().numpy(), var=var.cpu().numpy(), lpd=lpd.cpu().numpy(), ess=ess.item()), r)
    out = s.posterior_predictive(prod, feed, weights=torch.tensor(w, device=cuda))
    assert sorted(out) == ["ess", "lpd", "mean", "var"] and isinstance(out["ess"], float)
    mean, var, lpd, ess = prod.weighted_summary(s._matrix_f32(), feed, torch.tensor(w, device=cuda))
    for k, t in (("mean", mean), ("var", var), ("lpd", lpd)):
        assert out[k].dtype == np.float32 and np.array_equal(out[k].view(np.int32), t.cpu().numpy().view(np.int32)), k
    assert out["ess"] == ess.item()
    no_y = s.posterior_predictive(prod, {"X": feed["X"]}, weights=w)
    assert sorted(no_y) == ["ess", "mean", "var"] and np.array_equal(no_y["mean"], out["mean"]) and np.array_equal(no_y["var"], out["var"])
    m2, v2, l2, _ = prod.weighted_summary(s._matrix_f32(), feed, w, lpd=False)
    assert l2 is None and torch.equal(m2, mean) and torch.equal(v2, var)


def test_weights_from_importance_weights_and_from_thinning(cuda):
    rng = np.random.default_rng(7)
    ntr, n = 400, 64
    Xtr = rng.normal(size=(ntr, F))
    ytr = (rng.uniform(size=ntr) < 1.0 / (1.0 + np.exp(-Xtr @ rng.normal(size=F)))).astype(np.float64)
    full = {"X": torch.tensor(Xtr, dtype=torch.float32, device=cuda), "y": torch.tensor(ytr, dtype=torch.float32, device=cuda)}
    score = GlmScore("logistic", F, w_col=1, alpha_col=0, n_train=ntr)
    s = _sampler(n, GLM_VARS, cuda, score=score)
    for _ in range(5):
        s.train_on_batch(full)
    feed = _feed(40, F, cuda, True)
    prod = GlmPredict("logistic", F, w_col=1)
    w, _ = s.importance_weights(full, iters=60)
    assert w.dtype == torch.float64 and w.is_cuda
    out = s.posterior_predictive(prod, feed, weights=w)
    _check("importance weights", out, _numpy_fp64(s, prod, feed, w.cpu().numpy()))
    assert 1.0 <= out["ess"] <= n
    idx = s.thin(16, full)
    counts = torch.bincount(idx, minlength=n)
    assert counts.dtype == torch.int64 and int(counts.sum()) == 16
    out = s.posterior_predictive(prod, feed, weights=counts)                     # integer weights, as bincount gives them
    _check("thinning counts", out, _numpy_fp64(s, prod, feed, counts.cpu().numpy()))
    # the same multiset gathered and summarised unweighted: two evaluations of one exact value
    # (apart by at most the two reductions' allowances; pred is the same arithmetic for the same particle in both)
    ref = _numpy_fp64(s, prod, feed, counts.cpu().numpy())
    gathered = dict(zip(("mean", "var", "lpd"), prod.summary(s._matrix_f32()[idx].contiguous(), feed)))
    f = prod(s._matrix_f32()[idx].contiguous(), feed).double().cpu().numpy()
    l, dl = pr.loglik("logistic", f, np.zeros_like(f), feed["y"].double().cpu().numpy())
    _, slices, per = pc.plan(16, 40)
    _, a_mean, _, a_var = pr.mean_var(f, np.zeros_like(f), per, slices)
    _, a_lpd = pr.lpd(l, dl, per, slices)
    for k, a_u in (("mean", a_mean), ("var", a_var), ("lpd", a_lpd)):
        assert (np.abs(out[k].astype(np.float64) - gathered[k].double().cpu().numpy()) <= ref[k][1] + a_u).all(), k


def test_without_weights_nothing_changed(cuda):
    s = _sampler(41, GLM_VARS, cuda)
    feed = _feed(50, F, cuda, True)
    prod = GlmPredict("logistic", F, w_col=1, output="mean")
    mean, var, lpd = prod.summary(s.theta_matrix, feed)
    for out in (s.posterior_predictive(prod, feed), s.posterior_predictive(prod, feed, None), s.posterior_predictive(prod, feed, weights=None)):
        assert sorted(out) == ["lpd", "mean", "var"]
        for k, t in (("mean", mean), ("var", var), ("lpd", lpd)):
            assert out[k].dtype == np.float32 and np.array_equal(out[k].view(np.int32), t.cpu().numpy().view(np.int32)), k
    prod.weighted_summary(s.theta_matrix, feed, np.ones(41))                   # a weighted call in between changes nothing
    again = prod.summary(s.theta_matrix, feed)
    assert all(torch.equal(a, b) for a, b in zip(again, (mean, var, lpd)))


def test_argument_errors_are_value_errors(cuda):
    n = 8
    s = _sampler(n, GLM_VARS, cuda)
    feed = _feed(10, F, cuda, True)
    prod = GlmPredict("logistic", F, w_col=1)
    for bad in (np.ones(n - 1), np.ones(n + 1), np.ones((n, 1)), np.ones((1, n)), np.float64(1.0), np.ones(n, dtype=bool),
                np.ones(n, dtype=np.complex128), torch.ones(n, dtype=torch.bool, device=cuda),
                torch.ones(n, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            prod.weighted_summary(s.theta_matrix, feed, bad)
        with pytest.raises(ValueError):
            s.posterior_predictive(prod, feed, weights=bad)
    with pytest.raises(ValueError):
        prod.weighted_summary(s.theta_matrix, {"X": feed["X"]}, np.ones(n), lpd=True)     # lpd without y
    with pytest.raises(ValueError):
        prod.weighted_summary(s.theta_matrix.double(), feed, np.ones(n))
    with pytest.raises(ValueError):
        s.posterior_predictive(lambda th, f: th, feed, weights=np.ones(n))                 # not a producer
    s._group = object()                                     # stands for a process group: the check precedes any collective
    with pytest.raises(ValueError, match="one rank"):
        s.posterior_predictive(prod, feed, weights=np.ones(n))
    bad_w = np.ones(n)
    bad_w[3] = -1.0
    s._group = None
    out = s.posterior_predictive(prod, feed, weights=bad_w)                                # device data: NaN, not an error
    assert all(np.isnan(out[k]).all() for k in ("mean", "var", "lpd")) and np.isnan(out["ess"])
