"""CPU: the fp64 references of tests/softmax_ref.py are the model of the issue -- the score equals torch.autograd.grad of an
independently written fp64 log posterior, with two classes it is the logistic reference of tests/score_ref.py, and the
predictive summaries equal plain NumPy statistics of the softmax; and they work on NumPy arrays and torch tensors alike."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402
import softmax_ref as smr  # noqa: E402


def _problem(seed, n, F, C, B, lead, with_alpha, tail):
    rng = np.random.default_rng(seed)
    alpha_col = lead if with_alpha else -1
    w_col = lead + (1 if with_alpha else 0)
    d = w_col + F * C + tail
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    return {"theta": f32(rng.normal(size=(n, d)) * 0.7), "X": f32(rng.normal(size=(B, F))),
            "labels": rng.integers(0, C, size=B).astype(np.int32), "w_col": w_col, "alpha_col": alpha_col, "d": d}


def _log_posterior(theta, w_col, F, C, alpha_col, X, y, scale, prec, rate):
    """written from the issue's formulas with torch's own log_softmax and distributions' densities"""
    n = theta.shape[0]
    W = theta[:, w_col:w_col + F * C].reshape(n, F, C)
    logp = torch.log_softmax(torch.einsum("bf,nfc->nbc", X, W), dim=-1)
    lik = logp[:, torch.arange(X.shape[0]), y.long()].sum(-1)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731  (a Python float would make a float32 distribution)
    if alpha_col >= 0:
        alpha = torch.exp(theta[:, alpha_col])
        prior = torch.distributions.Normal(f64(0.0), alpha.rsqrt()[:, None, None]).log_prob(W).sum((-1, -2))
        prior = prior + torch.distributions.Gamma(f64(1.0), f64(rate)).log_prob(alpha)
    else:
        prior = torch.distributions.Normal(f64(0.0), f64(prec ** -0.5)).log_prob(W).sum((-1, -2))
    return scale * lik + prior


@pytest.mark.parametrize("shape", [(4, 3, 3, 7), (3, 5, 2, 1), (2, 9, 7, 12), (5, 1, 4, 6)], ids=str)
@pytest.mark.parametrize("with_alpha", [False, True], ids=["fixed", "alpha"])
def test_the_reference_score_is_autograd_of_the_log_posterior(shape, with_alpha):
    n, F, C, B = shape
    a = _problem(11 + F, n, F, C, B, 2, with_alpha, 1)
    scale, prec, rate = 2.5, 0.75, 0.01
    ref, allow = smr.score(a["theta"], a["w_col"], F, C, a["alpha_col"], a["X"], a["labels"], scale, prec, rate)
    th = torch.tensor(a["theta"], requires_grad=True)
    lp = _log_posterior(th, a["w_col"], F, C, a["alpha_col"], torch.tensor(a["X"]), torch.tensor(a["labels"]),
                        sr._f32(scale), sr._f32(prec), sr._f32(rate))
    (g,) = torch.autograd.grad(lp.sum(), th)
    g = g.numpy()
    assert np.abs(ref - g).max() <= 1e-10 * np.abs(g).max()
    assert (g[:, :a["w_col"] - (1 if with_alpha else 0)] == 0).all() and (ref[:, -1] == 0).all() and (allow[:, -1] == 0).all()
    # the same code on torch tensors
    tref, tallow = smr.score(torch.tensor(a["theta"]), a["w_col"], F, C, a["alpha_col"], torch.tensor(a["X"]),
                             torch.tensor(a["labels"]), scale, prec, rate)
    assert np.abs(tref.numpy() - ref).max() <= 1e-12 * np.abs(ref).max() and np.abs(tallow.numpy() - allow).max() <= 1e-9 * allow.max()


def test_two_classes_are_the_logistic_reference():
    n, F, B = 5, 6, 9
    a = _problem(3, n, F, 2, B, 0, False, 0)
    ref, _ = smr.score(a["theta"], 0, F, 2, -1, a["X"], a["labels"], 3.0, 0.5, 0.01)
    W = a["theta"].reshape(n, F, 2)
    w = W[:, :, 1] - W[:, :, 0]
    glm, _ = sr.glm_score(w.copy(), "logistic", 0, F, -1, a["X"], a["labels"].astype(np.float64), 3.0, 0.0, 0.01)
    lik1 = ref.reshape(n, F, 2)[:, :, 1] + sr._f32(0.5) * W[:, :, 1]             # the W[:, 1] gradient minus the prior term
    assert np.abs(lik1 - glm).max() <= 1e-12 * np.abs(glm).max()
    lik0 = ref.reshape(n, F, 2)[:, :, 0] + sr._f32(0.5) * W[:, :, 0]
    assert np.abs(lik0 + lik1).max() <= 1e-12 * np.abs(glm).max()                # the two classes' residuals cancel


def test_the_predictive_reference_is_plain_statistics_of_the_softmax():
    n, F, C, B = 23, 4, 5, 8
    a = _problem(5, n, F, C, B, 1, False, 2)
    ref = smr.predict(a["theta"], a["w_col"], F, C, a["X"], a["labels"], per=8)
    W = torch.tensor(a["theta"][:, a["w_col"]:a["w_col"] + F * C]).reshape(n, F, C)
    z = torch.einsum("bf,nfc->nbc", torch.tensor(a["X"]), W)
    p = torch.softmax(z, -1)
    close = lambda x, y: np.abs(np.asarray(x) - np.asarray(y)).max() <= 1e-12   # noqa: E731
    assert close(ref["pred_link"][0], z) and close(ref["pred_mean"][0], p) and close(ref["prob"][0], p.mean(0))
    assert close(ref["ent"][0], torch.distributions.Categorical(probs=p).entropy().mean(0))
    assert close(ref["lpd"][0], torch.log(p[:, torch.arange(B), torch.tensor(a["labels"]).long()].mean(0)))
    for k, (v, al) in ref.items():
        assert np.isfinite(v).all() and (al > 0).all() and (al < 1e-4).all(), k
    tref = smr.predict(torch.tensor(a["theta"]), a["w_col"], F, C, torch.tensor(a["X"]), torch.tensor(a["labels"]), per=8)
    for k in ref:
        assert close(tref[k][0], ref[k][0]) and np.abs(tref[k][1].numpy() - ref[k][1]).max() <= 1e-9 * ref[k][1].max(), k


def test_a_label_outside_the_classes_is_nan_where_the_calls_put_it():
    n, F, C, B = 3, 4, 3, 6
    a = _problem(8, n, F, C, B, 0, True, 1)
    for bad in (-1, C):
        labels = a["labels"].copy()
        labels[2] = bad
        ref, _ = smr.score(a["theta"], a["w_col"], F, C, a["alpha_col"], a["X"], labels)
        assert np.isnan(ref[:, a["w_col"]:a["w_col"] + F * C]).all() and np.isfinite(ref[:, a["alpha_col"]]).all()
        assert (ref[:, -1] == 0).all()
        lpd = smr.predict(a["theta"], a["w_col"], F, C, a["X"], labels, per=2)["lpd"][0]
        assert np.isnan(lpd[2]) and np.isfinite(np.delete(lpd, 2)).all()
        got = smr.predict_f32(a["theta"], a["w_col"], F, C, a["X"], labels, per=2)["lpd"]
        assert np.isnan(got[2]) and np.isfinite(np.delete(got, 2)).all()
