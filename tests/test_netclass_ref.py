"""CPU: the fp64 references of tests/netclass_ref.py are the model of the header -- the score equals torch.autograd.grad of an
independently written fp64 log posterior to 1e-10 relative, with and without log_lambda; the predictive summaries equal plain
statistics of the network's softmax; the fp32 emulation lies inside the allowance everywhere; and the allowance is not
vacuous: on some entry of every block the emulation's error reaches a hundredth of it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_cases as ncc  # noqa: E402
import netclass_ref as ncr  # noqa: E402
import score_ref as sr  # noqa: E402


def _case(n, F, H, C, B, with_lambda, seed=0):
    order = "permuted" if with_lambda else "permuted_none"
    return ncc._score("ref%d_%dx%dx%d_%d" % (seed, F, H, C, with_lambda), F, H, C, B, n, order=order, lead=2, gap=1, tail=1, scale=2.5)


def _log_posterior(theta, F, H, C, cols, X, y, scale, prec, rate):
    """written from the header's formulas with torch's own relu, log_softmax and distributions' densities"""
    n = theta.shape[0]
    blocks = [theta[:, cols[0]:cols[0] + F * H], theta[:, cols[1]:cols[1] + H], theta[:, cols[2]:cols[2] + H * C],
              theta[:, cols[3]:cols[3] + C]]
    w1, b1, w2, b2 = blocks[0].reshape(n, F, H), blocks[1], blocks[2].reshape(n, H, C), blocks[3]
    hid = torch.relu(torch.einsum("bf,nfh->nbh", X, w1) + b1[:, None, :])
    logp = torch.log_softmax(torch.einsum("nbh,nhc->nbc", hid, w2) + b2[:, None, :], dim=-1)
    lik = logp[:, torch.arange(X.shape[0]), y.long()].sum(-1)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    every = torch.cat(blocks, dim=1)
    if cols[4] >= 0:
        lam = torch.exp(theta[:, cols[4]])
        prior = torch.distributions.Normal(f64(0.0), lam.rsqrt()[:, None]).log_prob(every).sum(-1)
        prior = prior + torch.distributions.Gamma(f64(1.0), f64(rate)).log_prob(lam)
    else:
        prior = torch.distributions.Normal(f64(0.0), f64(prec ** -0.5)).log_prob(every).sum(-1)
    return scale * lik + prior


SHAPES = [(4, 3, 5, 3, 7), (3, 5, 2, 2, 1), (2, 9, 17, 7, 12), (5, 1, 4, 4, 6), (2, 13, 50, 3, 20)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("with_lambda", [False, True], ids=["fixed", "lambda"])
def test_the_reference_score_is_autograd_of_the_log_posterior(shape, with_lambda):
    n, F, H, C, B = shape
    case = _case(n, F, H, C, B, with_lambda)
    a = ncc.score_args(case)
    scale, prec, rate = 2.5, 0.75, 0.01
    ref, allow, share = ncr.score(a["theta"], F, H, C, a["cols"], a["X"], a["labels"], scale, prec, rate)
    th = torch.tensor(a["theta"], requires_grad=True)
    lp = _log_posterior(th, F, H, C, a["cols"], torch.tensor(a["X"]), torch.tensor(a["labels"]), sr._f32(scale), sr._f32(prec),
                        sr._f32(rate))
    (g,) = torch.autograd.grad(lp.sum(), th)
    g = g.numpy()
    assert np.abs(ref - g).max() <= 1e-10 * np.abs(g).max()
    live = ncc.live_columns(case)
    assert (g[:, ~live] == 0).all() and (ref[:, ~live] == 0).all() and (allow[:, ~live] == 0).all() and (allow[:, live] > 0).all()
    assert 0.0 <= share <= 1.0
    # the same code on torch tensors
    tref, tallow, tshare = ncr.score(torch.tensor(a["theta"]), F, H, C, a["cols"], torch.tensor(a["X"]), torch.tensor(a["labels"]),
                                     scale, prec, rate)
    assert np.abs(tref.numpy() - ref).max() <= 1e-12 * np.abs(ref).max() and np.abs(tallow.numpy() - allow).max() <= 1e-9 * allow.max()
    assert tshare == share


# The allowance stacks worst cases -- gamma(F + 1), gamma(H + 1) and gamma(B) each grow like the number of terms, where the
# rounding errors of a correct evaluation grow like its square root -- so how much of it a correct evaluation uses falls
# with the widths (at 54 x 100 x 7 with 100 rows: a thousandth on w1).  That it is not vacuous is therefore asserted where the
# sums are short; the wide shapes are held to the allowance itself and their ratios are printed.
SHORT_SUMS = [(4, 3, 5, 3, 7), (5, 1, 4, 4, 6), (6, 2, 3, 2, 9)]


@pytest.mark.parametrize("shape", SHORT_SUMS + [(2, 9, 17, 7, 12), (2, 13, 50, 3, 20), (3, 54, 100, 7, 100)], ids=str)
@pytest.mark.parametrize("with_lambda", [False, True], ids=["fixed", "lambda"])
def test_the_emulation_lies_inside_the_allowance_and_the_allowance_is_not_vacuous(shape, with_lambda):
    n, F, H, C, B = shape
    case = _case(n, F, H, C, B, with_lambda, seed=1)
    a = ncc.score_args(case)
    args = (a["theta"], F, H, C, a["cols"], a["X"], a["labels"], 2.5, 0.75, 0.01)
    ref, allow, _ = ncr.score(*args)
    got = ncr.score_f32(*args).astype(np.float64)
    live = ncc.live_columns(case)
    assert (np.abs(got - ref)[:, live] <= allow[:, live]).all() and (got[:, ~live] == 0).all()
    for name, sl in ncc.block_slices(case).items():
        ratio = (np.abs(got - ref)[:, sl] / allow[:, sl]).max()
        print("%-10s largest |err| / allowance = %.3f" % (name, ratio))
        assert ratio >= 0.01 or shape not in SHORT_SUMS, name


def test_the_predictive_reference_is_plain_statistics_of_the_networks_softmax():
    n, F, H, C, B = 23, 4, 9, 5, 8
    case = ncc._pred("ref_predict", F, H, C, B, n, order="permuted", lead=1, gap=1, tail=2)
    a = ncc.predict_args(case)
    cols = a["cols"]
    ref = ncr.predict(a["theta"], F, H, C, cols, a["X"], a["labels"], per=8)
    th = torch.tensor(a["theta"])
    w1, b1 = th[:, cols[0]:cols[0] + F * H].reshape(n, F, H), th[:, cols[1]:cols[1] + H]
    w2, b2 = th[:, cols[2]:cols[2] + H * C].reshape(n, H, C), th[:, cols[3]:cols[3] + C]
    z = torch.einsum("nbh,nhc->nbc", torch.relu(torch.einsum("bf,nfh->nbh", torch.tensor(a["X"]), w1) + b1[:, None, :]), w2) + b2[:, None, :]
    p = torch.softmax(z, -1)
    close = lambda x, y: np.abs(np.asarray(x) - np.asarray(y)).max() <= 1e-12   # noqa: E731
    assert close(ref["pred_link"][0], z) and close(ref["pred_mean"][0], p) and close(ref["prob"][0], p.mean(0))
    assert close(ref["ent"][0], torch.distributions.Categorical(probs=p).entropy().mean(0))
    assert close(ref["lpd"][0], torch.log(p[:, torch.arange(B), torch.tensor(a["labels"]).long()].mean(0)))
    for k, (v, al) in ref.items():
        assert np.isfinite(v).all() and (al > 0).all() and (al < 1e-4).all(), k
    tref = ncr.predict(th, F, H, C, cols, torch.tensor(a["X"]), torch.tensor(a["labels"]), per=8)
    for k in ref:
        assert close(tref[k][0], ref[k][0]) and np.abs(tref[k][1].numpy() - ref[k][1]).max() <= 1e-9 * ref[k][1].max(), k
    got = ncr.predict_f32(a["theta"], F, H, C, cols, a["X"], a["labels"], per=8)
    for k, (v, al) in ref.items():
        err = np.abs(np.asarray(got[k], np.float64) - v)
        assert (err <= al).all() and (err / al).max() >= 0.01, k


def test_a_label_outside_the_classes_is_nan_where_the_calls_put_it():
    a = ncc.score_args(ncc.BAD_LABEL_CASE)
    F, H, C = a["F"], a["H"], a["C"]
    live = ncc.live_columns(ncc.BAD_LABEL_CASE)
    for bad in (-1, C):
        labels = a["labels"].copy()
        labels[2] = bad
        ref, _, _ = ncr.score(a["theta"], F, H, C, a["cols"], a["X"], labels)
        four = live.copy()
        four[a["cols"][4]] = False
        assert np.isnan(ref[:, four]).all() and np.isfinite(ref[:, a["cols"][4]]).all() and (ref[:, ~live] == 0).all()
        lpd = ncr.predict(a["theta"], F, H, C, a["cols"], a["X"], labels, per=2)["lpd"][0]
        assert np.isnan(lpd[2]) and np.isfinite(np.delete(lpd, 2)).all()
        got = ncr.predict_f32(a["theta"], F, H, C, a["cols"], a["X"], labels, per=2)["lpd"]
        assert np.isnan(got[2]) and np.isfinite(np.delete(got, 2)).all()
