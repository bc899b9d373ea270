"""GPU: a 13-input, 50-hidden network through the public sampler API -- two train_on_batch steps with the device score
producer (BnnScore -> stein_score_bnn_wide) and with the autograd score of the same log posterior, from the same particles;
after the first step the particles agree to the score allowance propagated through the SVGD map and one Adam step; then
posterior_predictive on the result (BnnPredict -> stein_predict_bnn_wide).

The bound (stated here, derived, not tuned; u = 2^-24, gamma(m) = m u / (1 - m u), n particles, d parameters):

  scores    Both routes evaluate the score of tests/score_ref.py in fp32, so each lies within that reference's allowance A
            of the exact score G*:  |G^a - G^b| <= 2 A elementwise.
  phi       phi = (K G + dK) / n with K = exp(-D / 2 h2) in (0, 1] and dK functions of the particles alone: the same bits in
            both runs.  In exact arithmetic |phi^a - phi^b|_ic <= (2 / n) sum_j A_jc.  The one-kernel engine (n <= 160) sums
            the 2 n terms of an element in fp32: each run errs by at most gamma(2 n + 8) S_ic, S_ic = (1 / n) sum_j (|G*_jc| +
            A_jc + (|theta_ic| + |theta_jc|) / h2), so   dp_ic = (2 / n) sum_j A_jc + 2 gamma(2 n + 8) S_ic.
  clip      |phi|_2 <= |phi*|_2 + |dp / 2 + EK|_2 (phi* and EK below) stays under the clip threshold (asserted; the noise
            precisions start near e^-4, which keeps the scores small): the clip scale is exactly 1 in both runs.
  Adam      the first step is l (p / k1) / (eps + sqrt(p^2 / k2)) = c l f(p), c = sqrt(k2) / k1, f(p) = p / (e + |p|),
            e = eps sqrt(k2).  f is odd and increasing with |f| < 1, and for any a, b: |f(a) - f(b)| <= |a - b| / (e + min(|a|,
            |b|)) (same sign: e |a - b| / ((e + |a|)(e + |b|)); opposite signs: |a| / (e + |a|) + |b| / (e + |b|)), and <= 2.
            min(|p^a|, |p^b|) >= |phi*| - dp / 2 - EK, phi* the fp64 value from G* and the engine's own h2, EK the effect
            of the fp32 distances and expf on K (relative gamma(d + 3) (r_i + r_j) / h2 + 8 u per entry, r the row norms).
  rounding  each run rounds the six operations of its step (|step| <= c l) and theta + step:  gamma(8) c l + u (|theta| + c l).

  |theta^a - theta^b|_ic <= c l min(2, dp / (e + max(0, |phi*| - dp / 2 - EK))) + 2 (gamma(8) c l + u (|theta_ic| + c l))"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.optimizers import AdamGradientDescent
from stein_amd.optimizers.abstract_gradient_descent import CLIP_THRESHOLD
from stein_amd.optimizers.adam_gradient_descent import EPS
from stein_amd.predict import BnnPredict
from stein_amd.samplers import SteinSampler
from stein_amd.scores import BnnScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
F, H, N, B = 13, 50, 20, 100
N_TRAIN, GA, GB, LR = 500.0, 1.0, 0.01, 1e-2
SHAPES = {"model/w_1:0": [F, H], "model/b_1:0": [H], "model/w_2:0": [H, 1], "model/b_2:0": [],
          "model/log_lambda:0": [], "model/log_gamma:0": []}


def _log_posterior(theta, feed, a=GA, b=GB):
    def normal_logpdf(x, log_prec):
        return 0.5 * log_prec - 0.5 * log_prec.exp() * x ** 2 - 0.5 * math.log(2 * math.pi)

    def gamma_logpdf_of_exp(log_x):
        return a * math.log(b) - math.lgamma(a) + (a - 1) * log_x - b * log_x.exp()
    w1, b1, w2, b2 = theta["model/w_1:0"], theta["model/b_1:0"], theta["model/w_2:0"], theta["model/b_2:0"]
    log_lam, log_gam = theta["model/log_lambda:0"], theta["model/log_gamma:0"]
    hidden = torch.relu(torch.einsum("pf,nfh->nph", feed["X"], w1) + b1[:, None, :])
    pred = torch.einsum("nph,nh->np", hidden, w2[:, :, 0]) + b2[:, None]
    log_l = normal_logpdf(pred - feed["y"][None, :], log_gam[:, None]).sum(1)
    prior = gamma_logpdf_of_exp(log_lam) + gamma_logpdf_of_exp(log_gam) + normal_logpdf(b2, log_lam)
    for v in (w1, b1, w2):
        prior = prior + normal_logpdf(v.reshape(v.shape[0], -1), log_lam[:, None]).sum(1)
    return (log_l * N_TRAIN / feed["X"].shape[0] + prior) / N_TRAIN


def _sampler(init, cuda):
    return SteinSampler(N, _log_posterior, AdamGradientDescent(learning_rate=LR, decay=1.0), theta={k: v.copy() for k, v in init.items()},
                        model_vars=SHAPES, device=cuda)


def test_two_steps_with_the_device_score_follow_the_autograd_score(cuda):
    rng = np.random.default_rng(13)
    scale = {"model/w_1:0": 0.4, "model/b_1:0": 0.4, "model/w_2:0": 0.4, "model/b_2:0": 0.4, "model/log_lambda:0": 0.3, "model/log_gamma:0": 0.3}
    init = {k: rng.normal(size=[N] + s) * scale[k] for k, s in SHAPES.items()}
    init["model/log_gamma:0"] -= 4.0
    feeds = [{"X": torch.tensor(rng.normal(size=(B, F)), dtype=torch.float32, device=cuda),
              "y": torch.tensor(rng.normal(size=B), dtype=torch.float32, device=cuda)} for _ in range(2)]
    dev_s, auto_s = _sampler(init, cuda), _sampler(init, cuda)
    cols = BnnScore.columns(dev_s._access)
    d = dev_s.n_params
    assert d == F * H + 2 * H + 3
    dev_s.score = BnnScore(F, H, cols, n_train=N_TRAIN, gamma_a=GA, gamma_b=GB)
    th0 = dev_s.theta_matrix.detach().clone()
    assert torch.equal(th0, auto_s.theta_matrix) and th0.dtype == torch.float32
    # the two scores at the start, each inside the allowance (the premise of the bound)
    T = th0.double()
    Gs, A, share = sr.bnn_score(T, F, H, cols, feeds[0]["X"].double(), feeds[0]["y"].double(), N_TRAIN, GA, GB)
    assert share <= 0.02, share
    ga, gb_ = dev_s.score_matrix(feeds[0]), auto_s.score_matrix(feeds[0])
    for name, g in (("device", ga), ("autograd", gb_)):
        ratio = float(((g.double() - Gs).abs() / A.clamp_min(1e-300))[A > 0].max())
        print("%s score: max |err| / allowance = %.3f" % (name, ratio))
        assert ratio <= 1.0, name
    dev_s.train_on_batch(feeds[0])
    auto_s.train_on_batch(feeds[0])
    torch.cuda.synchronize()
    h2 = float(dev_s.engine.h2.item())
    assert h2 == float(auto_s.engine.h2.item()) and h2 > 0
    # ---- the bound of the docstring, in fp64 on the device -------------------------------------------------------------
    u, g = sr.U, sr.gamma
    absT = T.abs()
    r = (T * T).sum(1)
    D = (r[:, None] + r[None, :] - 2.0 * T @ T.t()).clamp_min(0.0)
    K = torch.exp(-D / (2.0 * h2))
    phi_star = (K @ Gs + (K.sum(1)[:, None] * T - K @ T) / h2) / N
    S = ((Gs.abs() + A).sum(0)[None, :] + (N * absT + absT.sum(0)[None, :]) / h2) / N
    dp = 2.0 * A.sum(0)[None, :] / N + 2.0 * g(2 * N + 8) * S
    EKrel = g(d + 3) * (r[:, None] + r[None, :]) / h2 + 8.0 * u
    EK = EKrel * K
    EKphi = (EK @ (Gs.abs() + A) + (EK.sum(1)[:, None] * absT + EK @ absT) / h2) / N
    assert float(phi_star.norm()) + float((0.5 * dp + EKphi).norm()) < CLIP_THRESHOLD        # no clip in either run
    k1, k2 = 1.0 - 0.9, 1.0 - 0.999                                  # AdamGradientDescent's defaults, first step
    c, e = math.sqrt(k2) / k1, EPS * math.sqrt(k2)
    lower = (phi_star.abs() - 0.5 * dp - EKphi).clamp_min(0.0)
    bound = c * LR * torch.minimum(torch.full_like(dp, 2.0), dp / (e + lower)) + 2.0 * (g(8) * c * LR + u * (absT + c * LR))
    diff = (dev_s.theta_matrix.double() - auto_s.theta_matrix.double()).abs()
    moved = (dev_s.theta_matrix.double() - T).abs()
    print("first step: max |theta_dev - theta_auto| / bound = %.3f; bound / step: median %.2e, share at the vacuous 2 c l: %.4f" % (
        float((diff / bound).max()), float((bound / (c * LR)).median()), float((bound >= 2.0 * c * LR).double().mean())))
    assert bool((moved > 0).any()) and bool((moved <= c * LR * (1.0 + g(8)) + u * (absT + c * LR)).all())   # |f| < 1: a step of at most c l
    assert float((bound >= 2.0 * c * LR).double().mean()) < 0.05     # the bound says something for more than 95 % of the entries
    assert bool((diff <= bound).all()), float((diff / bound).max())
    # ---- a second step, and the predictive readout of the result ---------------------------------------------------------------
    dev_s.train_on_batch(feeds[1])
    auto_s.train_on_batch(feeds[1])
    assert bool(torch.isfinite(dev_s.theta_matrix).all()) and bool(torch.isfinite(auto_s.theta_matrix).all())
    test = {"X": torch.tensor(rng.normal(size=(37, F)), dtype=torch.float32, device=cuda),
            "y": torch.tensor(rng.normal(size=37), dtype=torch.float32, device=cuda)}
    prod = BnnPredict(F, H, cols)
    out = dev_s.posterior_predictive(prod, test)
    for k in ("mean", "var", "lpd"):
        assert isinstance(out[k], np.ndarray) and out[k].shape == (37,) and np.isfinite(out[k]).all(), k
    assert (out["var"] >= 0).all()
    wout = dev_s.posterior_predictive(prod, test, weights=np.ones(N))
    assert np.allclose(wout["mean"], out["mean"], rtol=1e-5, atol=1e-6) and np.isfinite(wout["lpd"]).all()
    pred = dev_s.function_posterior(prod, test)
    assert pred.shape == (N, 37) and np.allclose(pred.mean(0), out["mean"], rtol=1e-4, atol=1e-5)
