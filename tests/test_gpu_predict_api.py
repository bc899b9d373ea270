"""GPU: the predictive producers behind the public interface -- function_posterior(GlmPredict / BnnPredict) against the
examples' own torch callables inside the allowance of tests/predict_ref.py, posterior_predictive against .summary to the
bit, argument errors as ValueError, and the dict of views for every callable that does not ask for the matrix."""
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.optimizers import AdamGradientDescent
from stein_amd.predict import BnnPredict, GlmPredict
from stein_amd.samplers import SteinSampler
from stein_amd.scores import BnnScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
F, H = 9, 12
GLM_VARS = {"model/w:0": [F, 1], "model/log_alpha:0": []}     # packed by sorted name: log_alpha, then the weights
BNN_VARS = {"model/w_1:0": [1, H], "model/b_1:0": [H], "model/w_2:0": [H, 1], "model/b_2:0": [], "model/log_lambda:0": [],
            "model/log_gamma:0": []}
# packed by sorted name: b_1, b_2, log_gamma, log_lambda, w_1, w_2 -> first columns of (w1, b1, w2, b2, log_lambda, log_gamma)
BNN_COLS = (H + 3, 0, 2 * H + 3, H, H + 2, H + 1)


def logits(th, feed):            # the callable of examples/logistic_regression/main.py
    return (feed["X"] @ th["model/w:0"][:, :, 0].T).T


def network(th, feed):           # predict() of examples/regression_neural_network/main.py
    hidden = torch.relu(torch.einsum("pf,nfh->nph", feed["X"], th["model/w_1:0"]) + th["model/b_1:0"][:, None, :])
    return torch.einsum("nph,nh->np", hidden, th["model/w_2:0"][:, :, 0]) + th["model/b_2:0"][:, None]


def _sampler(n, shapes, dtype=torch.float32, bare=False, seed=0):
    rng = np.random.default_rng(seed)
    init = {k: rng.normal(size=[n] + s) * 0.6 for k, s in shapes.items()}
    s = SteinSampler(n, lambda th, feed: None, AdamGradientDescent(learning_rate=1e-2), theta=init, dtype=dtype)
    if bare:
        s = SteinSampler(n, lambda th, feed: None, AdamGradientDescent(learning_rate=1e-2), theta=s.theta_matrix.clone(), dtype=dtype)
        assert s._access is None
    return s


def _feed(B, width, dev, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(B, width)) if width == 1 else rng.normal(size=(B, width))
    return {"X": torch.tensor(X, dtype=torch.float32, device=dev), "y": torch.tensor(rng.normal(size=B), dtype=torch.float32, device=dev)}


def _allowances(s, producer, feed):
    th = s._matrix_f32().double()
    X = feed["X"].double()
    if isinstance(producer, BnnPredict):
        z, dz, _ = pr.bnn_link(th, producer.n_in, producer.n_hidden, tuple(producer._cols), X)
    else:
        z, dz = pr.glm_link(th, producer.w_col, producer.n_feats, X)
    return z.cpu().numpy(), dz.cpu().numpy()


@pytest.mark.parametrize("dtype,bare", [(torch.float32, False), (torch.float32, True), (torch.float64, False)],
                         ids=["dict_views", "bare_matrix", "float64"])
def test_function_posterior_takes_the_producers(cuda, dtype, bare):
    n, B = 37, 70
    for shapes, prod, torch_fn, width in ((GLM_VARS, GlmPredict("logistic", F, w_col=1), logits, F),
                                          (BNN_VARS, BnnPredict(1, H, BNN_COLS), network, 1)):
        s = _sampler(n, shapes, dtype, bare)
        feed = _feed(B, width, cuda)
        if not bare and shapes is BNN_VARS:
            assert BnnScore.columns(s._access) == BNN_COLS
        got = s.function_posterior(prod, feed)
        assert isinstance(got, np.ndarray) and got.shape == (n, B) and got.dtype == np.float32
        z, dz = _allowances(s, prod, feed)
        assert (np.abs(got - z) <= dz).all()
        if not bare:                                        # the example's own callable, on the same sampler
            theirs = s.function_posterior(torch_fn, {k: v.to(s.theta_matrix.dtype) for k, v in feed.items()})
            # theirs is another evaluation of the same z: in fp32, or in fp64 of the particles before their fp32 copy
            # (one rounding per weight: within dz as well)
            assert (np.abs(got - theirs) <= 2.0 * dz).all()
        mean0 = s.function_posterior(prod, feed, axis=0)
        assert mean0.shape == (B,) and np.array_equal(mean0, got.mean(axis=0))
        assert np.array_equal(s.function_posterior(prod, feed, axis=None), got)


def test_posterior_predictive_equals_summary_to_the_bit(cuda):
    s = _sampler(41, GLM_VARS)
    feed = _feed(50, F, cuda)
    feed["y"] = (feed["y"] > 0).float()
    prod = GlmPredict("logistic", F, w_col=1, output="mean")
    out = s.posterior_predictive(prod, feed)
    mean, var, lpd = prod.summary(s.theta_matrix, feed)
    assert sorted(out) == ["lpd", "mean", "var"]
    for k, t in (("mean", mean), ("var", var), ("lpd", lpd)):
        assert out[k].dtype == np.float32 and np.array_equal(out[k].view(np.int32), t.cpu().numpy().view(np.int32)), k
    assert (out["mean"] > 0).all() and (out["mean"] < 1).all() and (out["var"] >= 0).all() and (out["lpd"] < 0).all()
    no_y = s.posterior_predictive(prod, {"X": feed["X"]})
    assert sorted(no_y) == ["mean", "var"] and np.array_equal(no_y["mean"], out["mean"]) and np.array_equal(no_y["var"], out["var"])
    # the network, from a float64 sampler: the summary is taken of the fp32 copy
    s64 = _sampler(20, BNN_VARS, torch.float64)
    bnn = BnnPredict(1, H, BnnScore.columns(s64._access))
    f2 = _feed(20, 1, cuda)
    out = s64.posterior_predictive(bnn, f2)
    mean, var, lpd = bnn.summary(s64.theta_matrix.float(), f2)
    for k, t in (("mean", mean), ("var", var), ("lpd", lpd)):
        assert np.array_equal(out[k].view(np.int32), t.cpu().numpy().view(np.int32)), k
    pred = s64.function_posterior(bnn, f2).astype(np.float64)
    assert np.allclose(out["mean"], pred.mean(0), rtol=1e-5, atol=1e-6) and np.allclose(out["var"], pred.var(0), rtol=1e-4, atol=1e-7)


def test_argument_errors_are_value_errors(cuda):
    s = _sampler(8, GLM_VARS)
    feed = _feed(10, F, cuda)
    with pytest.raises(ValueError):
        GlmPredict("probit", F)
    with pytest.raises(ValueError):
        GlmPredict("linear", F, output="logit")
    with pytest.raises(ValueError):
        BnnPredict(1, H, (0, 1, 2, 3, 4, 5), output="nope")
    prod = GlmPredict("logistic", F, w_col=1)
    with pytest.raises(ValueError):
        prod(s.theta_matrix, {"X": feed["X"][:, :3].contiguous()})              # X of the wrong width
    with pytest.raises(ValueError):
        prod(s.theta_matrix.double(), feed)                                       # not float32
    with pytest.raises(ValueError):
        prod(s.theta_matrix.cpu(), feed)                                          # not on the device
    with pytest.raises(ValueError):
        prod.summary(s.theta_matrix, {"X": feed["X"]}, lpd=True)                  # lpd without y
    with pytest.raises(ValueError):
        prod.summary(s.theta_matrix, {"X": feed["X"], "y": feed["y"][:4].contiguous()})
    with pytest.raises(ValueError):
        GlmPredict("logistic", F, w_col=5)(s.theta_matrix, feed)                  # the weights run past d (from the library)
    with pytest.raises(ValueError):
        GlmPredict("linear", F, w_col=1, noise_precision=0.0).summary(s.theta_matrix, feed)
    with pytest.raises(ValueError):
        BnnPredict(1, H, (0, 5, 9, 12, 13, 14))(_sampler(4, BNN_VARS).theta_matrix, _feed(5, 1, cuda))   # overlapping blocks
    with pytest.raises(ValueError):
        s.posterior_predictive(logits, feed)                                      # not a producer


def test_a_sharded_sampler_refuses_posterior_predictive(cuda):
    s = _sampler(8, GLM_VARS)
    s._group = object()                                     # stands for a process group: the check precedes any collective
    with pytest.raises(ValueError, match="one rank"):
        s.posterior_predictive(GlmPredict("logistic", F, w_col=1), _feed(10, F, cuda))


def test_other_callables_still_get_the_dict_of_views(cuda):
    s = _sampler(8, GLM_VARS)
    seen = {}

    def func(th, feed):
        seen["arg"] = th
        return th["model/w:0"][:, :, 0]
    out = s.function_posterior(func, None)
    assert isinstance(seen["arg"], dict) and sorted(seen["arg"]) == sorted(GLM_VARS) and out.shape == (8, F)
    assert torch.equal(seen["arg"]["model/w:0"][:, :, 0], s.theta_matrix[:, 1:])

    class Flagged:
        wants_matrix = False

        def __call__(self, th, feed):
            seen["flagged"] = th
            return th["model/log_alpha:0"]
    s.function_posterior(Flagged(), None)
    assert isinstance(seen["flagged"], dict)
    bare = _sampler(8, GLM_VARS, bare=True)
    bare.function_posterior(lambda th, feed: seen.__setitem__("bare", th) or th, None)
    assert seen["bare"] is bare.theta_matrix
