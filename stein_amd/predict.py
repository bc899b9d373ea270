"""Posterior predictive producers on the device: the forward pass of every particle in one launch.

The reference's examples end in ``function_posterior`` with a callable of the model and average what comes back
(examples/logistic_regression/main.py:52-61, regression_neural_network/main.py:100-106).  For the three models the score
producers cover (stein_amd/scores.py) the forward pass has a closed form; ``GlmPredict`` / ``BnnPredict`` evaluate it with
hand-written HIP kernels (csrc/stein_predict.hip) in two forms:

* ``producer(theta_matrix, feed)`` -> the [n, batch] outputs, a device tensor: a valid ``function_posterior`` callable;
* ``producer.summary(theta_matrix, feed)`` -> (mean, var, lpd) per test point, device tensors of [batch]: the ensemble
  mean and variance of the outputs and the log predictive density log(1/n sum_p p(y_b | theta_p)), without ever
  materialising [n, batch].  ``SteinSampler.posterior_predictive`` hands these back as NumPy;
* ``producer.weighted_summary(theta_matrix, feed, weights)`` -> (mean, var, lpd, ess): the same summaries under per-particle
  weights -- ``sampler.importance_weights(...)`` or the counts of ``sampler.thin(...)`` -- and the weights' effective sample
  size (``posterior_predictive(..., weights=w)``).
"""
import ctypes

import torch

from . import _lib

_OUTPUTS = {"link": _lib.PRED_LINK, "mean": _lib.PRED_MEAN}


def _device_f32(name, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 device tensor" % name)


class _Predict:
    """What the two producers share: argument checks, the workspace each object holds and regrows, the two call forms."""
    wants_matrix = True   # function_posterior hands this callable the packed [n, d] matrix, not the dict of views

    def __init__(self, output, width):
        if output not in _OUTPUTS:
            raise ValueError("output must be 'link' or 'mean'")
        self.output = _OUTPUTS[output]
        self._width = int(width)      # columns of feed["X"]
        self._ws = None
        self._wws = None              # the workspace of weighted_summary: the weight pass's sums ahead of the states

    def _workspace(self, n, batch, device):
        need = _lib.predict_workspace_bytes(n, batch)
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def _inputs(self, theta, feed, want_y):
        X = feed["X"]
        y = feed.get("y") if want_y else None
        _device_f32("theta", theta)
        _device_f32("X", X)
        if theta.dim() != 2:
            raise ValueError("theta must be the packed [n, d] particle matrix")
        batch = X.shape[0]
        if X.shape != (batch, self._width):
            raise ValueError("X must be [batch, %d]" % self._width)
        if want_y:
            if y is None:
                raise ValueError("the log predictive density needs feed['y']")
            _device_f32("y", y)
            if y.numel() != batch:
                raise ValueError("y must be [batch]")
        return X, y, batch

    def __call__(self, theta, feed, out=None):
        """-> [n, batch] float32 device tensor of the outputs f_pb (written into `out` when given)."""
        X, _, batch = self._inputs(theta, feed, False)
        n = theta.shape[0]
        if out is None:
            out = torch.empty(n, batch, dtype=torch.float32, device=theta.device)
        else:
            _device_f32("out", out)
            if out.shape != (n, batch):
                raise ValueError("out must be [%d, %d]" % (n, batch))
        self._launch(theta, X, None, batch, out, None, None, None, None)
        return out

    def summary(self, theta, feed, lpd=None):
        """-> (mean, var, lpd or None), float32 device tensors of [batch]; lpd=None: computed when `feed` has a "y"."""
        if lpd is None:
            lpd = feed.get("y") is not None
        X, y, batch = self._inputs(theta, feed, bool(lpd))
        mean = torch.empty(batch, dtype=torch.float32, device=theta.device)
        var = torch.empty_like(mean)
        out_lpd = torch.empty_like(mean) if lpd else None
        self._launch(theta, X, y, batch, None, mean, var, out_lpd, self._workspace(theta.shape[0], batch, theta.device))
        return mean, var, out_lpd

    def weighted_summary(self, theta, feed, weights, lpd=None):
        """-> (mean, var, lpd or None, ess) under per-particle weights w_p >= 0 (Stein importance weights, or the counts
        ``torch.bincount(idx, minlength=n)`` of a thinned sample; they need not sum to 1): mean_b = sum_p w_p f_pb / W and
        so on, ess = W^2 / sum_p w_p^2 as a 1-element float64 device tensor.  `weights`: any real-valued [n] tensor or
        NumPy array; it is moved to the particles' device as contiguous float64 and never read on the host, so a negative
        or non-finite weight (or W = 0) shows as NaN in every result."""
        if lpd is None:
            lpd = feed.get("y") is not None
        X, y, batch = self._inputs(theta, feed, bool(lpd))
        n = theta.shape[0]
        w = torch.as_tensor(weights)
        if w.dtype == torch.bool or w.is_complex():
            raise ValueError("weights must be real-valued, not %s" % w.dtype)
        if w.dim() != 1 or w.shape[0] != n:
            raise ValueError("weights must be [%d], one per particle" % n)
        w = w.to(device=theta.device, dtype=torch.float64).contiguous()
        mean = torch.empty(batch, dtype=torch.float32, device=theta.device)
        var = torch.empty_like(mean)
        out_lpd = torch.empty_like(mean) if lpd else None
        ess = torch.empty(1, dtype=torch.float64, device=theta.device)
        need = _lib.predict_weighted_workspace_bytes(n, batch)
        if self._wws is None or self._wws.device != theta.device or self._wws.numel() < need:
            self._wws = torch.empty(need, dtype=torch.uint8, device=theta.device)
        self._launch(theta, X, y, batch, None, mean, var, out_lpd, self._wws, weights=w, ess=ess)
        return mean, var, out_lpd, ess

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()


class GlmPredict(_Predict):
    """Outputs of the generalised linear models of GlmScore: z = X w per particle.

    kind            : "linear" or "logistic"
    n_feats, w_col  : as for GlmScore (the weights' width and first packed column)
    output          : "link" -> z (logits / regression mean: what the reference's examples average);
                      "mean" -> sigmoid(z) for the logistic model, z otherwise
    noise_precision : tau of the linear model's likelihood N(y; z, 1/tau), read by the log predictive density only
    """

    def __init__(self, kind, n_feats, w_col=0, output="link", noise_precision=1.0):
        if kind not in ("linear", "logistic"):
            raise ValueError("kind must be 'linear' or 'logistic'")
        super().__init__(output, n_feats)
        self.kind = _lib.GLM_LINEAR if kind == "linear" else _lib.GLM_LOGISTIC
        self.n_feats, self.w_col = int(n_feats), int(w_col)
        self.noise_precision = float(noise_precision)

    def _launch(self, theta, X, y, batch, pred, mean, var, lpd, ws, weights=None, ess=None):
        n, d = theta.shape
        name, w, e = ("stein_predict_glm", (), ()) if weights is None else \
            ("stein_predict_glm_weighted", (weights.data_ptr(),), (ess.data_ptr(),))
        _lib.call_on(theta.device, name, theta.data_ptr(), n, d, self.kind, self.output, self.w_col, self.n_feats,
                     X.data_ptr(), self._ptr(y), batch, self.noise_precision, *w, self._ptr(pred), self._ptr(mean),
                     self._ptr(var), self._ptr(lpd), *e, self._ptr(ws), 0 if ws is None else ws.numel(),
                     torch.cuda.current_stream(theta.device).cuda_stream)


class BnnPredict(_Predict):
    """Outputs of the one-hidden-layer network of BnnScore: relu(X w1 + b1) w2 + b2 per particle.

    cols: first column of (w1, b1, w2, b2, log_lambda, log_gamma) in the packed particle matrix, as for BnnScore
    (``BnnScore.columns(sampler._access)``).  output: "link" and "mean" are the same for this model.
    """
    def __init__(self, n_in, n_hidden, cols, output="link"):
        super().__init__(output, n_in)
        self.n_in, self.n_hidden = int(n_in), int(n_hidden)
        self._cols = (ctypes.c_int64 * 6)(*[int(c) for c in cols])

    def _launch(self, theta, X, y, batch, pred, mean, var, lpd, ws, weights=None, ess=None):
        n, d = theta.shape
        name, w, e = ("stein_predict_bnn", (), ()) if weights is None else \
            ("stein_predict_bnn_weighted", (weights.data_ptr(),), (ess.data_ptr(),))
        _lib.call_on(theta.device, name, theta.data_ptr(), n, d, self.n_in, self.n_hidden, self._cols, self.output,
                     X.data_ptr(), self._ptr(y), batch, *w, self._ptr(pred), self._ptr(mean), self._ptr(var), self._ptr(lpd),
                     *e, self._ptr(ws), 0 if ws is None else ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)
