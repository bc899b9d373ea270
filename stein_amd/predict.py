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
  size (``posterior_predictive(..., weights=w)``);
* ``producer.order_statistics(theta_matrix, feed, ranks)`` / ``producer.quantiles(theta_matrix, feed, q)`` -> [len, batch]:
  exact order statistics of the outputs over the particles per test point -- the ensemble median, credible bands -- again
  without [n, batch] (``posterior_predictive(..., quantiles=(0.05, 0.5, 0.95))``);
* ``producer.weighted_quantiles(theta_matrix, feed, weights, q)`` -> [len(q), batch]: the band under importance weights or
  of a thinned multiset (counts), by the inverted weighted distribution function -- an element of the ensemble, not
  interpolated (``sampler.predictive_quantiles(producer, feed, q, weights=w)``);
* ``producer.y_cdf(theta_matrix, feed, t)`` / ``producer.y_quantiles(theta_matrix, feed, q)``: the predictive distribution of
  y itself, observation noise included -- the Gaussian mixture over the particles, evaluated at points (``t=None``: at
  ``feed["y"]``, the probability integral transform) and inverted at levels (predictive intervals), with or without weights
  (csrc/stein_predict_y.hip; ``sampler.predictive_cdf`` / ``sampler.predictive_interval``).  Regression models only.

``SoftmaxPredict`` (csrc/stein_predict_softmax.hip) is the producer of the softmax regression model of
``stein_amd.scores.SoftmaxScore``: a vector of class probabilities per test point, so ``producer(theta_matrix, feed)`` is
[n, batch, C] and its summaries -- class probabilities, label, expected entropy, log predictive density -- come from
``producer.summary`` / ``sampler.predictive_classes``, under per-particle weights from ``producer.weighted_summary`` /
``sampler.predictive_classes(..., weights=w)``; the other scalar-output methods above refuse it.  ``BnnClassPredict``
(csrc/stein_predict_bnn_class.hip) is the same producer for the network classifier of ``stein_amd.scores.BnnClassScore``.
"""
import ctypes
import math

import torch

from . import _lib

_OUTPUTS = {"link": _lib.PRED_LINK, "mean": _lib.PRED_MEAN}


def _device_f32(name, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 device tensor" % name)


def _labels_i32(y, batch, device):
    """feed["y"] of the softmax model: any integer-dtype tensor of [batch] -> contiguous int32 on `device` (never read on
    the host: a label outside [0, n_classes) shows as NaN in the results)"""
    if not isinstance(y, torch.Tensor):
        y = torch.as_tensor(y)
    if y.dtype.is_floating_point or y.is_complex() or y.dtype == torch.bool:
        raise ValueError("y must hold integer class indices (an integer dtype), not %s" % y.dtype)
    if y.numel() != batch:
        raise ValueError("y must be [batch]")
    return y.reshape(batch).to(device=device, dtype=torch.int32).contiguous()


class _Buffers:
    """What every producer holds: cached device buffers that regrow, and pointers of optional tensors."""
    wants_matrix = True   # function_posterior hands this callable the packed [n, d] matrix, not the dict of views

    def _buffer(self, name, need, device, dtype=torch.uint8):
        """the cached buffer self.<name>, regrown when it is missing, on another device or too small"""
        buf = getattr(self, name)
        if buf is None or buf.device != device or buf.numel() < need:
            buf = torch.empty(need, dtype=dtype, device=device)
            setattr(self, name, buf)
        return buf

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()


class _Predict(_Buffers):
    """What the two producers share: argument checks, the workspace each object holds and regrows, the two call forms."""

    def __init__(self, output, width):
        if output not in _OUTPUTS:
            raise ValueError("output must be 'link' or 'mean'")
        self.output = _OUTPUTS[output]
        self._width = int(width)      # columns of feed["X"]
        self._ws = None
        self._wws = None              # the workspace of weighted_summary: the weight pass's sums ahead of the states
        self._rws = None              # the workspace of order_statistics: 76 bytes per (row, rank of one call)
        self._masses = self._mass_info = None   # weighted_quantiles: the particles' integer masses and their total
        self._mws = self._wrws = None           # ... the workspaces of the masses pass and of the weighted select
        self._ycws = self._yqws = None          # the workspaces of y_cdf and y_quantiles

    @staticmethod
    def _weights(weights, n, device, want_mode=False):
        """-> `weights` as a contiguous float64 [n] tensor on `device`; want_mode: and how weighted_quantiles takes them,
        an integer dtype as counts, a float dtype as weights to normalise (noted before the conversion)"""
        w = torch.as_tensor(weights)
        if w.dtype == torch.bool or w.is_complex():
            raise ValueError("weights must be real-valued, not %s" % w.dtype)
        if w.dim() != 1 or w.shape[0] != n:
            raise ValueError("weights must be [%d], one per particle" % n)
        mode = _lib.MASS_NORMALISED if w.dtype.is_floating_point else _lib.MASS_COUNTS
        w = w.to(device=device, dtype=torch.float64).contiguous()
        return (w, mode) if want_mode else w

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
        ws = self._buffer("_ws", _lib.predict_workspace_bytes(theta.shape[0], batch), theta.device)
        self._launch(theta, X, y, batch, None, mean, var, out_lpd, ws)
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
        w = self._weights(weights, n, theta.device)
        mean = torch.empty(batch, dtype=torch.float32, device=theta.device)
        var = torch.empty_like(mean)
        out_lpd = torch.empty_like(mean) if lpd else None
        ess = torch.empty(1, dtype=torch.float64, device=theta.device)
        ws = self._buffer("_wws", _lib.predict_weighted_workspace_bytes(n, batch), theta.device)
        self._launch(theta, X, y, batch, None, mean, var, out_lpd, ws, weights=w, ess=ess)
        return mean, var, out_lpd, ess

    def order_statistics(self, theta, feed, ranks):
        """-> [len(ranks), batch] float32 device tensor: row i holds, per test point, the ranks[i]-th smallest (0-based) of
        the n outputs f_pb -- exactly the entry ``torch.sort(self(theta, feed), dim=0)`` has there (NaNs last), found by a
        radix select that recomputes the forward pass and never forms [n, batch].  `ranks`: integers in [0, n), in any
        order, repeats allowed; eight go into one call of the library, more are split over several calls."""
        X, _, batch = self._inputs(theta, feed, False)
        n = theta.shape[0]
        ranks = [int(r) for r in ranks]
        if not ranks:
            raise ValueError("ranks must not be empty")
        for r in ranks:
            if not 0 <= r < n:
                raise ValueError("rank %d is outside [0, %d)" % (r, n))
        out = torch.empty(len(ranks), batch, dtype=torch.float32, device=theta.device)
        ws = self._buffer("_rws", _lib.predict_ranks_workspace_bytes(n, batch, min(len(ranks), _lib.PRED_RANKS_MAX)),
                          theta.device)
        for at in range(0, len(ranks), _lib.PRED_RANKS_MAX):
            part = ranks[at:at + _lib.PRED_RANKS_MAX]
            self._launch_ranks(theta, X, batch, (ctypes.c_int64 * len(part))(*part), len(part), out[at:at + len(part)],
                               ws)
        return out

    def quantiles(self, theta, feed, q, interpolation="linear"):
        """-> [len(q), batch] float32 device tensor: the q-quantiles of the n outputs per test point by NumPy's definition,
        position q (n - 1) among the sorted outputs.  "linear": lo + (hi - lo) frac of the two neighbouring order statistics,
        in fp32 on the device (a position that is an integer gives that order statistic itself); "lower" / "higher": the
        neighbour below / above, exact.  Built on ``order_statistics``: no [n, batch] matrix."""
        if interpolation not in ("linear", "lower", "higher"):
            raise ValueError("interpolation must be 'linear', 'lower' or 'higher'")
        q = [float(v) for v in q]
        if not q:
            raise ValueError("q must not be empty")
        n = theta.shape[0]
        ranks, plan = [], []
        for v in q:
            if not 0.0 <= v <= 1.0:       # NaN too
                raise ValueError("quantiles must lie in [0, 1], not %r" % v)
            pos = v * (n - 1)
            lo = min(int(math.floor(pos)), n - 1)
            frac = pos - lo
            hi = lo + 1 if frac > 0.0 else lo
            if interpolation == "lower":
                hi, frac = lo, 0.0
            elif interpolation == "higher":
                lo, frac = hi, 0.0
            for r in (lo, hi):
                if r not in ranks:
                    ranks.append(r)
            plan.append((ranks.index(lo), ranks.index(hi), frac))
        stats = self.order_statistics(theta, feed, ranks)
        out = torch.empty(len(q), stats.shape[1], dtype=torch.float32, device=stats.device)
        for i, (lo, hi, frac) in enumerate(plan):
            if frac == 0.0:
                out[i] = stats[lo]
            else:
                out[i] = stats[lo] + (stats[hi] - stats[lo]) * frac
        return out

    def weighted_quantiles(self, theta, feed, weights, q):
        """-> [len(q), batch] float32 device tensor: the q-quantiles of the outputs per test point under per-particle
        weights, by the inverted weighted distribution function (NumPy's ``method="inverted_cdf"`` with weights): the
        smallest output at which the cumulative weight reaches q of the total.  Always an element of the ensemble, never
        an interpolation -- a different definition from ``quantiles``' "linear".  `weights` [n], validated as for
        ``weighted_summary`` and never read on the host.  An integer dtype -- ``torch.bincount(sampler.thin(m),
        minlength=n)`` -- is taken as counts: the result is exactly the order statistic ceil(q M) - 1 (0 for q = 0) of the
        multiset with M = sum of the counts elements.  Any float dtype is normalised on the device to integer masses
        rint(w_p / W 2^31), so the cumulative probabilities are exact to (n / 2 + 1) / 2^31.  A particle of weight zero
        is skipped; bad weights (negative, non-finite, all zero, a count sum of 2^32 or more) give NaN rows.  No
        [n, batch] matrix: a weighted radix select that recomputes the forward pass; eight levels go into one call of the
        library, more are split."""
        X, _, batch = self._inputs(theta, feed, False)
        n = theta.shape[0]
        w, mode = self._weights(weights, n, theta.device, want_mode=True)
        q = [float(v) for v in q]
        if not q:
            raise ValueError("q must not be empty")
        for v in q:
            if not 0.0 <= v <= 1.0:       # NaN too
                raise ValueError("quantiles must lie in [0, 1], not %r" % v)
        dev = theta.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        masses = self._buffer("_masses", n, dev, torch.int32)                 # the uint32 masses, as bytes
        info = self._buffer("_mass_info", 2, dev, torch.float64)
        mws = self._buffer("_mws", _lib.predict_rank_masses_workspace_bytes(n), dev)
        _lib.call_on(dev, "stein_predict_rank_masses", w.data_ptr(), n, mode, masses.data_ptr(), info.data_ptr(),
                     mws.data_ptr(), mws.numel(), stream)
        ws = self._buffer("_wrws", _lib.predict_ranks_weighted_workspace_bytes(n, batch, min(len(q), _lib.PRED_RANKS_MAX)),
                          dev)
        out = torch.empty(len(q), batch, dtype=torch.float32, device=dev)
        for at in range(0, len(q), _lib.PRED_RANKS_MAX):
            part = q[at:at + _lib.PRED_RANKS_MAX]
            self._launch_wranks(theta, X, batch, masses, (ctypes.c_double * len(part))(*part), len(part),
                                out[at:at + len(part)], ws)
        return out

    def _check_y_model(self):
        """y_cdf / y_quantiles: the models with a Gaussian y (GlmPredict overrides this for the logistic kind)"""

    def y_cdf(self, theta, feed, t=None, weights=None):
        """-> F_b(t) = sum_p w_p Phi((t - z_pb) sqrt(tau_p)) / W, the predictive distribution function of y_b -- the mixture
        over the particles of the model's Gaussian likelihood, tau the noise precision (``noise_precision`` for the linear
        model, each particle's exp(log_gamma) for the network).  `t`: a float32 device tensor of [n_pts, batch] or [batch],
        any n_pts (eight go into one call of the library) -> float32 [n_pts, batch]; ``t=None`` takes ``feed["y"]`` and
        returns [batch], the probability integral transform of the rows: uniform on (0, 1) for a calibrated model.
        `weights`: None (every particle counts alike) or [n] as for ``weighted_summary``; never read on the host, bad
        weights give NaN rows.  No [n, batch] matrix."""
        self._check_y_model()
        pit = t is None
        X, y, batch = self._inputs(theta, feed, pit)
        if pit:
            t = y.reshape(1, batch)
        else:
            _device_f32("t", t)
            if t.dim() == 1:
                t = t.reshape(1, -1)
            if t.dim() != 2 or t.shape[1] != batch or t.shape[0] < 1:
                raise ValueError("t must be [n_pts, %d] or [%d]" % (batch, batch))
        n, dev = theta.shape[0], theta.device
        w = None if weights is None else self._weights(weights, n, dev)
        n_pts = t.shape[0]
        out = torch.empty(n_pts, batch, dtype=torch.float32, device=dev)
        ws = self._buffer("_ycws", _lib.predict_ycdf_workspace_bytes(n, batch, min(n_pts, _lib.PRED_Y_POINTS_MAX)), dev)
        for at in range(0, n_pts, _lib.PRED_Y_POINTS_MAX):
            m = min(_lib.PRED_Y_POINTS_MAX, n_pts - at)
            self._launch_ycdf(theta, X, batch, t[at:at + m], m, w, out[at:at + m], ws)
        return out[0] if pit else out

    def y_quantiles(self, theta, feed, q, weights=None, passes=8, return_bracket=False):
        """-> [len(q), batch] float32 device tensor: the q-quantiles of the predictive distribution of y per test point --
        ``y_quantiles(theta, feed, (0.05, 0.95))`` is the 90 % predictive interval, noise included.  q strictly inside
        (0, 1).  A bracketed search on the device: one pass brackets every quantile between the least and the largest
        component quantile, then `passes` (1 .. 12) passes cut each bracket to an eighth; 8 reach neighbouring floats.  The
        result is the bracket's upper end; ``return_bracket=True`` -> (lower ends, upper ends): the distribution function as
        the device evaluates it is below q at the lower end and at least q at the upper.  `weights` as for ``y_cdf``.  Eight
        levels go into one call of the library, more are split.  No [n, batch] matrix."""
        self._check_y_model()
        X, _, batch = self._inputs(theta, feed, False)
        q = [float(v) for v in q]
        if not q:
            raise ValueError("q must not be empty")
        for v in q:
            if not 0.0 < v < 1.0:         # NaN too
                raise ValueError("quantiles of y must lie strictly inside (0, 1), not %r" % v)
        passes = int(passes)
        if not 1 <= passes <= _lib.PRED_Y_PASSES_MAX:
            raise ValueError("passes must lie in [1, %d]" % _lib.PRED_Y_PASSES_MAX)
        n, dev = theta.shape[0], theta.device
        w = None if weights is None else self._weights(weights, n, dev)
        hi = torch.empty(len(q), batch, dtype=torch.float32, device=dev)
        lo = torch.empty_like(hi) if return_bracket else None
        ws = self._buffer("_yqws", _lib.predict_yquantiles_workspace_bytes(n, batch, min(len(q), _lib.PRED_RANKS_MAX)), dev)
        for at in range(0, len(q), _lib.PRED_RANKS_MAX):
            part = q[at:at + _lib.PRED_RANKS_MAX]
            self._launch_yquantiles(theta, X, batch, (ctypes.c_double * len(part))(*part), len(part), passes, w,
                                    hi[at:at + len(part)], None if lo is None else lo[at:at + len(part)], ws)
        return (lo, hi) if return_bracket else hi


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

    def _launch_ranks(self, theta, X, batch, ranks, n_ranks, out, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_glm_ranks", theta.data_ptr(), n, d, self.kind, self.output, self.w_col,
                     self.n_feats, X.data_ptr(), batch, ranks, n_ranks, out.data_ptr(), ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream(theta.device).cuda_stream)

    def _launch_wranks(self, theta, X, batch, masses, levels, n_levels, out, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_glm_ranks_weighted", theta.data_ptr(), n, d, self.kind, self.output,
                     self.w_col, self.n_feats, X.data_ptr(), batch, masses.data_ptr(), levels, n_levels, out.data_ptr(),
                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)

    def _check_y_model(self):
        if self.kind != _lib.GLM_LINEAR:
            raise ValueError("y of the logistic model is Bernoulli, not Gaussian: its predictive probability is the mean of "
                             "the outputs of GlmPredict(..., output=\"mean\")")

    def _launch_ycdf(self, theta, X, batch, t, n_pts, weights, out, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_glm_ycdf", theta.data_ptr(), n, d, self.kind, self.w_col, self.n_feats,
                     X.data_ptr(), batch, self.noise_precision, t.data_ptr(), n_pts, self._ptr(weights), out.data_ptr(),
                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)

    def _launch_yquantiles(self, theta, X, batch, levels, n_levels, passes, weights, out, out_lo, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_glm_yquantiles", theta.data_ptr(), n, d, self.kind, self.w_col,
                     self.n_feats, X.data_ptr(), batch, self.noise_precision, levels, n_levels, passes, self._ptr(weights),
                     out.data_ptr(), self._ptr(out_lo), ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream(theta.device).cuda_stream)


class BnnPredict(_Predict):
    """Outputs of the one-hidden-layer network of BnnScore: relu(X w1 + b1) w2 + b2 per particle.

    cols: first column of (w1, b1, w2, b2, log_lambda, log_gamma) in the packed particle matrix, as for BnnScore
    (``BnnScore.columns(sampler._access)``).  output: "link" and "mean" are the same for this model.

    More than NARROW_MAX = 4 input features (up to 128, n_in * n_hidden <= 16384) take the library's wide kernels
    (stein_predict_bnn_wide): the outputs, ``summary`` and ``weighted_summary`` -- so ``function_posterior`` and
    ``posterior_predictive(..., weights=)`` -- work as for a narrow network; ``quantiles``, ``order_statistics``,
    ``weighted_quantiles``, ``y_cdf`` and ``y_quantiles`` are built for n_in <= 4 only and raise a ValueError.
    """
    NARROW_MAX = 4

    def __init__(self, n_in, n_hidden, cols, output="link"):
        super().__init__(output, n_in)
        self.n_in, self.n_hidden = int(n_in), int(n_hidden)
        self._cols = (ctypes.c_int64 * 6)(*[int(c) for c in cols])

    def _narrow_only(self, what):
        if self.n_in > self.NARROW_MAX:
            raise ValueError("%s is built for n_in <= %d only (this producer has n_in = %d): take the [n, batch] outputs "
                             "through function_posterior and sort or integrate them there" % (what, self.NARROW_MAX, self.n_in))

    def order_statistics(self, theta, feed, ranks):
        self._narrow_only("order_statistics")
        return super().order_statistics(theta, feed, ranks)

    def quantiles(self, theta, feed, q, interpolation="linear"):
        self._narrow_only("quantiles")
        return super().quantiles(theta, feed, q, interpolation)

    def weighted_quantiles(self, theta, feed, weights, q):
        self._narrow_only("weighted_quantiles")
        return super().weighted_quantiles(theta, feed, weights, q)

    def y_cdf(self, theta, feed, t=None, weights=None):
        self._narrow_only("y_cdf")
        return super().y_cdf(theta, feed, t, weights)

    def y_quantiles(self, theta, feed, q, weights=None, passes=8, return_bracket=False):
        self._narrow_only("y_quantiles")
        return super().y_quantiles(theta, feed, q, weights, passes, return_bracket)

    def _launch(self, theta, X, y, batch, pred, mean, var, lpd, ws, weights=None, ess=None):
        n, d = theta.shape
        name, w, e = ("stein_predict_bnn", (), ()) if weights is None else \
            ("stein_predict_bnn_weighted", (weights.data_ptr(),), (ess.data_ptr(),))
        if self.n_in > self.NARROW_MAX:      # (up to four features the old names: no existing path changes)
            name = name.replace("stein_predict_bnn", "stein_predict_bnn_wide")
        _lib.call_on(theta.device, name, theta.data_ptr(), n, d, self.n_in, self.n_hidden, self._cols, self.output,
                     X.data_ptr(), self._ptr(y), batch, *w, self._ptr(pred), self._ptr(mean), self._ptr(var), self._ptr(lpd),
                     *e, self._ptr(ws), 0 if ws is None else ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)

    def _launch_ranks(self, theta, X, batch, ranks, n_ranks, out, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_bnn_ranks", theta.data_ptr(), n, d, self.n_in, self.n_hidden, self._cols,
                     self.output, X.data_ptr(), batch, ranks, n_ranks, out.data_ptr(), ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream(theta.device).cuda_stream)

    def _launch_wranks(self, theta, X, batch, masses, levels, n_levels, out, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_bnn_ranks_weighted", theta.data_ptr(), n, d, self.n_in, self.n_hidden,
                     self._cols, self.output, X.data_ptr(), batch, masses.data_ptr(), levels, n_levels, out.data_ptr(),
                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)

    def _launch_ycdf(self, theta, X, batch, t, n_pts, weights, out, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_bnn_ycdf", theta.data_ptr(), n, d, self.n_in, self.n_hidden, self._cols,
                     X.data_ptr(), batch, t.data_ptr(), n_pts, self._ptr(weights), out.data_ptr(), ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream(theta.device).cuda_stream)

    def _launch_yquantiles(self, theta, X, batch, levels, n_levels, passes, weights, out, out_lo, ws):
        n, d = theta.shape
        _lib.call_on(theta.device, "stein_predict_bnn_yquantiles", theta.data_ptr(), n, d, self.n_in, self.n_hidden,
                     self._cols, X.data_ptr(), batch, levels, n_levels, passes, self._ptr(weights), out.data_ptr(),
                     self._ptr(out_lo), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)


class SoftmaxPredict(_Buffers):
    """Class probabilities of the softmax regression model of SoftmaxScore: softmax(X W) per particle
    (csrc/stein_predict_softmax.hip).

    n_feats, n_classes, w_col : as for SoftmaxScore (W [n_feats, n_classes] row-major at w_col)
    output                    : "mean" -> the probabilities p_pbc; "link" -> the logits z_pbc

    ``producer(theta_matrix, feed)`` -> [n, batch, n_classes], a valid ``function_posterior`` callable
    (``sampler.function_posterior`` flattens every callable's result per particle, so it hands back NumPy [n, batch * C]:
    reshape it to (n, batch, C));
    ``producer.summary(theta_matrix, feed)`` -> {"prob" [batch, C], "label" [batch] int32, "ent" [batch], "lpd" [batch]}:
    the posterior predictive class probabilities mean_p p_pbc, their argmax, the expected entropy mean_p H(p_pb.) and -- only
    when the feed has a "y" -- the log predictive density log(mean_p p_{pb,y_b}); device tensors, no [n, batch, C] formed.
    ``sampler.predictive_classes(producer, feed)`` hands them back as NumPy with the entropy of prob and the mutual
    information.
    ``producer.weighted_summary(theta_matrix, feed, weights)`` -> the same dict under per-particle weights w_p >= 0 (Stein
    importance weights, or the counts of a thinned sample): sum_p w_p (.) / W in the place of every mean, and "ess", the
    weights' effective sample size (``sampler.predictive_classes(producer, feed, weights=w)``).
    The scalar-output methods of GlmPredict / BnnPredict (order statistics, quantiles, the distribution of y) have no
    meaning for a vector of class probabilities and raise a ValueError.
    """
    classes = True    # the samplers' scalar-output methods refuse this producer and name predictive_classes
    _workspace_bytes = staticmethod(_lib.predict_softmax_workspace_bytes)
    _weighted_workspace_bytes = staticmethod(_lib.predict_softmax_weighted_workspace_bytes)
    _weights = staticmethod(_Predict._weights)

    def __init__(self, n_feats, n_classes, w_col=0, output="mean"):
        if output not in _OUTPUTS:
            raise ValueError("output must be 'link' or 'mean'")
        self.output = _OUTPUTS[output]
        self.n_feats, self.n_classes, self.w_col = int(n_feats), int(n_classes), int(w_col)
        self._ws = self._wws = None

    def _inputs(self, theta, feed, want_y):
        X = feed["X"]
        _device_f32("theta", theta)
        _device_f32("X", X)
        if theta.dim() != 2:
            raise ValueError("theta must be the packed [n, d] particle matrix")
        batch = X.shape[0]
        if X.shape != (batch, self.n_feats):
            raise ValueError("X must be [batch, %d]" % self.n_feats)
        y = None
        if want_y:
            y = _labels_i32(feed["y"], batch, theta.device)
        return X, y, batch

    def _launch(self, theta, X, y, batch, pred, prob, lpd, ent, label, ws, weights=None, ess=None):
        n, d = theta.shape
        p = self._ptr
        name, w, e = ("stein_predict_softmax", (), ()) if weights is None else \
            ("stein_predict_softmax_weighted", (weights.data_ptr(),), (ess.data_ptr(),))
        _lib.call_on(theta.device, name, theta.data_ptr(), n, d, self.output, self.w_col, self.n_feats,
                     self.n_classes, X.data_ptr(), p(y), batch, *w, p(pred), p(prob), p(lpd), p(ent), p(label), *e, p(ws),
                     0 if ws is None else ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)

    def __call__(self, theta, feed, out=None):
        """-> [n, batch, n_classes] float32 device tensor (written into `out` when given)."""
        X, _, batch = self._inputs(theta, feed, False)
        n = theta.shape[0]
        if out is None:
            out = torch.empty(n, batch, self.n_classes, dtype=torch.float32, device=theta.device)
        else:
            _device_f32("out", out)
            if out.shape != (n, batch, self.n_classes):
                raise ValueError("out must be [%d, %d, %d]" % (n, batch, self.n_classes))
        self._launch(theta, X, None, batch, out, None, None, None, None, None)
        return out

    def _summary_outputs(self, batch, want_y, dev):
        out = {"prob": torch.empty(batch, self.n_classes, dtype=torch.float32, device=dev),
               "label": torch.empty(batch, dtype=torch.int32, device=dev),
               "ent": torch.empty(batch, dtype=torch.float32, device=dev)}
        if want_y:
            out["lpd"] = torch.empty(batch, dtype=torch.float32, device=dev)
        return out

    def summary(self, theta, feed):
        """-> {"prob", "label", "ent"} and, when `feed` has a "y", "lpd": device tensors (see the class)."""
        want_y = feed.get("y") is not None
        X, y, batch = self._inputs(theta, feed, want_y)
        dev = theta.device
        out = self._summary_outputs(batch, want_y, dev)
        ws = self._buffer("_ws", self._workspace_bytes(theta.shape[0], batch, self.n_classes), dev)
        self._launch(theta, X, y, batch, None, out["prob"], out.get("lpd"), out["ent"], out["label"], ws)
        return out

    def weighted_summary(self, theta, feed, weights):
        """-> {"prob", "label", "ent", "ess"} and, when `feed` has a "y", "lpd", under per-particle weights w_p >= 0 (Stein
        importance weights, or the counts ``torch.bincount(idx, minlength=n)`` of a thinned sample; they need not sum to
        1): prob_bc = sum_p w_p p_pbc / W, ent_b = sum_p w_p H(p_pb.) / W, lpd_b = log(sum_p w_p p_{pb,y_b} / W), label the
        argmax of prob, ess = W^2 / sum_p w_p^2 as a 1-element float64 tensor; all device tensors.  `weights`: any
        real-valued [n] tensor or NumPy array (an integer dtype is taken as counts); it is moved to the particles' device as
        contiguous float64 and never read on the host, so a negative or non-finite weight (or W = 0) shows as NaN in every
        row and in ess, and as the label -1.  Particles of weight zero are not computed: a thinned sample costs about what
        its distinct particles cost."""
        want_y = feed.get("y") is not None
        X, y, batch = self._inputs(theta, feed, want_y)
        n, dev = theta.shape[0], theta.device
        w = self._weights(weights, n, dev)
        out = self._summary_outputs(batch, want_y, dev)
        out["ess"] = torch.empty(1, dtype=torch.float64, device=dev)
        ws = self._buffer("_wws", self._weighted_workspace_bytes(n, batch, self.n_classes), dev)
        self._launch(theta, X, y, batch, None, out["prob"], out.get("lpd"), out["ent"], out["label"], ws, weights=w,
                     ess=out["ess"])
        return out

    def _scalar_only(self, *args, **kw):
        raise ValueError("a %s gives a vector of class probabilities per test point, not a scalar output: its "
                         "summaries come from sampler.predictive_classes(producer, feed) (or producer.summary)"
                         % type(self).__name__)

    order_statistics = quantiles = weighted_quantiles = y_cdf = y_quantiles = _scalar_only


class BnnClassPredict(SoftmaxPredict):
    """Class probabilities of the network classifier of BnnClassScore: softmax(relu(X w1 + b1) w2 + b2) per particle
    (csrc/stein_predict_bnn_class.hip).

    n_in, n_hidden, n_classes, cols : as for BnnClassScore (cols[4], the log_lambda column, is not read and may be left out)
    output                          : "mean" -> the probabilities p_pbc; "link" -> the logits z_pbc

    The call forms, ``summary``'s dict and the refusals of the scalar-output methods are SoftmaxPredict's:
    ``producer(theta_matrix, feed)`` -> [n, batch, n_classes]; ``producer.summary(theta_matrix, feed)`` -> {"prob", "label",
    "ent"} and, with a "y" in the feed, "lpd"; ``producer.weighted_summary(theta_matrix, feed, weights)`` -> the same
    under per-particle weights, with "ess"; ``sampler.predictive_classes(producer, feed, weights=None)`` hands them back as
    NumPy.
    """
    _workspace_bytes = staticmethod(_lib.predict_bnn_class_workspace_bytes)
    _weighted_workspace_bytes = staticmethod(_lib.predict_bnn_class_weighted_workspace_bytes)

    def __init__(self, n_in, n_hidden, n_classes, cols, output="mean"):
        if output not in _OUTPUTS:
            raise ValueError("output must be 'link' or 'mean'")
        self.output = _OUTPUTS[output]
        self.n_in, self.n_hidden, self.n_classes = int(n_in), int(n_hidden), int(n_classes)
        self.n_feats = self.n_in      # the columns of feed["X"], as _inputs checks them
        cols = list(cols)[:4]
        if len(cols) != 4:
            raise ValueError("cols must give the first column of w1, b1, w2 and b2")
        self._cols = (ctypes.c_int64 * 5)(*([int(c) for c in cols] + [-1]))
        self._ws = self._wws = None

    def _launch(self, theta, X, y, batch, pred, prob, lpd, ent, label, ws, weights=None, ess=None):
        n, d = theta.shape
        p = self._ptr
        name, w, e = ("stein_predict_bnn_class", (), ()) if weights is None else \
            ("stein_predict_bnn_class_weighted", (weights.data_ptr(),), (ess.data_ptr(),))
        _lib.call_on(theta.device, name, theta.data_ptr(), n, d, self.output, self.n_in, self.n_hidden,
                     self.n_classes, self._cols, X.data_ptr(), p(y), batch, *w, p(pred), p(prob), p(lpd), p(ent), p(label), *e,
                     p(ws), 0 if ws is None else ws.numel(), torch.cuda.current_stream(theta.device).cuda_stream)
