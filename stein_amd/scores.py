"""Score producers on the device: d log p / d theta for every particle in one launch.

The reference obtains the score matrix with n sequential ``sess.run(grad_log_p)`` calls on a TF1 graph of the
model (stein/samplers/stein_sampler.py:59-68).  For the generalised linear models of its examples the gradient has
a closed form; ``GlmScore`` evaluates it with one hand-written HIP kernel (csrc/stein_score.hip) and plugs into
``SteinSampler(score=...)``.  Other models keep the autograd route of ``SteinSampler.score_matrix``.
"""
import torch

from . import _lib
from .predict import _labels_i32


class GlmScore:
    """score(theta_matrix, feed) -> [n, d] float32 device tensor, feed = {"X": [batch, n_feats], "y": [batch]}.

    kind        : "linear" (examples/linear_regression/main.py:18-31) or "logistic"
                  (examples/logistic_regression/main.py:23-49)
    w_col       : first column of the weights in the packed particle matrix (columns are ordered by sorted variable
                  name, stein/utilities/converters.py:40)
    alpha_col   : column of log(alpha) for the hierarchical prior w ~ N(0, 1/alpha), alpha ~ Gamma(1, gamma_rate);
                  None -> fixed prior precision
    n_train     : the log-likelihood of a batch is scaled by n_train / batch (logistic_regression/main.py:47);
                  None -> no scaling
    """
    wants_matrix = True   # SteinSampler hands this callable the packed [n, d] matrix, not the dict of views

    def __init__(self, kind, n_feats, w_col=0, alpha_col=None, n_train=None, prior_precision=1.0, gamma_rate=0.01):
        if kind not in ("linear", "logistic"):
            raise ValueError("kind must be 'linear' or 'logistic'")
        self.kind = _lib.GLM_LINEAR if kind == "linear" else _lib.GLM_LOGISTIC
        self.n_feats, self.w_col = int(n_feats), int(w_col)
        self.alpha_col = -1 if alpha_col is None else int(alpha_col)
        self.n_train = n_train
        self.prior_precision, self.gamma_rate = float(prior_precision), float(gamma_rate)

    def __call__(self, theta, feed, out=None):
        X, y = feed["X"], feed["y"]
        for name, t in (("theta", theta), ("X", X), ("y", y)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
        n, d = theta.shape
        batch = X.shape[0]
        if X.shape != (batch, self.n_feats) or y.numel() != batch:
            raise ValueError("X must be [batch, %d] and y [batch]" % self.n_feats)
        if out is None:
            out = torch.empty_like(theta)
        scale = 1.0 if self.n_train is None else float(self.n_train) / batch
        _lib.call_on(theta.device, "stein_score_glm", theta.data_ptr(), n, d, self.kind, self.w_col, self.n_feats, self.alpha_col,
                  X.data_ptr(), y.data_ptr(), batch, scale, self.prior_precision, self.gamma_rate, out.data_ptr(),
                  torch.cuda.current_stream(theta.device).cuda_stream)
        return out


class BnnScore:
    """Score of the one-hidden-layer Bayesian neural-network regression model of
    examples/regression_neural_network/main.py:29-85 (ReLU, Gamma(a, b) priors on the weight precision lambda and the
    noise precision gamma, both sampled in log space), for every particle in one launch.

    cols: first column of (w1, b1, w2, b2, log_lambda, log_gamma) in the packed particle matrix -- use
    ``BnnScore.columns(sampler)`` for a SteinSampler built with the variable names of the example.

    Up to four input features run stein_score_bnn; 5 .. 128 (n_in * n_hidden <= 16384: the tabular regression sets) run
    stein_score_bnn_wide, which keeps a particle's first layer and its gradient in LDS (csrc/stein_score_wide.hip).
    """
    wants_matrix = True
    NAMES = ("model/w_1:0", "model/b_1:0", "model/w_2:0", "model/b_2:0", "model/log_lambda:0", "model/log_gamma:0")

    def __init__(self, n_in, n_hidden, cols, n_train, gamma_a=1.0, gamma_b=0.01):
        import ctypes
        self.n_in, self.n_hidden, self.n_train = int(n_in), int(n_hidden), float(n_train)
        self.gamma_a, self.gamma_b = float(gamma_a), float(gamma_b)
        self._cols = (ctypes.c_int64 * 6)(*[int(c) for c in cols])

    @staticmethod
    def columns(access, names=NAMES):
        """first packed column of each parameter block from a sampler's access map {name: (start, end)}"""
        return tuple(access[k][0] for k in names)

    def __call__(self, theta, feed, out=None):
        X, y = feed["X"], feed["y"]
        for name, t in (("theta", theta), ("X", X), ("y", y)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
        n, d = theta.shape
        batch = X.shape[0]
        if X.shape != (batch, self.n_in) or y.numel() != batch:
            raise ValueError("X must be [batch, %d] and y [batch]" % self.n_in)
        if out is None:
            out = torch.empty_like(theta)
        name = "stein_score_bnn" if self.n_in <= 4 else "stein_score_bnn_wide"
        _lib.call_on(theta.device, name, theta.data_ptr(), n, d, self.n_in, self.n_hidden, self._cols, X.data_ptr(),
                  y.data_ptr(), batch, self.n_train, self.gamma_a, self.gamma_b, out.data_ptr(),
                  torch.cuda.current_stream(theta.device).cuda_stream)
        return out


class SoftmaxScore:
    """Score of softmax (multi-class logistic) regression, for every particle in one launch (csrc/stein_score_softmax.hip).

    score(theta_matrix, feed) -> [n, d] float32 device tensor, feed = {"X": [batch, n_feats] float32, "y": [batch] class
    indices in any integer dtype}.  A particle packs W [n_feats, n_classes] row-major at w_col -- how a [F, C] variable
    flattens -- and log(alpha) at alpha_col (None: the fixed prior precision); there is no bias term, append a column of
    ones to X.  Prior and scaling as GlmScore's logistic model: W ~ N(0, 1/alpha), alpha ~ Gamma(1, gamma_rate), the batch's
    log-likelihood times n_train / batch.  2 <= n_classes <= 32, n_feats <= 1024, n_feats * n_classes <= 16384.
    """
    wants_matrix = True

    def __init__(self, n_feats, n_classes, w_col=0, alpha_col=None, n_train=None, prior_precision=1.0, gamma_rate=0.01):
        self.n_feats, self.n_classes, self.w_col = int(n_feats), int(n_classes), int(w_col)
        self.alpha_col = -1 if alpha_col is None else int(alpha_col)
        self.n_train = n_train
        self.prior_precision, self.gamma_rate = float(prior_precision), float(gamma_rate)

    def __call__(self, theta, feed, out=None):
        X = feed["X"]
        for name, t in (("theta", theta), ("X", X)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
        n, d = theta.shape
        batch = X.shape[0]
        if X.shape != (batch, self.n_feats):
            raise ValueError("X must be [batch, %d]" % self.n_feats)
        y = _labels_i32(feed["y"], batch, theta.device)
        if out is None:
            out = torch.empty_like(theta)
        scale = 1.0 if self.n_train is None else float(self.n_train) / batch
        _lib.call_on(theta.device, "stein_score_softmax", theta.data_ptr(), n, d, self.w_col, self.n_feats, self.n_classes,
                     self.alpha_col, X.data_ptr(), y.data_ptr(), batch, scale, self.prior_precision, self.gamma_rate,
                     out.data_ptr(), torch.cuda.current_stream(theta.device).cuda_stream)
        return out


class BnnClassScore:
    """Score of the network classifier, one hidden ReLU layer with a softmax head, for every particle in one launch
    (csrc/stein_score_bnn_class.hip).

    score(theta_matrix, feed) -> [n, d] float32 device tensor, feed = {"X": [batch, n_in] float32, "y": [batch] class indices
    in any integer dtype}.  cols: first column of (w1 [n_in, H], b1 [H], w2 [H, C], b2 [C], log_lambda) in the packed
    particle matrix, each flattened row-major -- use ``BnnClassScore.columns(sampler.access)``; cols[4] may be None: the fixed
    prior precision.  Likelihood, prior and scaling are SoftmaxScore's over all four blocks -- every entry ~ N(0, 1/lambda),
    lambda ~ Gamma(1, gamma_rate), the batch's log-likelihood times n_train / batch; BnnScore's division of everything by
    n_train is not taken over.  1 <= n_in <= 128, 2 <= n_classes <= 32, n_hidden <= 512 and
    (n_in + CS) * n_hidden <= 16384 with CS = n_classes rounded up to a multiple of 4.
    """
    wants_matrix = True
    NAMES = ("model/w_1:0", "model/b_1:0", "model/w_2:0", "model/b_2:0", "model/log_lambda:0")

    def __init__(self, n_in, n_hidden, n_classes, cols, n_train=None, prior_precision=1.0, gamma_rate=0.01):
        import ctypes
        self.n_in, self.n_hidden, self.n_classes = int(n_in), int(n_hidden), int(n_classes)
        self.n_train = n_train
        self.prior_precision, self.gamma_rate = float(prior_precision), float(gamma_rate)
        cols = list(cols)
        if len(cols) == 4:
            cols.append(None)
        if len(cols) != 5:
            raise ValueError("cols must give the first column of w1, b1, w2, b2 and log_lambda (None: fixed precision)")
        self._cols = (ctypes.c_int64 * 5)(*[-1 if c is None else int(c) for c in cols])

    @staticmethod
    def columns(access, names=NAMES):
        """first packed column of each parameter block from a sampler's access map {name: (start, end)}; a name that is
        None or absent from the map (the log_lambda of a fixed-precision model) gives None"""
        return tuple(access[k][0] if k is not None and k in access else None for k in names)

    def __call__(self, theta, feed, out=None):
        X = feed["X"]
        for name, t in (("theta", theta), ("X", X)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
        n, d = theta.shape
        batch = X.shape[0]
        if X.shape != (batch, self.n_in):
            raise ValueError("X must be [batch, %d]" % self.n_in)
        y = _labels_i32(feed["y"], batch, theta.device)
        if out is None:
            out = torch.empty_like(theta)
        scale = 1.0 if self.n_train is None else float(self.n_train) / batch
        _lib.call_on(theta.device, "stein_score_bnn_class", theta.data_ptr(), n, d, self.n_in, self.n_hidden, self.n_classes,
                     self._cols, X.data_ptr(), y.data_ptr(), batch, scale, self.prior_precision, self.gamma_rate,
                     out.data_ptr(), torch.cuda.current_stream(theta.device).cuda_stream)
        return out


from .predict import BnnClassPredict, BnnPredict, GlmPredict, SoftmaxPredict  # noqa: E402,F401  (the producers of the step after the update)
