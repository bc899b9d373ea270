"""SteinSampler: the user-facing SVGD sampler (stein/samplers/stein_sampler.py:8-78).

``SteinSampler(n_particles, log_p, gd, theta=None)`` keeps the reference's argument order.
Because there is no TF graph here, ``log_p`` is a callable:

    log_p(theta, batch_feed) -> tensor [n_local]     log-posterior of every particle,

written with torch ops on ``theta`` (the dict of per-variable views, or the packed matrix
when no model_vars were given), batched over the particle axis.  The score matrix the
reference obtains with n sequential ``sess.run(grad_log_p)`` calls (:59-68) comes from one
reverse pass: particles are independent, so d(sum_i log_p_i)/d(theta) is the per-particle
score.  A closed-form ``score(theta, batch_feed) -> [n_local, d]`` may be supplied instead
(keyword ``score=``), or the caller can skip both and drive ``update_particles`` directly.
"""
import torch

from ..utilities.converters import convert_array_to_dictionary
from .abstract_stein_sampler import AbstractSteinSampler


class SteinSampler(AbstractSteinSampler):
    def __init__(self, n_particles, log_p, gd, theta=None, *, score=None, **kwargs):
        super().__init__(n_particles, log_p, theta, **kwargs)
        self.gd = gd
        self.score = score
        # stein_sampler.py:48.  While this is the package's own RBF kernel the sampler goes through the fused engine (K is
        # never materialised); assign any other object with kernel_and_grad(theta) -> (K, dK) and update_particles /
        # compute_phi call it exactly as the reference does (abstract_stein_sampler.py:103)
        from ..kernels import SquaredExponentialKernel
        self.kernel = SquaredExponentialKernel(self.n_particles, None, device=self.device) \
            if self._group is None and self.kernel_name == "rbf" else None   # (kernel="imq": no n x n kernel_and_grad exists)

    def score_matrix(self, batch_feed=None):
        """[n_local, d] float32 device tensor of d log_p / d theta for every particle."""
        if self.score is not None:
            if getattr(self.score, "wants_matrix", False):   # device score producers (stein_amd.scores) take the packed matrix
                if self.dtype != torch.float32:
                    raise ValueError("device score producers need float32 particles")
                return self.score(self.theta_matrix, batch_feed)
            arg = self.theta if self._access is not None else self.theta_matrix
            g = self.score(arg, batch_feed)
            if isinstance(g, dict):
                from ..utilities.converters import convert_dictionary_to_array
                g, _ = convert_dictionary_to_array(g)
            return torch.as_tensor(g).to(device=self.device, dtype=torch.float32).reshape(
                self.n_local, self.n_params).contiguous()
        if self.log_p is None:
            raise ValueError("no log_p / score callable: call update_particles(score_matrix) directly")
        t = self.theta_matrix.detach().clone().requires_grad_(True)
        arg = convert_array_to_dictionary(t, self._access, self._shapes) if self._access is not None else t
        lp = self.log_p(arg, batch_feed)
        if lp.shape != (self.n_local,):
            raise ValueError("log_p must return one value per particle, shape (%d,), got %s" %
                             (self.n_local, tuple(lp.shape)))
        (g,) = torch.autograd.grad(lp.sum(), t)
        return g.to(torch.float32).contiguous()

    def train_on_batch(self, batch_feed=None):
        """One SVGD iteration on a batch (stein_sampler.py:50-71)."""
        self.update_particles(self.score_matrix(batch_feed))

    def thin(self, m, batch_feed=None, bandwidth="median", kernel="imq", return_ksd=False):
        """Stein thinning of the sampler's own particles at their current scores (score_matrix(batch_feed)): the indices,
        an int64 device tensor [m], of the m greedy picks (stein_amd.utilities.stein_thinning, which see for bandwidth,
        kernel and return_ksd).  `theta_matrix[idx]` is the thinned particle set.  One rank only."""
        if self._group is not None:
            raise ValueError("thin works on one rank only: a pick is an argmin over all n particles; gather them "
                             "(samples_all) and call stein_amd.utilities.stein_thinning")
        from ..utilities.stein_thinning import stein_thinning
        return stein_thinning(self._matrix_f32().detach(), self.score_matrix(batch_feed).detach(), m, bandwidth=bandwidth,
                              kernel=kernel, return_ksd=return_ksd)

    def goodness_of_fit(self, batch_feed=None, **kw):
        """The KSD goodness-of-fit test of the sampler's own particles at their current scores (score_matrix(batch_feed)):
        (statistic, p_value) from stein_amd.utilities.stein_goodness_of_fit, which takes the keyword arguments.
        Caveat: SVGD particles interact, and the test's level is only guaranteed for (possibly dependent) DRAWS from a
        distribution.  For particles the p-value is a calibrated scale for the statistic -- how large it is against
        what sign-flipped copies of the same sample give -- not a proof of convergence.  One rank only."""
        if self._group is not None:
            raise ValueError("goodness_of_fit works on one rank only: the statistic couples all n particles; gather "
                             "them (samples_all) and call stein_amd.utilities.stein_goodness_of_fit")
        from ..utilities.stein_test import stein_goodness_of_fit
        return stein_goodness_of_fit(self._matrix_f32().detach(), self.score_matrix(batch_feed).detach(), **kw)

    def importance_weights(self, batch_feed=None, iters=None, bandwidth="median", kernel="imq", return_path=False):
        """Stein importance weights of the sampler's own particles at their current scores (score_matrix(batch_feed)):
        (w, info) from stein_amd.utilities.stein_importance_weights, which see -- w a float64 device tensor [n] on the
        simplex that lowers the KSD^2 of the weighted particles, info its KSD^2, the uniform weights' and the duality gap.
        `(w[:, None] * f(theta_matrix)).sum(0)` is the corrected estimate; the particles do not move.  One rank only."""
        if self._group is not None:
            raise ValueError("importance_weights works on one rank only: the weights couple all n particles; gather "
                             "them (samples_all) and call stein_amd.utilities.stein_importance_weights")
        from ..utilities.stein_weights import stein_importance_weights
        return stein_importance_weights(self._matrix_f32().detach(), self.score_matrix(batch_feed).detach(), iters=iters,
                                        bandwidth=bandwidth, kernel=kernel, return_path=return_path)

    @property
    def samples(self):
        """Packed [n_local, d] particle matrix as NumPy (stein_sampler.py:73-78)."""
        return self.theta_matrix.detach().cpu().numpy()
