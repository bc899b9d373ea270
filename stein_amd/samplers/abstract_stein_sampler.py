"""SVGD driver with device-resident particles.

Counterpart of stein/samplers/abstract_stein_sampler.py:7-168.  What stays the same:
the constructor arguments, ``compute_phi(theta_array, grads_array)``,
``update_particles(grads_array)``, ``function_posterior(func, feed_dict, axis)``,
``train_on_batch(batch_feed)``, the ``theta`` dictionary keyed by model variable and
the N(0, 0.01^2) initialisation (:69-74).

What differs, deliberately: there is no TensorFlow session.  Particles live in ONE
contiguous [n, d] device tensor (``theta_matrix``); ``theta`` is a dict of zero-copy
views into it (columns ordered by sorted variable name, stein/utilities/converters.py:40).
``log_p`` is a callable instead of a TF tensor (see SteinSampler).  K is never
materialised and nothing on the update path synchronises with the host.

With a ``group`` (torch.distributed) each rank holds n/P particles; the engine gathers
rows once per step and reduces histograms and |phi|^2 (see engine.py).
"""
from abc import abstractmethod

import numpy as np
import torch

from .._checks import bandwidth_to_h2, check_kernel_name, ksd_statistic
from ..engine import SvgdEngine
from ..utilities.converters import convert_array_to_dictionary, convert_dictionary_to_array


class AbstractSteinSampler:
    INIT_SCALE = 0.01  # abstract_stein_sampler.py:72

    def __init__(self, n_particles, log_p, theta=None, *, model_vars=None, device="cuda", dtype=torch.float32,
                 group=None, seed=None, kernel_dtype=torch.float32, x3=None, ksd=False, bandwidth=None, h2=None,
                 median_every=1, ksd_every=None, kernel="rbf"):
        """
        n_particles : total number of particles n (across all ranks).
        log_p       : see SteinSampler.
        theta       : initial particles -- a dict {variable: [n_local, *shape]} (reference form) or a packed
                      [n_local, d] matrix; NumPy or torch.  None -> N(0, 0.01^2) draws, which needs model_vars.
        model_vars  : {name: shape} (or a list of objects with .name / .get_shape()) describing the parameters
                      of one particle; required when theta is None or a bare matrix that should be exposed as a dict.
        dtype       : storage type of particles and optimizer state: float32 (device-native) or float64 (the
                      reference's host dtype; the kernel path still runs in fp32 exactly as the reference's
                      fp32 placeholders do, stein/kernels/abstract_kernel.py:31).
        kernel_dtype: torch.float32 (default) or torch.bfloat16 -- what theta and the score are rounded to when they
                      are fed to the kernel / contraction (the reference rounds fp64 -> fp32 at that point).
        x3          : None (default: split-fp16 GEMMs on the 16-bit matrix cores) / False (fp32-input MFMA GEMMs); see engine.SvgdEngine.
        ksd         : also compute the kernelized Stein discrepancy in every step (stein_discrepancy()); see engine.SvgdEngine.
        bandwidth   : None (default): the median heuristic, every step.  A positive finite float h -- the reference's
                      ``kernel.bandwidth`` quantity, K = exp(-D / (2 h^2)) -- fixes the kernel instead: every step then takes
                      the streaming path (no median, no n x n workspace; see engine.SvgdEngine, h2=).
        h2          : the device form of the same: a 1-element float32 device tensor holding h^2, read on the device in every
                      step, which the caller may rewrite in place (annealing).  Give one of bandwidth / h2, not both.
                      bandwidth="median": the median heuristic on the streaming path -- the exact median of the n^2
                      distances taken without the n x n workspace (engine.SvgdEngine, h2="median").
        median_every : with bandwidth="median", refresh the median every this many steps (integer >= 1, default 1) and
                      hold the bandwidth in between; refused otherwise.
        ksd_every   : with bandwidth= / h2= (the streaming path), an integer k >= 1: every k-th update_particles, starting
                      with the first, also computes the kernelized Stein discrepancy at that step's bandwidth
                      (stein_discrepancy() returns the latest).  None (default): never.  Refused on any other sampler, where
                      ksd=True is the switch.
        kernel      : "rbf" (default) or "imq": the inverse multiquadric kernel (1 + D / (2 h^2))^(-1/2) at the same bandwidth
                      h, for the SVGD direction and for the Stein discrepancy of ksd_every= (engine.SvgdEngine, kernel=).
                      It exists on the streaming path only: give bandwidth= (a float, or "median") or h2=.
        """
        self.n_particles = int(n_particles)
        self.log_p = log_p
        self.device = torch.device(device)
        self.dtype = dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        world = 1
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
        if self.n_particles % world:
            raise ValueError("n_particles must be divisible by the number of ranks")
        self.n_local = self.n_particles // world
        self._group = group

        self._shapes = None
        if model_vars is not None:
            if isinstance(model_vars, dict):
                self._shapes = {k: list(v) for k, v in model_vars.items()}
            else:
                self._shapes = {v: list(v.get_shape().as_list()) for v in model_vars}
        self.model_vars = list(self._shapes.keys()) if self._shapes else None

        if theta is None:
            if not self._shapes:
                raise ValueError("theta=None needs model_vars={name: shape} to size the particles")
            if seed is not None:
                # every rank draws the FULL [n, ...] arrays from the same seeded stream and keeps its own rows: the
                # gathered particles equal the single-rank draw, and no two ranks start from the same particles (with
                # one stream per rank and the same seed, all ranks would hold identical copies and, SVGD being
                # deterministic, keep them forever)
                gen = np.random.default_rng(seed)
                rank = 0
                if group is not None:
                    rank = dist.get_rank(group)
                lo = rank * self.n_local
                theta = {v: (gen.normal(size=[self.n_particles] + s) * self.INIT_SCALE)[lo:lo + self.n_local]
                         for v, s in self._shapes.items()}
            else:   # the reference's unseeded global stream (abstract_stein_sampler.py:69-74); processes differ
                theta = {v: np.random.normal(size=[self.n_local] + s) * self.INIT_SCALE for v, s in self._shapes.items()}
        if isinstance(theta, dict):
            packed, self._access = convert_dictionary_to_array(theta)
            if self._shapes is None:
                self._shapes = {v: list(theta[v].shape[1:]) for v in theta}
                self.model_vars = list(self._shapes.keys())
        else:
            packed = theta
            if self._shapes:
                self._access, at = {}, 0
                for v in sorted(self._shapes, key=lambda k: k if isinstance(k, str) else k.name):
                    w = int(np.prod(self._shapes[v])) if self._shapes[v] else 1
                    self._access[v] = (at, at + w)
                    at += w
            else:
                self._access = None
        packed = torch.as_tensor(np.asarray(packed) if not isinstance(packed, torch.Tensor) else packed)
        if packed.dim() != 2 or packed.shape[0] != self.n_local:
            raise ValueError("theta must pack to [%d, d], got %s" % (self.n_local, tuple(packed.shape)))
        self.theta_matrix = packed.to(device=self.device, dtype=dtype).contiguous()
        self.n_params = self.theta_matrix.shape[1]
        self.kernel_dtype = kernel_dtype
        check_kernel_name(kernel)
        if kernel == "imq" and bandwidth is None and h2 is None:
            raise ValueError("kernel=\"imq\": the IMQ kernel exists on the streaming path only; pass bandwidth= (a float h, or "
                             "\"median\" for the median heuristic) or h2=")
        self.kernel_name = kernel
        if bandwidth is not None:
            if h2 is not None:
                raise ValueError("give bandwidth= (a float h) or h2= (a device tensor holding h^2), not both")
            h2 = bandwidth_to_h2(bandwidth, "a positive finite float or \"median\"")
        if ksd_every is not None:
            if isinstance(ksd_every, bool) or not isinstance(ksd_every, int) or ksd_every < 1:
                raise ValueError("ksd_every must be an integer >= 1 or None, got %r" % (ksd_every,))
            if h2 is None:
                raise ValueError("ksd_every= is the Stein discrepancy period of the streaming path (bandwidth= / h2=); a "
                                 "sampler at the median heuristic of every step computes it with ksd=True")
        self.ksd_every = ksd_every
        self._updates = 0           # update_particles calls so far
        self._ksd_sums = None       # [S, S_diag] of the latest step that computed them (streaming path; a device copy)
        self.engine = SvgdEngine(self.n_particles, self.n_params, device=self.device, group=group, x3=x3,
                                 dtype=kernel_dtype, ksd=ksd, h2=h2, median_every=median_every, kernel=kernel)
        self._theta32 = (self.theta_matrix if dtype == kernel_dtype else
                         torch.empty(self.n_local, self.n_params, dtype=kernel_dtype, device=self.device))

    # -- particle access ---------------------------------------------------------------------------
    @property
    def theta(self):
        """{variable: view [n_local, *shape]} over the packed device matrix (no copies)."""
        if self._access is None:
            raise AttributeError("the sampler was given a bare matrix and no model_vars; use theta_matrix / samples")
        return convert_array_to_dictionary(self.theta_matrix, self._access, self._shapes)

    def _theta_f32(self):
        if self.dtype != self.kernel_dtype:
            self._theta32.copy_(self.theta_matrix)  # the reference's fp64 -> fp32 feed (squared_exponential_kernel.py:27)
        return self._theta32

    def _score_to_device(self, grads_array):
        g = grads_array
        if isinstance(g, dict):
            g, _ = convert_dictionary_to_array(g)
        if not isinstance(g, torch.Tensor):
            g = np.asarray(g)
            if g.dtype not in (np.float32, np.float64):     # the reference hands over float64; float32 goes up as it is
                g = g.astype(np.float64)
            g = torch.from_numpy(np.ascontiguousarray(g))
        if tuple(g.shape) != (self.n_local, self.n_params):
            raise ValueError("score must be [%d, %d], got %s" % (self.n_local, self.n_params, tuple(g.shape)))
        return g.to(device=self.device, dtype=self.kernel_dtype).contiguous()

    # -- the hot path ---------------------------------------------------------------------------------
    def _foreign_kernel(self):
        """The reference's kernel seam (abstract_stein_sampler.py:103): any object with ``kernel_and_grad(theta) ->
        (K, dK)`` drops in as ``sampler.kernel``.  Returns it when it is NOT this package's fused RBF kernel (whose K the
        sampler never materialises), else None."""
        k = getattr(self, "kernel", None)
        if k is None:
            return None
        from ..kernels import SquaredExponentialKernel
        return None if isinstance(k, SquaredExponentialKernel) else k

    def compute_phi(self, theta_array, grads_array, discrepancy=False):
        """phi = (K . grads + dK) / n for the given particles (abstract_stein_sampler.py:100-105).
        discrepancy=True (streaming path only): the engine also leaves the Stein discrepancy sums of these particles.

        NumPy in -> float64 NumPy out (values carry fp32 precision); device tensors in -> float32 tensor out.
        With a user-supplied ``self.kernel`` the reference's own lines run instead: ``K, dK =
        self.kernel.kernel_and_grad(theta_array)``; ``(K.dot(grads_array) + dK) / n_particles`` in NumPy.
        """
        was_numpy = not isinstance(theta_array, torch.Tensor)
        foreign = self._foreign_kernel()
        if foreign is not None:
            if discrepancy:
                raise ValueError("a user-supplied kernel computes phi on the host: no Stein discrepancy")
            if self._group is not None:
                raise ValueError("a user-supplied kernel needs all particles on one rank")
            th = theta_array if was_numpy else theta_array.detach().double().cpu().numpy()
            g = grads_array
            if isinstance(g, dict):
                g, _ = convert_dictionary_to_array(g)
            g = g.detach().double().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
            n_particles, n_params = g.shape                                  # abstract_stein_sampler.py:100
            K, dK = foreign.kernel_and_grad(th)                              # :103
            K, dK = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (K, dK))
            phi = (K.dot(g) + dK) / n_particles                              # :105
            return phi if was_numpy else torch.as_tensor(phi).to(device=self.device, dtype=torch.float32)
        T = theta_array if not was_numpy else torch.from_numpy(np.ascontiguousarray(np.asarray(theta_array, dtype=np.float64)))
        T = T.to(device=self.device, dtype=self.kernel_dtype).contiguous()
        G = self._score_to_device(grads_array)
        phi = self.engine.compute_phi(T, G, discrepancy=True) if discrepancy else self.engine.compute_phi(T, G)
        return phi.double().cpu().numpy() if was_numpy else phi.clone()

    def stein_discrepancy(self, statistic="u"):
        """KSD^2 (a float) of the particles at the last step's score evaluation, i.e. before that step's update, under the
        step's RBF kernel and median bandwidth: statistic "u" (U-statistic, the default) or "v" (V-statistic).  Needs
        ksd=True and a step through the package's own kernel; reading it synchronises with the device.  Sharded: the
        statistic of all n particles, the same on every rank.
        With ksd_every=k (the streaming path): of the latest step that computed it -- every k-th, from the first -- under
        that step's bandwidth; a RuntimeError before the first."""
        if self.ksd_every is not None:
            # the streaming path: the sums of the latest step that computed them, at that step's bandwidth
            if self._ksd_sums is None:
                raise RuntimeError("no step has computed the Stein discrepancy yet (ksd_every=%d: the first "
                                   "update_particles does)" % self.ksd_every)
            return float(ksd_statistic(self._ksd_sums[0], self._ksd_sums[1], self.n_particles, statistic).item())
        if not self.engine.ksd:
            raise RuntimeError("build the sampler with ksd=True to get the Stein discrepancy")
        if self._foreign_kernel() is not None:
            raise RuntimeError("a user-supplied kernel computes phi on the host: the Stein discrepancy is only computed "
                               "with the package's own RBF kernel")
        return float(self.engine.stein_discrepancy(statistic).item())

    def update_particles(self, grads_array):
        """One SVGD step from the score matrix: phi, norm clip, optimizer apply
        (abstract_stein_sampler.py:121-127), all on device."""
        want = self.ksd_every is not None and self._updates % self.ksd_every == 0
        self._updates += 1
        if self._foreign_kernel() is not None or not hasattr(self.gd, "apply_"):
            self._update_particles_by_the_seams(grads_array, want)
        else:
            G = self._score_to_device(grads_array)
            phi = self.engine.compute_phi(self._theta_f32(), G, discrepancy=True) if want else \
                self.engine.compute_phi(self._theta_f32(), G)
            self.gd.apply_(self.theta_matrix, phi, self.engine.sqnorm)
        if want:
            self._ksd_sums = self.engine._sums[1:3].clone()   # (the next plain step leaves them alone, but says "not ready")

    def _update_particles_by_the_seams(self, grads_array, discrepancy=False):
        """The reference's duck-typed seams, line for line (abstract_stein_sampler.py:121-127): taken when ``self.gd`` is a
        reference-style optimizer (only ``update(phi) -> step``, no fused ``apply_``) or ``self.kernel`` is a user's
        object (only ``kernel_and_grad``).  phi still comes from the HIP engine unless the kernel is foreign; the clip and
        the optimizer run on the host in float64 as the reference's NumPy does."""
        g = grads_array
        if isinstance(g, dict):
            g, _ = convert_dictionary_to_array(g)
        g = g.detach().double().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g, dtype=np.float64)
        theta_array = self.theta_matrix.detach().double().cpu().numpy()      # :121 (a float64 copy, as the reference packs)
        phi = self.compute_phi(theta_array, g, discrepancy) if discrepancy else self.compute_phi(theta_array, g)   # :123
        # :125 -- on one rank NumPy's norm of phi, as the reference; sharded, phi holds this rank's rows and the norm is the
        # engine's all-reduced one
        norm = np.linalg.norm(phi) if self._group is None else float(self.engine.sqnorm.sqrt().item())
        phi *= 10. / max(10., norm)
        theta_array += self.gd.update(phi)                                   # :126
        self.theta_matrix.copy_(torch.as_tensor(theta_array).to(self.theta_matrix))   # :127

    def function_posterior(self, func, feed_dict=None, axis=None, gather=True):
        """Evaluate `func` under every particle (abstract_stein_sampler.py:157-168).

        func(theta_dict_or_matrix, feed_dict) must be batched over particles and return [n_local, ...]; the
        result is flattened per particle to [n_local, out] like the reference's np.ravel.  Sharded sampler: every rank
        evaluates its own particles and the rows are all-gathered in rank order (rank p holds particles
        [p n/P, (p + 1) n/P), so the gathered array is indexed like the reference's, all n particles: :160-162), unless
        gather=False.  The mean over `axis` is taken of that [n, out] array, as the reference does (:165-168).  Returns
        NumPy, the same array on every rank.  Collective when sharded: every rank must call it.

        A callable that carries ``wants_matrix = True`` (the predictive producers of stein_amd/predict.py) is handed the
        packed float32 [n_local, d] matrix instead of the dict of views, as the score producers are.
        """
        if getattr(func, "wants_matrix", False):
            arg = self._matrix_f32()
        else:
            arg = self.theta if self._access is not None else self.theta_matrix
        with torch.no_grad():
            out = func(arg, feed_dict)
        out = torch.as_tensor(out).reshape(self.n_local, -1).detach()
        if self._group is not None and gather:
            import torch.distributed as dist
            world = dist.get_world_size(self._group)
            # (the per-particle output width is the same on every rank: the same func on the same shapes)
            mine = out.to(self.device).contiguous()
            full = torch.empty(world * self.n_local, mine.shape[1], dtype=mine.dtype, device=mine.device)
            dist.all_gather_into_tensor(full, mine, group=self._group)
            out = full
        out = out.cpu().numpy()
        return out.mean(axis=axis) if axis is not None else out

    def _matrix_f32(self):
        """the packed particles as float32: the matrix itself, or the fp32 copy of a float64 sampler"""
        if self.dtype == torch.float32:
            return self.theta_matrix
        return self._theta_f32() if self.kernel_dtype == torch.float32 else self.theta_matrix.float()

    def posterior_predictive(self, producer, feed, weights=None, quantiles=None):
        """Per-test-point ensemble summaries of a predictive producer (stein_amd.predict.GlmPredict / BnnPredict) under
        the current particles: {"mean", "var"} of its outputs over the particles and, when `feed` has a "y", "lpd", the log
        predictive density log(1/n sum_p p(y_b | theta_p)) -- NumPy arrays of [batch].  The [n, batch] matrix that
        function_posterior returns is never formed; only the three vectors cross to the host.  One rank only.

        weights ([n], w_p >= 0: ``importance_weights(...)``, or ``torch.bincount(thin(m), minlength=n)``): the summaries
        under these weights, sum_p w_p (.) / sum_p w_p in place of 1/n sum_p (.), and "ess", the weights' effective
        sample size (sum w)^2 / sum w^2, a float.  A bad weight vector (a negative or non-finite entry, all zero) gives NaN.

        quantiles (e.g. (0.05, 0.5, 0.95)): also "quantiles", a NumPy [len(quantiles), batch] array of these quantiles of
        the outputs over the particles per test point (``producer.quantiles``: exact order statistics, NumPy's linear
        interpolation) -- the ensemble median and credible bands, where mean +- k sqrt(var) assumes a Gaussian ensemble.
        `quantiles` together with `weights` is a ValueError: weighted quantiles follow another definition (no
        interpolation) and come from ``predictive_quantiles(producer, feed, q, weights=w)``."""
        if quantiles is not None and weights is not None:
            raise ValueError("weighted quantiles are not interpolated and are not part of posterior_predictive: pass "
                             "`quantiles` or `weights`, not both, and use predictive_quantiles(producer, feed, q, weights=w)")
        if self._group is not None:
            raise ValueError("posterior_predictive works on one rank only: a sharded sampler would have to merge the "
                             "ranks' states; use function_posterior, which gathers the outputs")
        if not hasattr(producer, "summary"):
            raise ValueError("posterior_predictive needs a predictive producer (GlmPredict / BnnPredict)")
        if getattr(producer, "classes", False):
            raise ValueError("posterior_predictive summarises a scalar output per test point; a SoftmaxPredict gives class "
                             "probabilities: use predictive_classes(producer, feed)")
        ess = None
        with torch.no_grad():
            if weights is None:
                mean, var, lpd = producer.summary(self._matrix_f32(), feed)
            else:
                mean, var, lpd, ess = producer.weighted_summary(self._matrix_f32(), feed, weights)
            band = None if quantiles is None else producer.quantiles(self._matrix_f32(), feed, quantiles)
        out = {"mean": mean.cpu().numpy(), "var": var.cpu().numpy()}
        if band is not None:
            out["quantiles"] = band.cpu().numpy()
        if lpd is not None:
            out["lpd"] = lpd.cpu().numpy()
        if ess is not None:
            out["ess"] = float(ess.item())
        return out

    def predictive_classes(self, producer, feed, weights=None):
        """Per-test-point summaries of a class-probability producer (stein_amd.predict.SoftmaxPredict) under the current
        particles, NumPy arrays: "prob" [batch, C], the posterior predictive class probabilities mean_p p_pbc; "label"
        [batch] int32, their argmax (ties to the lowest class); "entropy" [batch], H(prob_b.), the total predictive
        uncertainty; "mutual_information" [batch], entropy minus the expected entropy mean_p H(p_pb.), clipped at 0 -- the
        part of the uncertainty that comes from the particles disagreeing, large far from the training data; and, when
        `feed` has a "y", "lpd" [batch] = log(mean_p p_{pb,y_b}).  The [n, batch, C] tensor that function_posterior returns
        is never formed.  One rank only.

        weights ([n], w_p >= 0: ``importance_weights(...)``, or the integer counts ``torch.bincount(thin(m), minlength=n)``):
        every mean over the particles becomes the weighted mean sum_p w_p (.) / W (``producer.weighted_summary``), the
        entropy and the mutual information are taken of the weighted prob as before, and "ess" (float), the weights'
        effective sample size W^2 / sum_p w_p^2, joins the dict.  The weights are never read on the host: bad ones (negative,
        non-finite, all zero) give NaN rows, NaN "ess" and the label -1."""
        if self._group is not None:
            raise ValueError("predictive_classes works on one rank only: a sharded sampler would have to merge the ranks' "
                             "sums; use function_posterior, which gathers the outputs")
        if not getattr(producer, "classes", False):
            raise ValueError("predictive_classes needs a class-probability producer (SoftmaxPredict); GlmPredict and "
                             "BnnPredict go to posterior_predictive")
        with torch.no_grad():
            if weights is None:
                s = producer.summary(self._matrix_f32(), feed)
            else:
                s = producer.weighted_summary(self._matrix_f32(), feed, weights)
        prob = s["prob"].cpu().numpy()
        p64 = prob.astype(np.float64)
        entropy = -(p64 * np.log(np.where(p64 > 0, p64, 1.0))).sum(-1)
        out = {"prob": prob, "label": s["label"].cpu().numpy(), "entropy": entropy.astype(np.float32)}
        out["mutual_information"] = np.maximum(out["entropy"] - s["ent"].cpu().numpy(), np.float32(0))
        if "lpd" in s:
            out["lpd"] = s["lpd"].cpu().numpy()
        if weights is not None:
            out["ess"] = float(s["ess"].item())
        return out

    def predictive_quantiles(self, producer, feed, q, weights=None):
        """-> NumPy [len(q), batch]: the q-quantiles (e.g. (0.05, 0.5, 0.95)) of a predictive producer's outputs over the
        current particles per test point, without the [n, batch] matrix.  One rank only.

        weights=None: ``producer.quantiles`` -- exact order statistics under NumPy's linear interpolation, what
        ``posterior_predictive(..., quantiles=q)`` returns.
        weights ([n]: ``importance_weights(...)``, or the integer counts ``torch.bincount(thin(m), minlength=n)``):
        ``producer.weighted_quantiles`` -- the inverted weighted distribution function, the smallest output at which the
        cumulative weight reaches q of the total.  It is an element of the ensemble and is NOT interpolated, so with
        uniform weights it is the "inverted_cdf" quantile, not the linear one.  Bad weights give NaN."""
        if self._group is not None:
            raise ValueError("predictive_quantiles works on one rank only: a sharded sampler would have to merge the "
                             "ranks' counts; use function_posterior, which gathers the outputs")
        if not hasattr(producer, "weighted_quantiles"):
            raise ValueError("predictive_quantiles needs a predictive producer (GlmPredict / BnnPredict)")
        with torch.no_grad():
            if weights is None:
                band = producer.quantiles(self._matrix_f32(), feed, q)
            else:
                band = producer.weighted_quantiles(self._matrix_f32(), feed, weights, q)
        return band.cpu().numpy()

    def predictive_cdf(self, producer, feed, t=None, weights=None):
        """-> NumPy: the predictive distribution function of y, observation noise included, over the current particles --
        ``producer.y_cdf``.  t=None: at ``feed["y"]`` -> [batch], the probability integral transform of the rows (its
        histogram is flat for a calibrated sampler); t [n_pts, batch] (NumPy or a tensor) -> [n_pts, batch].  weights ([n]:
        ``importance_weights(...)``, or the integer counts ``torch.bincount(thin(m), minlength=n)``, taken as they are): the
        mixture under these weights.  Regression models only; one rank only.  Bad weights give NaN."""
        if self._group is not None:
            raise ValueError("predictive_cdf works on one rank only: a sharded sampler would have to merge the ranks' "
                             "sums; use function_posterior, which gathers the outputs")
        if not hasattr(producer, "y_cdf"):
            raise ValueError("predictive_cdf needs a predictive producer (GlmPredict / BnnPredict)")
        with torch.no_grad():
            if t is not None:
                t = torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous()
            out = producer.y_cdf(self._matrix_f32(), feed, t, weights=weights)
        return out.cpu().numpy()

    def predictive_interval(self, producer, feed, q, weights=None, passes=8):
        """-> NumPy [len(q), batch]: the q-quantiles of the predictive distribution of y per test point, observation noise
        included -- ``predictive_interval(producer, feed, (0.05, 0.95))`` is the 90 % interval that should hold 90 % of
        held-out observations, which the credible band of ``predictive_quantiles`` (the spread of the model outputs alone)
        does not.  ``producer.y_quantiles``: q strictly inside (0, 1), `passes` bracket refinements (8 reach neighbouring
        floats); weights as for ``predictive_cdf``.  Regression models only; one rank only."""
        if self._group is not None:
            raise ValueError("predictive_interval works on one rank only: a sharded sampler would have to merge the ranks' "
                             "sums; use function_posterior, which gathers the outputs")
        if not hasattr(producer, "y_quantiles"):
            raise ValueError("predictive_interval needs a predictive producer (GlmPredict / BnnPredict)")
        with torch.no_grad():
            band = producer.y_quantiles(self._matrix_f32(), feed, q, weights=weights, passes=passes)
        return band.cpu().numpy()

    def samples_all(self):
        """All n particles as one float64 [n, d] NumPy array on every rank (the reference's `samples`, stein_sampler.py:73-78,
        for a sharded sampler; on one rank it equals `samples`).  Collective when sharded."""
        if self._group is None:
            return self.theta_matrix.detach().double().cpu().numpy()
        import torch.distributed as dist
        world = dist.get_world_size(self._group)
        full = torch.empty(world * self.n_local, self.n_params, dtype=self.theta_matrix.dtype, device=self.device)
        dist.all_gather_into_tensor(full, self.theta_matrix.contiguous(), group=self._group)
        return full.double().cpu().numpy()

    @abstractmethod
    def train_on_batch(self, batch_feed):
        raise NotImplementedError()

    # -- save / restore (the reference leaves this to pickling its attributes) -----------------------
    def state_dict(self):
        return {"theta": self.theta_matrix.detach().cpu().numpy(), "gd": self.gd.state_dict()}

    def load_state_dict(self, state):
        self.theta_matrix.copy_(torch.as_tensor(state["theta"]).to(self.theta_matrix))
        self.gd.load_state_dict(state["gd"], device=self.device)
