"""StreamEngine, what SvgdEngine(..., h2=...) (engine.py) constructs; the two share the stages, _checks.py and nothing else."""
import torch

from . import _lib
from ._checks import check_engine_switches, ksd_statistic, positive_float
from .engine import HipStages

# per kernel: the stages' step without / with the Stein discrepancy sums, the plan, the workspace bytes of the two steps
_KERNELS = {
    "rbf": ("svgd_phi_stream", "svgd_phi_stream_ksd", _lib.stream_plan, _lib.stream_workspace_bytes,
            _lib.stream_ksd_workspace_bytes),
    "imq": ("svgd_phi_imq", "svgd_phi_imq_ksd", _lib.imq_plan, _lib.imq_workspace_bytes, _lib.imq_ksd_workspace_bytes),
}
_STORED_D_ONLY = ("dist_matrix", "rownorm", "dist", "hist", "select_state", "select_state_bytes", "spec_section",
                  "spec_table", "planes", "window_stats")


class StreamEngine:
    """phi by the streaming SVGD step (include/steinhip.h): no n x n image, a workspace of O(n d) bytes without sections, one
    rank, float32 inputs on the split path.  SvgdEngine's signature; its stored-D switches (small ... fold) mean nothing here.

    h2      : the SQUARED bandwidth.  A positive finite float is stored once in a 1-element device tensor; a 1-element
              float32 device tensor is used as it is -- the library reads it on the device in every step, so the caller may
              rewrite it in place between steps (an annealing schedule) or hand over another engine's `h2`.  Either way
              `self.h2` is that tensor.  "median": the engine owns `self.h2` and `self.median` and, before the step of every
              call whose 0-based index is a multiple of `median_every` (an integer >= 1), takes the exact median of the n^2
              distances (n >= 2) in its own workspace (stein_stream_median) and holds h2 in between; refresh_bandwidth(theta).
    kernel  : "rbf" (default): exp(-D / (2 h2)).  "imq": the inverse multiquadric kernel (1 + D / (2 h2))^(-1/2), whose Stein
              discrepancy detects non-convergence for d >= 3 (Gorham & Mackey 2017): the SAME bandwidth, about twice the cost.
    """

    streaming, group, sharded, comm = True, None, False, None               # (what callers of either engine read)
    dtype, x3, ksd, fold, flags = torch.float32, True, False, False, 0

    def __init__(self, n, d, device="cuda", group=None, stages=None, x3=None, dtype=torch.float32, small=True,
                 window=True, force_collectives=False, comm="auto", tile_distance=False, dist_window=None, ksd=False,
                 fold=None, *, h2, median_every=1, kernel="rbf"):
        self.n, self.d = int(n), int(d)
        stream_median = check_engine_switches(kernel, h2, median_every)
        self.kernel, self.n_local, self.median = kernel, self.n, None
        self.median_every = median_every if stream_median else None
        refused = "group=" if group is not None else "bf16" if dtype != torch.float32 else \
            "x3=False" if (x3 is not None and not x3) else "ksd=True" if ksd else None
        if refused and kernel == "imq":
            raise ValueError("kernel=\"imq\": %s is not supported; the IMQ step is the streaming step's shape: one rank, float32 "
                             "inputs, the split path, and the Stein discrepancy per call (compute_phi(theta, score, "
                             "discrepancy=True), then stein_discrepancy())" % refused)
        if refused:
            raise ValueError("h2=: " + {
                "group=": "the streaming step runs on one rank; group= is not supported with a supplied bandwidth",
                "bf16": "the streaming step takes float32 inputs; bf16 is not supported with a supplied bandwidth",
                "x3=False": "the streaming step only exists on the split path; x3=False is not supported",
                "ksd=True": "ksd=True is not supported; the streaming step computes the Stein discrepancy per call: "
                            "compute_phi(theta, score, discrepancy=True), then stein_discrepancy()"}[refused])
        dev = self.device = torch.device(device)
        if stream_median:
            if self.n < 2:
                raise ValueError("n_particles = %d: the median-heuristic bandwidth divides by ln(n); need n >= 2" % self.n)
            self.h2 = torch.zeros(1, dtype=torch.float32, device=dev)     # written by the median call, on the device
            self.median = torch.zeros(1, dtype=torch.float32, device=dev)
        elif isinstance(h2, torch.Tensor):
            if h2.numel() != 1 or h2.dtype != torch.float32 or h2.device.type != dev.type or \
                    (dev.index is not None and h2.device.index != dev.index):
                raise ValueError("h2 must be a positive finite float or a 1-element float32 tensor on %s, got %s %s on %s" %
                                 (dev, tuple(h2.shape), h2.dtype, h2.device))
            self.h2 = h2       # read on the device in every step: never copied, never checked (that would synchronise)
        else:
            self.h2 = torch.full((1,), positive_float(h2, "h2", "a positive finite float or a 1-element float32 device tensor",
                                                      "h2 (the squared bandwidth)"), dtype=torch.float32, device=dev)
        if self.n < 1 or self.d < 1:
            raise ValueError("need n >= 1 and d >= 1, got n = %d, d = %d" % (self.n, self.d))
        step_name, ksd_name, plan, step_bytes, ksd_bytes = _KERNELS[kernel]
        self.stages = stages if stages is not None else HipStages()
        if not hasattr(self.stages, step_name):
            raise ValueError("h2=: the stages have no streaming step (HipStages has)")
        if stream_median and not hasattr(self.stages, "stream_median"):
            raise ValueError("h2=\"median\": the stages have no streaming median (HipStages has)")
        self._run, self._run_ksd = getattr(self.stages, step_name), getattr(self.stages, ksd_name, None)   # looked up once
        self.row_tiles, self.col_groups, self.jsplit = plan(self.n, self.d)
        # one buffer for the median call, the step and, once grown, the step with the statistic: each layout appends to the last
        self.ws_bytes, self._ksd_bytes = step_bytes(self.n, self.d), ksd_bytes(self.n, self.d)
        median_bytes = _lib.stream_median_workspace_bytes(self.n, self.d) if stream_median else 0
        assert median_bytes <= self.ws_bytes <= self._ksd_bytes
        self.ws_bytes = max(self.ws_bytes, median_bytes)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)   # nothing in it is read before it is written
        self.phi = torch.empty(self.n, self.d, dtype=torch.float32, device=dev)
        self._sums = torch.zeros(3, dtype=torch.float64, device=dev)      # |phi|^2 and, after a call with the statistic, S, S_diag
        self.sqnorm = self._sums[:1]                                      # (the view the optimizer apply reads)
        self._calls, self._ksd_ready = 0, False    # compute_phi calls so far (the refresh schedule); the last left S, S_diag

    def __getattr__(self, name):   # (only asked for what the engine lacks) a stored-D engine's views are refused by name
        if name in _STORED_D_ONLY:
            raise ValueError("h2=: the streaming step stores no distance matrix and its workspace has no sections of the stored-D "
                             "layout (row norms, distance image, histograms, select state, planes): no %s" % name)
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def _check_input(self, name, t):
        if tuple(t.shape) != (self.n, self.d) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous torch.float32 [%d, %d] tensor, got %s %s" %
                             (name, self.n, self.d, tuple(t.shape), t.dtype))

    def _stream_ksd_workspace(self):   # grow the workspace to what the step with the statistic needs (first use)
        if self._run_ksd is None:
            raise ValueError("discrepancy=True: the stages have no streaming step with the statistic (HipStages has)")
        if self.ws_bytes < self._ksd_bytes:
            self.ws = None      # (release before allocating: at the largest shapes both would not fit)
            self.ws = torch.empty(self._ksd_bytes, dtype=torch.uint8, device=self.device)
            self.ws_bytes = self._ksd_bytes

    def _step(self, theta, score, phi, discrepancy, refresh):
        self._check_input("theta", theta)
        self._check_input("score", score)
        if discrepancy:
            self._stream_ksd_workspace()
        if refresh:
            self.stages.stream_median(theta, self.n, self.d, self.h2, self.median, self.ws)
        run, out = (self._run_ksd, self._sums) if discrepancy else (self._run, self.sqnorm)
        run(theta, score, self.n, self.d, self.h2, phi, out, self.ws)
        self._ksd_ready = bool(discrepancy)

    def compute_phi(self, theta, score, K_out=None, dK_out=None, mark=None, timing=False, discrepancy=False):
        """As SvgdEngine.compute_phi on [n, d] float32 tensors: returns self.phi, leaves self.h2 and self.sqnorm, no host sync.
        discrepancy=True: the call also leaves the Stein discrepancy sums at its own bandwidth for stein_discrepancy(); phi,
        sqnorm and h2 are bit-identical to a call without it.  The workspace grows once, by one more row sum's partials."""
        if K_out is not None or dK_out is not None:
            raise ValueError("h2=: the streaming step forms neither K nor dK; K_out / dK_out are not supported")
        if mark is not None or timing:
            raise ValueError("h2=: the streaming step is one call; mark= / timing= are not supported")
        self._step(theta, score, self.phi, discrepancy, self.median_every is not None and self._calls % self.median_every == 0)
        self._calls += 1
        return self.phi

    def stream_discrepancy_sums(self, theta, score):
        """The statistic alone: |phi|^2, S, S_diag of `theta`, `score` at this engine's bandwidth into self._sums, phi not
        stored (the C entry with phi = NULL).  h2="median": taken from `theta` first, outside compute_phi's schedule."""
        self._step(theta, score, None, True, self.median_every is not None)
        return self._sums

    def refresh_bandwidth(self, theta):
        """h2="median": take the median-heuristic bandwidth of `theta` ([n, d] float32 device tensor) now; returns self.h2
        (self.median holds the median).  No host sync; compute_phi's refresh schedule (median_every) is not affected."""
        if self.median_every is None:
            raise ValueError("refresh_bandwidth needs an engine built with h2=\"median\"")
        self._check_input("theta", theta)
        self.stages.stream_median(theta, self.n, self.d, self.h2, self.median, self.ws)
        return self.h2

    def stein_discrepancy(self, statistic="u"):
        """as SvgdEngine.stein_discrepancy, of the last call if it computed the sums, at that call's bandwidth; "u": n >= 2"""
        if not self._ksd_ready:
            raise RuntimeError("the last compute_phi did not compute the Stein discrepancy: call "
                               "compute_phi(theta, score, discrepancy=True) first")
        return ksd_statistic(self._sums[1], self._sums[2], self.n, statistic)
