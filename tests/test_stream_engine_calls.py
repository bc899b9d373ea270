"""CPU: what a streaming engine (SvgdEngine(..., h2=...)) asks of its stages, call by call.  The stages are a recording
double, the tensors live on the CPU and nothing is launched; the plan and the workspace sizes are the library's own host
arithmetic (as in tests/test_stream_layout.py).  Both kernels, at 300 x 10 (three row tiles, three j ranges) and at 1 x 3."""
import numpy as np
import pytest
import torch

from stein_amd import _lib
from stein_amd.engine import SvgdEngine

# kernel -> (plain step, step with the statistic, plan, bytes of the step, bytes of the step with the statistic)
KERNELS = {"rbf": ("svgd_phi_stream", "svgd_phi_stream_ksd", _lib.stream_plan, _lib.stream_workspace_bytes,
                   _lib.stream_ksd_workspace_bytes),
           "imq": ("svgd_phi_imq", "svgd_phi_imq_ksd", _lib.imq_plan, _lib.imq_workspace_bytes, _lib.imq_ksd_workspace_bytes)}
SHAPES = [(300, 10), (1, 3)]
S, S_DIAG = 7.0, 3.0      # what the double's steps with the statistic leave in sums[1], sums[2]


class RecordingStages:
    """The five streaming stage calls: each stores (name, keyword form of its arguments) and launches nothing."""

    name = "recording"

    def __init__(self):
        self.calls = []

    def _step(self, name, T, G, n, d, h2, phi, out, ws):
        self.calls.append((name, dict(T=T, G=G, n=n, d=d, h2=h2, phi=phi, out=out, ws=ws)))

    def svgd_phi_stream(self, *args):
        self._step("svgd_phi_stream", *args)

    def svgd_phi_imq(self, *args):
        self._step("svgd_phi_imq", *args)

    def _step_ksd(self, name, *args):
        self._step(name, *args)
        args[6][1], args[6][2] = S, S_DIAG

    def svgd_phi_stream_ksd(self, *args):
        self._step_ksd("svgd_phi_stream_ksd", *args)

    def svgd_phi_imq_ksd(self, *args):
        self._step_ksd("svgd_phi_imq_ksd", *args)

    def stream_median(self, T, n, d, h2, median, ws):
        self.calls.append(("stream_median", dict(T=T, n=n, d=d, h2=h2, median=median, ws=ws)))


def _engine(n, d, kernel, h2, **kw):
    st = RecordingStages()
    return SvgdEngine(n, d, device="cpu", stages=st, h2=h2, kernel=kernel, **kw), st


def _inputs(n, d):
    return torch.zeros(n, d), torch.ones(n, d)


def _new_calls(eng, st, fn):
    """run fn; the calls it made, every one of them on the engine's current workspace and bandwidth tensor"""
    before = len(st.calls)
    fn()
    made = st.calls[before:]
    for name, a in made:
        assert a["ws"] is eng.ws and a["ws"].numel() == eng.ws_bytes, name
        assert a["h2"] is eng.h2 and (a["n"], a["d"]) == (eng.n, eng.d), name
    return made


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_call_order_and_arguments_with_the_median_refreshed_every_second_step(kernel):
    n, d = SHAPES[0]
    step, step_ksd, plan, step_bytes, ksd_bytes = KERNELS[kernel]
    eng, st = _engine(n, d, kernel, "median", median_every=2)
    T, G = _inputs(n, d)
    assert eng.streaming and eng.kernel == kernel and eng.median_every == 2 and eng.stages is st
    assert (eng.row_tiles, eng.col_groups, eng.jsplit) == plan(n, d) and eng.row_tiles == 3 and eng.jsplit == 3
    assert eng.sqnorm.data_ptr() == eng._sums.data_ptr() and eng.sqnorm.shape == (1,) and eng._sums.shape == (3,)
    assert eng.h2.shape == eng.median.shape == (1,) and eng.h2.dtype == eng.median.dtype == torch.float32
    first = max(step_bytes(n, d), _lib.stream_median_workspace_bytes(n, d))
    grown = ksd_bytes(n, d)
    print("%s %d x %d: workspace %d bytes (step %d, median %d), with the statistic %d" %
          (kernel, n, d, first, step_bytes(n, d), _lib.stream_median_workspace_bytes(n, d), grown))
    assert grown > first
    ws0 = eng.ws
    assert eng.ws_bytes == first == ws0.numel() and ws0.dtype == torch.uint8

    made = _new_calls(eng, st, lambda: eng.compute_phi(T, G))
    assert eng.ws is ws0 and eng.ws_bytes == first
    made += _new_calls(eng, st, lambda: eng.compute_phi(T, G, discrepancy=True))
    ws1 = eng.ws
    assert ws1 is not ws0 and eng.ws_bytes == grown == ws1.numel()        # re-allocated, once
    made += _new_calls(eng, st, lambda: eng.compute_phi(T, G))
    made += _new_calls(eng, st, lambda: eng.stream_discrepancy_sums(T, G))
    made += _new_calls(eng, st, lambda: eng.refresh_bandwidth(T))
    assert eng.ws is ws1 and eng.ws_bytes == grown                        # ... and never shrinks
    assert len(made) == len(st.calls)
    assert [name for name, _ in made] == ["stream_median", step, step_ksd, "stream_median", step, "stream_median", step_ksd,
                                          "stream_median"]
    for i, (name, a) in enumerate(made):
        assert a["T"] is T, i
        if name == "stream_median":
            assert a["median"] is eng.median, i
            continue
        assert a["G"] is G, i
        assert a["out"] is (eng._sums if name == step_ksd else eng.sqnorm), i
        assert a["phi"] is (None if i == 6 else eng.phi), i               # stream_discrepancy_sums stores no phi
    assert eng.phi.shape == (n, d) and eng.phi.dtype == torch.float32


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("n,d", SHAPES)
def test_a_supplied_bandwidth_and_the_workspace(kernel, n, d):
    step, step_ksd, plan, step_bytes, ksd_bytes = KERNELS[kernel]
    T, G = _inputs(n, d)
    h2t = torch.full((1,), 2.5)
    eng, st = _engine(n, d, kernel, h2t)
    assert eng.h2 is h2t and eng.median_every is None                     # adopted, not copied
    assert (eng.row_tiles, eng.col_groups, eng.jsplit) == plan(n, d)
    assert eng.ws_bytes == step_bytes(n, d) == eng.ws.numel() and ksd_bytes(n, d) >= step_bytes(n, d)
    made = _new_calls(eng, st, lambda: eng.compute_phi(T, G))
    made += _new_calls(eng, st, lambda: eng.compute_phi(T, G, discrepancy=True))
    assert eng.ws_bytes == ksd_bytes(n, d) == eng.ws.numel()
    made += _new_calls(eng, st, lambda: eng.stream_discrepancy_sums(T, G))
    assert [name for name, _ in made] == [step, step_ksd, step_ksd]       # no median call without h2="median"
    assert made[0][1]["out"] is eng.sqnorm and made[1][1]["out"] is eng._sums and made[2][1]["out"] is eng._sums
    assert made[0][1]["phi"] is eng.phi and made[1][1]["phi"] is eng.phi and made[2][1]["phi"] is None
    assert eng.stream_discrepancy_sums(T, G) is eng._sums
    # a float is stored once, rounded to float32
    flt, _ = _engine(n, d, kernel, 0.1)
    assert flt.h2.shape == (1,) and flt.h2.dtype == torch.float32 and flt.h2.item() == float(np.float32(0.1)) != 0.1
    assert flt.ws_bytes == step_bytes(n, d) and flt.median_every is None
    # the GPU tests grow a fresh engine's workspace by hand before its first call (tests/test_gpu_stream_ksd.py)
    flt._stream_ksd_workspace()
    assert flt.ws_bytes == ksd_bytes(n, d) == flt.ws.numel()


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("n,d", SHAPES)
def test_the_statistic_is_of_the_last_call_only(kernel, n, d):
    eng, st = _engine(n, d, kernel, 1.5)
    T, G = _inputs(n, d)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        eng.stein_discrepancy()
    eng.compute_phi(T, G)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        eng.stein_discrepancy()
    eng.compute_phi(T, G, discrepancy=True)
    v = eng.stein_discrepancy("v")
    assert v.dtype == torch.float64 and v.dim() == 0 and v.item() == S / (float(n) * n)
    assert torch.equal(v, eng._sums[1] / (float(n) * n))
    if n == 1:
        with pytest.raises(ValueError, match="at least two"):
            eng.stein_discrepancy("u")
        with pytest.raises(ValueError, match="at least two"):
            eng.stein_discrepancy()
    else:
        u = eng.stein_discrepancy()
        assert u.dtype == torch.float64 and u.dim() == 0 and u.item() == (S - S_DIAG) / (float(n) * (n - 1.0))
        assert torch.equal(u, eng.stein_discrepancy("u"))
    with pytest.raises(ValueError, match="statistic must be"):
        eng.stein_discrepancy("w")
    eng.compute_phi(T, G)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        eng.stein_discrepancy("v")
    eng.stream_discrepancy_sums(T, G)
    assert eng.stein_discrepancy("v").item() == S / (float(n) * n)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_the_stored_distance_surface_is_refused_by_name(kernel):
    n, d = SHAPES[0]
    eng, st = _engine(n, d, kernel, 1.5)
    T, G = _inputs(n, d)
    eng.compute_phi(T, G)
    with pytest.raises(ValueError, match="dist_matrix"):
        eng.dist_matrix()
    for view in ("rownorm", "dist", "hist", "select_state", "spec_section", "spec_table", "planes"):
        with pytest.raises(ValueError, match="streaming"):
            getattr(eng, view)
    with pytest.raises(ValueError, match="streaming"):
        eng.window_stats()
    with pytest.raises(ValueError, match="K_out"):
        eng.compute_phi(T, G, K_out=torch.empty(n, n))
    with pytest.raises(ValueError, match="dK_out"):
        eng.compute_phi(T, G, dK_out=torch.empty(n, d))
    with pytest.raises(ValueError, match="mark"):
        eng.compute_phi(T, G, mark=lambda label: None)
    with pytest.raises(ValueError, match="timing"):
        eng.compute_phi(T, G, timing=True)
    with pytest.raises(ValueError, match="contiguous"):
        eng.compute_phi(T[:, :2], G)
    with pytest.raises(ValueError, match="refresh_bandwidth"):
        eng.refresh_bandwidth(T)
    assert len(st.calls) == 1                                             # every refusal came before a stage call
