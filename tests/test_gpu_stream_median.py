"""GPU: the streaming median (stein_stream_median; SvgdEngine(h2="median"), SteinSampler(bandwidth="median")): the exact
median-heuristic bandwidth of all n^2 squared distances in the streaming step's O(n d) workspace.  The distance tiles are
recomputed once per radix level and counted straight from the accumulators (k_stream_hist, stein_amd/csrc/stein_stream.hip).

Where the distances are exact (integer lattices, tests/select_inputs.py) the expectation is an exact sort of the int64 D and
no GPU output enters it: h2, the median and the two order statistics are compared bit for bit.  On normal inputs the
bounds are other modules' (quoted where they are used), nothing is fitted to this code.
Run with -s to see every figure."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import select_inputs as si  # noqa: E402
import test_gpu_stream as ts  # noqa: E402
import test_gpu_x3 as tx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import HipStages, SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST_BYTES = _lib.HIST_LEVELS * 2 * _lib.HIST_BINS * 8
TOL_D = 4e-6       # per-entry bound of the split path's distances against fp64, x max D (test_gpu_x3.py:93); the median is
#                    1-Lipschitz in the sup norm of its inputs
TOL_H2 = 2e-6      # relative, h2 between two distance paths (test_gpu_x3.py:96)


def _run(T, cuda, ws=None):
    """one stein_stream_median call -> h2, median, lo, hi (Python floats) and the three histograms"""
    n, d = T.shape
    if ws is None:
        ws = torch.empty(_lib.stream_median_workspace_bytes(n, d), dtype=torch.uint8, device=cuda)
    h2 = torch.full((1,), float("nan"), dtype=torch.float32, device=cuda)
    med = torch.full((1,), float("nan"), dtype=torch.float32, device=cuda)
    HipStages().stream_median(T, n, d, h2, med, ws)
    torch.cuda.synchronize()
    hist_at, state_at, _, _ = _lib.stream_median_plan(n, d)
    lo, hi = ws[state_at + 40:state_at + 48].view(torch.float32).cpu().numpy()          # SelState::lo, ::hi
    hist = ws[hist_at:hist_at + HIST_BYTES].view(torch.int64).cpu().numpy().copy()
    return dict(h2=float(h2), med=float(med), lo=float(lo), hi=float(hi), hist=hist)


def _dev(P, cuda, scale=1.0):
    T = torch.tensor(np.asarray(P, dtype=np.float64) * scale, dtype=torch.float32, device=cuda).contiguous()
    assert torch.equal(T.double().cpu(), torch.tensor(np.asarray(P, dtype=np.float64) * scale))   # exact in fp32
    return T


def _assert_exact(got, ref, n, tag, scale2=1.0):
    """bit for bit against the int64 sort (scale2: the exact power of two the distances were scaled by)"""
    med = np.float32(ref.med) * np.float32(scale2)
    assert got["med"] == float(med), (tag, "median", got["med"], float(med))
    assert got["h2"] == float(si.bandwidth(med, n)), (tag, "h2", got["h2"], float(si.bandwidth(med, n)))
    assert (got["lo"], got["hi"]) == (ref.lo * scale2, ref.hi * scale2), (tag, "lo|hi", got["lo"], got["hi"], ref.lo, ref.hi)


def _same(a, b):
    return (a["h2"], a["med"], a["lo"], a["hi"]) == (b["h2"], b["med"], b["lo"], b["hi"]) and np.array_equal(a["hist"], b["hist"])


# ---------------------------------------------------------------------------------------------------------------
# 1. exact on the lattices
# ---------------------------------------------------------------------------------------------------------------
LATTICE_N = (129, 384, 768, 1001, 1536)
LATTICE_CASES = [(f, n) for n in LATTICE_N for f in si.families_at(n)]


@pytest.mark.parametrize("family,n", LATTICE_CASES, ids=lambda v: str(v))
def test_exact_on_lattices(cuda, family, n):
    ref = si.lattice_ref(family, n)
    got = _run(_dev(ref.P, cuda), cuda)
    _assert_exact(got, ref, n, (family, n))
    assert got["h2"] == float(ref.h2)
    assert int(got["hist"].reshape(3, 2, -1)[0, 0].sum()) == n * n            # level 0 counts every entry once


# ---------------------------------------------------------------------------------------------------------------
# 2. exact on wide lattices: the k loop, d > 256
# ---------------------------------------------------------------------------------------------------------------
WIDE = ((150, 37), (257, 33), (1536, 130), (700, 300))
_WIDE_REFS = {}


def _wide(n, d):
    if (n, d) not in _WIDE_REFS:
        P = np.random.default_rng([n, d, 3]).integers(0, 4, size=(n, d)).astype(np.int64)
        _WIDE_REFS[(n, d)] = si.LatticeRef(P)
        assert _WIDE_REFS[(n, d)].D.max() <= 2700
    return _WIDE_REFS[(n, d)]


@pytest.mark.parametrize("n,d", WIDE)
def test_exact_on_wide_lattices(cuda, n, d):
    ref = _wide(n, d)
    got = _run(_dev(ref.P, cuda), cuda)
    _assert_exact(got, ref, n, ("wide", n, d))
    scaled = _run(_dev(ref.P, cuda, 2.0 ** -7), cuda)
    _assert_exact(scaled, ref, n, ("wide x 2^-7", n, d), 2.0 ** -14)
    assert scaled["h2"] == got["h2"] * 2.0 ** -14 and scaled["med"] == got["med"] * 2.0 ** -14


# ---------------------------------------------------------------------------------------------------------------
# 3. every tile loop: one workgroup owns all tiles, three share them, more workgroups than tiles
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["wide", "simplex4_128_1"])
def test_every_grid_gives_the_same_counts(cuda, case):
    n = 1536
    ref = _wide(n, 130) if case == "wide" else si.lattice_ref(case, n)
    T = _dev(ref.P, cuda)
    base = _run(T, cuda)
    _assert_exact(base, ref, n, (case, "default grid"))
    assert _lib.stream_median_plan(n, T.shape[1])[2:] == (78, 78)
    try:
        for grid in (1, 3, 4096):
            _lib.debug_stream_median_grid(grid)
            assert _lib.stream_median_plan(n, T.shape[1])[3] == grid
            got = _run(T, cuda)
            _assert_exact(got, ref, n, (case, grid))
            assert _same(got, base), (case, grid)
    finally:
        _lib.debug_stream_median_grid(0)


def test_one_workgroup_flushes_before_its_counters_could_overflow(cuda):
    """363 row tiles are 66066 tiles: one workgroup that owns them all flushes its 32-bit LDS counters once on the way
    (after 65536 tiles) and once at the end.  Counts are integers: the histograms equal the default grid's to the bit."""
    n, d = 46400, 1
    T = torch.randn(n, d, generator=torch.Generator(device="cpu").manual_seed(11)).to(cuda)
    assert _lib.stream_median_plan(n, d)[2] == 66066 > 65536
    base = _run(T, cuda)
    assert np.isfinite(base["h2"]) and base["h2"] > 0
    assert int(base["hist"].reshape(3, 2, -1)[0, 0].sum()) == n * n
    try:
        _lib.debug_stream_median_grid(1)
        got = _run(T, cuda)
    finally:
        _lib.debug_stream_median_grid(0)
    assert _same(got, base)


# ---------------------------------------------------------------------------------------------------------------
# 4. n = 2 and n = 3, by hand
# ---------------------------------------------------------------------------------------------------------------
def test_two_and_three_particles(cuda):
    # n = 2: the four values are {0, 0, 9, 9}: lo = 0, hi = 9, median 4.5
    got = _run(_dev([[0, 0, 0], [1, 2, 2]], cuda), cuda)
    assert (got["lo"], got["hi"], got["med"]) == (0.0, 9.0, 4.5)
    assert got["h2"] == float(si.bandwidth(np.float32(4.5), 2))
    # n = 3 on a line at 0, 1, 3: {0, 0, 0, 1, 1, 4, 4, 9, 9}, odd total: the fifth value
    got = _run(_dev([[0], [1], [3]], cuda), cuda)
    assert (got["lo"], got["hi"], got["med"]) == (1.0, 1.0, 1.0)
    assert got["h2"] == float(si.bandwidth(np.float32(1.0), 3))


# ---------------------------------------------------------------------------------------------------------------
# 5. normal inputs: against the fp64 median and against a stored-D engine
# ---------------------------------------------------------------------------------------------------------------
NORMAL = list(ts.NORMAL_SHAPES) + [(4096, 64)]
_WORST = {"median": 0.0, "h2": 0.0}


def _normal(n, d):
    """(theta as fp32 values in fp64, fp64 distances) -- test_gpu_stream's inputs and oracle where it has the shape"""
    if (n, d) in ts.NORMAL_SHAPES:
        T64, _, ref = ts._normal_case(n, d)
        return T64, np.asarray(ref["D"], dtype=np.float64)
    T64 = ci.f32(tx._inputs(n, d)[0])
    return T64, orc.pairwise_sq_dists(T64, np.float64)


@pytest.mark.parametrize("n,d", NORMAL)
def test_normal_inputs(cuda, n, d):
    T64, D64 = _normal(n, d)
    med64 = float(np.median(D64))
    T = ts._dev(T64, cuda)
    got = _run(T, cuda)
    allowed = TOL_D * float(np.abs(D64).max())
    e_med = abs(got["med"] - med64)
    stored = SvgdEngine(n, d, device=cuda, small=False)
    stored.compute_phi(T, torch.zeros_like(T))
    h2_stored = float(stored.h2.item())
    e_h2 = abs(got["h2"] - h2_stored)
    _WORST["median"] = max(_WORST["median"], e_med / allowed)
    _WORST["h2"] = max(_WORST["h2"], e_h2 / (TOL_H2 * h2_stored))
    print("stream median %dx%d: median %.9g (fp64 %.9g): error / allowance %.4f;  h2 %.9g (stored-D %.9g): error / allowance "
          "%.4f;  worst so far %.4f, %.4f" % (n, d, got["med"], med64, e_med / allowed, got["h2"], h2_stored,
                                              e_h2 / (TOL_H2 * h2_stored), _WORST["median"], _WORST["h2"]))
    assert e_med <= allowed, (n, d, got["med"], med64, allowed)
    assert e_h2 <= TOL_H2 * h2_stored, (n, d, got["h2"], h2_stored)
    assert got["h2"] == float(si.bandwidth(np.float32(got["med"]), n))        # median_bandwidth, as on every path


# ---------------------------------------------------------------------------------------------------------------
# 6. the workspace carries nothing; a repeated call is bit-identical
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(257, 33), (1536, 256)])
def test_result_does_not_depend_on_what_the_workspace_held(cuda, n, d):
    T = ts._dev(_normal(n, d)[0], cuda)
    ws = torch.zeros(_lib.stream_median_workspace_bytes(n, d), dtype=torch.uint8, device=cuda)
    want = _run(T, cuda, ws)
    assert np.isfinite(want["h2"]) and want["h2"] > 0
    gen = torch.Generator(device="cpu").manual_seed(n + d)
    for name in ("0xFF", "random"):
        for call in range(2):
            if name == "0xFF":
                ws.fill_(0xFF)
            else:
                ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, generator=gen))
            assert _same(_run(T, cuda, ws), want), (n, d, name, call)
    assert _same(_run(T, cuda, ws), want)                                     # straight after a call of its own, too


# ---------------------------------------------------------------------------------------------------------------
# 7. the engine and the sampler
# ---------------------------------------------------------------------------------------------------------------
def test_engine_refreshes_every_third_step(cuda):
    n, d = 700, 300
    T64, G64 = (ci.f32(x) for x in tx._inputs(n, d, 2))
    G = ts._dev(G64, cuda)
    eng = SvgdEngine(n, d, device=cuda, h2="median", median_every=3)
    assert eng.streaming and eng.median_every == 3 and eng.ws_bytes == _lib.stream_workspace_bytes(n, d)
    plain = SvgdEngine(n, d, device=cuda, h2=eng.h2)
    assert plain.h2 is eng.h2 and plain.median_every is None
    seen, held = [], None
    for call in range(7):
        T = ts._dev(T64 * (1.0 + 0.125 * call), cuda)            # the particles spread: the median grows every step
        phi = eng.compute_phi(T, G).clone()
        h2 = float(eng.h2.item())
        seen.append(h2)
        if call % 3 == 0:
            direct = _run(T, cuda)
            assert h2 == direct["h2"] and float(eng.median.item()) == direct["med"], (call, h2, direct["h2"])
            assert held is None or h2 != held, call
            held = h2
        else:
            assert h2 == held, (call, seen)
        assert torch.equal(plain.compute_phi(T, G), phi), call   # the step itself is the streaming step at that h2
        assert torch.equal(plain.sqnorm, eng.sqnorm)
    assert len(set(seen)) == 3, seen
    # on demand, outside the schedule
    T = ts._dev(T64 * 3.0, cuda)
    assert eng.refresh_bandwidth(T) is eng.h2
    assert float(eng.h2.item()) == _run(T, cuda)["h2"]
    with pytest.raises(ValueError, match="median"):
        plain.refresh_bandwidth(T)
    with pytest.raises(ValueError, match="contiguous"):
        eng.refresh_bandwidth(T[:, :10])


def test_sampler_with_the_median_bandwidth(cuda):
    """The logistic-regression example's shape (100 particles x 55 parameters) and model, a few iterations."""
    from stein_amd.optimizers import AdamGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.scores import GlmScore
    spec = importlib.util.spec_from_file_location("logistic_example", os.path.join(ROOT, "examples", "logistic_regression",
                                                                                   "main.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    (Xtr, ytr), _ = ex.make_data(n=2000)
    X, y = torch.tensor(Xtr[:50], dtype=torch.float32, device=cuda), torch.tensor(ytr[:50], dtype=torch.float32, device=cuda)
    model_vars = {"model/w:0": [Xtr.shape[1], 1], "model/log_alpha:0": []}

    def sampler(**kw):
        score = GlmScore("logistic", Xtr.shape[1], w_col=1, alpha_col=0, n_train=len(Xtr))
        return SteinSampler(100, ex.make_log_posterior(len(Xtr), 50), AdamGradientDescent(learning_rate=1e-1), score=score,
                            model_vars=model_vars, device=cuda, seed=4, **kw)

    s, default = sampler(bandwidth="median"), sampler()
    assert s.engine.streaming and s.engine.median_every == 1 and not default.engine.streaming
    assert np.array_equal(s.samples, default.samples) and s.samples.shape == (100, 55)
    s.train_on_batch({"X": X, "y": y})
    default.train_on_batch({"X": X, "y": y})
    h2, h2_default = float(s.engine.h2.item()), float(default.engine.h2.item())
    print("sampler 100x55: first-step h2 %.9g, default sampler %.9g" % (h2, h2_default))
    assert abs(h2 - h2_default) <= TOL_H2 * h2_default
    for _ in range(4):
        s.train_on_batch({"X": X, "y": y})
    assert np.isfinite(s.samples).all() and np.isfinite(float(s.engine.h2.item()))
    assert float(s.engine.h2.item()) != h2                        # refreshed as the particles moved
    every = sampler(bandwidth="median", median_every=5)
    assert every.engine.median_every == 5


# ---------------------------------------------------------------------------------------------------------------
# 8. the memory claim
# ---------------------------------------------------------------------------------------------------------------
def test_large_n_median_in_the_streaming_workspace(cuda):
    n, d = 32768, 64
    gen = torch.Generator(device="cpu").manual_seed(5)
    T = torch.randn(n, d, generator=gen).to(cuda)
    eng = SvgdEngine(n, d, device=cuda, h2="median")
    assert eng.ws_bytes == _lib.stream_workspace_bytes(n, d) < (50 << 20)
    h2 = float(eng.refresh_bandwidth(T).item())
    assert np.isfinite(h2) and h2 > 0
    stored = SvgdEngine(n, d, device=cuda)
    assert stored.ws_bytes > (4 << 30)
    stored.compute_phi(T, torch.zeros_like(T))
    h2_stored = float(stored.h2.item())
    print("stream median %dx%d: workspace %.1f MiB (stored-D %.2f GiB); h2 %.9g, stored-D %.9g: error / allowance %.4f" %
          (n, d, eng.ws_bytes / 2.0 ** 20, stored.ws_bytes / 2.0 ** 30, h2, h2_stored, abs(h2 - h2_stored) / (TOL_H2 * h2_stored)))
    assert abs(h2 - h2_stored) <= TOL_H2 * h2_stored
