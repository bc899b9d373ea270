"""GPU: Stein importance weights (stein_weights, include/steinhip.h; stein_amd.utilities.stein_importance_weights;
SteinSampler.importance_weights).

The steps are checked teacher-forced against the fp64 replay of tests/weights_ref.py, whose docstring derives every allowance:
given the GPU's own vertices and step lengths, every vertex lies within allow_t of the fp64 minimum of g and equals the fp64
argmin on every decisive step (at least 9/10 of the steps of every case: tests/test_weights_cases.py), and every step length
lies in the interval the allowances leave it; stats_out is the fp64 certificate of w_out within the fresh product's allowance;
on a NaN-filled workspace, with guard values behind every output.  Measured on the MI355X (largest over the table, printed by
the tests): DESIGN.md section 6i.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import weights_cases as C
import weights_ref as R
from stein_amd import _lib
from stein_amd.engine import HipStages
from stein_amd.utilities import stein_importance_weights

pytestmark = pytest.mark.gpu
KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}
GUARD = 8


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _weights(T, G, h2, kernel, iters, grid=0, path=True, fill=float("nan")):
    """the C call on device tensors, on a workspace filled with `fill` -> (w, stats, idx, gamma) as NumPy (idx, gamma None
    without the path); every output has GUARD elements behind it that must stay"""
    n, d = T.shape
    dev = T.device
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=dev)
    w = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((3 + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    idx = torch.full((iters + GUARD,), -7, dtype=torch.int64, device=dev)
    gamma = torch.full((iters + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    for t, k in ((w, n), (stats, 3), (gamma, iters)):
        t[k:] = -12345.0
    _lib.debug_weights_grid(grid)
    try:
        ws = torch.full((_lib.weights_workspace_bytes(n, d) // 4,), fill, dtype=torch.float32, device=dev)
        HipStages().weights(T, G, n, d, h2_t, KERNEL_IDS[kernel], iters, w, stats, idx if path else None, gamma if path else None,
                            ws.view(torch.uint8))
    finally:
        _lib.debug_weights_grid(0)
    torch.cuda.synchronize()
    assert (w[n:] == -12345.0).all() and (stats[3:] == -12345.0).all() and (gamma[iters:] == -12345.0).all() and \
        (idx[iters:] == -7).all(), "a guard behind an output was written"
    if not path:
        assert (idx == -7).all() and bool(torch.isnan(gamma[:iters]).all())
    return (w[:n].cpu().numpy(), stats[:3].cpu().numpy(), idx[:iters].cpu().numpy() if path else None,
            gamma[:iters].cpu().numpy() if path else None)


def _check_weights(tag, iters, w):
    n = w.size
    assert np.isfinite(w).all() and (w >= 0.0).all(), tag
    assert abs(w.sum() - 1.0) <= (iters + n) * 2.0 ** -50, (tag, w.sum() - 1.0)


def _check_certificate(tag, m, w, stats, f_uniform=None):
    (f, gap), (a_f, a_gap) = R.certificate(m, w)
    n = m.n
    uni = np.full(n, 1.0 / n)
    (fu, _), (a_u, _) = R.certificate(m, uni)
    print("weights %s: |f err| / allowance %.3g  |gap err| / allowance %.3g  |f(uniform) err| / allowance %.3g;  f %.4e  gap %.3e"
          "  f(uniform) %.4e" % (tag, abs(stats[0] - f) / a_f, abs(stats[1] - gap) / a_gap, abs(stats[2] - fu) / a_u, f, gap, fu))
    assert abs(stats[0] - f) <= a_f and abs(stats[1] - gap) <= a_gap and abs(stats[2] - fu) <= a_u, tag
    assert gap >= -a_gap and stats[1] >= -a_gap
    return f, fu


def _check_forced(tag, m, idx, gamma, w, share=C.DECISIVE_SHARE):
    """the teacher-forced check of the vertices and step lengths, and w_out against the replay of the same steps; share: the
    decisive share the inputs were proven to have (0: inputs nobody chose, every other check still holds)"""
    f = R.teacher_forced(m, idx, gamma)
    late = f.allow > 0
    r_gap = float((f.gap[late] / f.allow[late]).max()) if late.any() else 0.0
    width = f.g_hi - f.g_lo
    mid = 0.5 * (f.g_hi + f.g_lo)
    r_gam = float((np.abs(gamma - mid) / np.maximum(0.5 * width, 1e-300)).max())
    print("weights %s: decisive %.3f  largest gap / allow_t %.3g  largest |gamma - centre| / half width %.3g  (widest interval %.3g)"
          % (tag, f.decisive.mean(), r_gap, r_gam, width.max()))
    assert (f.gap <= f.allow).all(), (tag, np.flatnonzero(f.gap > f.allow))
    assert (idx[f.decisive] == f.argmin[f.decisive]).all(), (tag, np.flatnonzero(f.decisive & (idx != f.argmin)))
    assert f.decisive.mean() >= share, tag
    assert ((gamma >= f.g_lo) & (gamma <= f.g_hi)).all(), (tag, np.flatnonzero((gamma < f.g_lo) | (gamma > f.g_hi)))
    assert np.abs(w - f.w).max() <= (idx.size + 4) * 2.0 ** -50, tag       # the same updates in fp64, rounding apart
    return f


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_case_table(cuda, name):
    c = C.BY_NAME[name]
    r = C.reference(name)
    T, S = _dev(cuda, r.X, r.G)
    n, d = r.X.shape
    w, stats, idx, gamma = _weights(T, S, r.h2, c.kernel, c.iters)
    _check_weights(name, c.iters, w)
    f, fu = _check_certificate(name, r.model, w, stats)
    if c.iters == 0:
        assert (w == 1.0 / n).all() and stats[0] == stats[2] and idx.size == 0
    else:
        assert idx.min() >= 0 and idx.max() < n and (gamma >= 0.0).all() and (gamma <= 1.0).all()
        _check_forced(name, r.model, idx, gamma, w)
        assert f < fu and stats[0] < stats[2]
    if c.kind == "near":                    # all the mass to one vertex, then converged
        assert gamma[0] == 1.0 and (gamma[1:] == 0.0).all() and (w == (np.arange(n) == idx[0])).all()
    if c.dup:                               # equal g: never the copy
        assert idx.max() < c.n and (idx == C.DUP_ROW).sum() >= 1
    for grid in C.grids(n, d):              # any grid: the same bits, the fp64 sums included
        w2, s2, i2, g2 = _weights(T, S, r.h2, c.kernel, c.iters, grid=grid)
        assert np.array_equal(w2, w) and np.array_equal(s2, stats) and np.array_equal(i2, idx) and np.array_equal(g2, gamma), grid


@pytest.mark.parametrize("case", C.PATH_CASES, ids=lambda c: c.name)
def test_four_n_steps_lower_the_discrepancy(cuda, case):
    """the default iteration count: the fp64 f of w_out is below f(uniform), by far more than any allowance"""
    r = C.reference(case.name)
    T, S = _dev(cuda, r.X, r.G)
    n = case.n
    w, stats, _, _ = _weights(T, S, r.h2, case.kernel, 4 * n, path=False)
    _check_weights(case.name, 4 * n, w)
    f, fu = _check_certificate("%s, 4 n steps" % case.name, r.model, w, stats)
    assert f < fu and stats[0] < stats[2]


@pytest.mark.parametrize("name", ["257x17_imq_t64", "300x5_rbf_t8", "24x520_imq_t8", "1300x7_imq_t10"])
def test_bit_identical(cuda, name):
    c = C.BY_NAME[name]
    r = C.reference(name)
    T, S = _dev(cuda, r.X, r.G)
    w, stats, idx, gamma = _weights(T, S, r.h2, c.kernel, c.iters)
    for fill in (float("nan"), 0.0, 1e30, -1.0):        # on repeat, and whatever the workspace held
        w2, s2, i2, g2 = _weights(T, S, r.h2, c.kernel, c.iters, fill=fill)
        assert np.array_equal(w2, w) and np.array_equal(s2, stats) and np.array_equal(i2, idx) and np.array_equal(g2, gamma), fill
    w2, s2, i2, g2 = _weights(T, S, r.h2, c.kernel, c.iters, path=False)      # idx_out = gamma_out = NULL
    assert i2 is None and g2 is None and np.array_equal(w2, w) and np.array_equal(s2, stats)
    for k in (1, 5):                                     # every prefix of the path is the path of its own length
        _, _, i2, g2 = _weights(T, S, r.h2, c.kernel, k)
        assert np.array_equal(i2, idx[:k]) and np.array_equal(g2, gamma[:k])


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_rows_that_do_not_start_on_16_bytes_take_the_4_byte_arm(cuda, kernel):
    c = C.BY_NAME["90x8_imq_t16"]
    X, G, h2 = c.inputs()
    m = R.Model(X, G, h2, kernel)
    n, d = X.shape
    bufs = [torch.zeros(n * d + 1, dtype=torch.float32, device=cuda) for _ in range(2)]
    T, S = (b[1:].view(n, d) for b in bufs)
    T.copy_(torch.from_numpy(X)), S.copy_(torch.from_numpy(G))
    assert T.data_ptr() % 16 == 4 and T.is_contiguous() and C.arm(d, aligned=False) == (False, 8, 1)
    w, stats, idx, gamma = _weights(T, S, h2, kernel, 12)
    _check_weights("90x8 off 16 bytes", 12, w)
    _check_certificate("90x8 off 16 bytes %s" % kernel, m, w, stats)
    _check_forced("90x8 off 16 bytes %s" % kernel, m, idx, gamma, w)


def test_many_batches_per_virtual_workgroup(cuda):
    """n past 1024 x 16 rows at 64 lanes per row: a virtual workgroup takes a second batch.  The fp64 reference of this size
    (the n x n matrix) is out of a test's reach; checked here: the same bits at any grid, w_out is the fp64 replay of the
    reported steps, and the device's own certificate falls"""
    n, d, iters = 16400, 33, 5
    assert C.parts(n, d) == 1024 and n > 1024 * C.rows_per_workgroup(d)
    rng = np.random.default_rng(77)
    X = (1.3 * rng.standard_normal((n, d)) + 0.5).astype(np.float32)
    T, S = _dev(cuda, X, -X)
    w, stats, idx, gamma = _weights(T, S, float(d), "imq", iters)
    _check_weights("16400x33", iters, w)
    for grid in (1, 300, 1024):
        w2, s2, i2, g2 = _weights(T, S, float(d), "imq", iters, grid=grid)
        assert np.array_equal(w2, w) and np.array_equal(s2, stats) and np.array_equal(i2, idx) and np.array_equal(g2, gamma), grid
    ref = np.full(n, 1.0 / n)
    for s, g in zip(idx, gamma):
        ref = (1.0 - g) * ref
        ref[s] += g
    assert np.abs(w - ref).max() <= (iters + 4) * 2.0 ** -50 and (gamma > 0).all() and len(set(idx.tolist())) > 1
    assert 0.0 < stats[0] < stats[2] and stats[1] > 0.0


def test_python_function_and_bandwidth_forms(cuda):
    from stein_amd.stream_engine import StreamEngine
    c = C.BY_NAME["300x5_rbf_t8"]
    r = C.reference(c.name)
    T, S = _dev(cuda, r.X, r.G)
    n, d = r.X.shape
    h2 = StreamEngine(n, d, device=cuda, h2="median").refresh_bandwidth(T).clone()
    for kernel in R.KERNELS:
        w, info = stein_importance_weights(T, S, iters=8, kernel=kernel, return_path=True)          # bandwidth="median"
        assert w.dtype == torch.float64 and w.shape == (n,) and w.device == T.device
        assert set(info) == {"ksd2", "ksd2_uniform", "gap", "idx", "gamma"} and isinstance(info["ksd2"], float)
        assert info["idx"].dtype == torch.int64 and info["idx"].shape == (8,) and info["gamma"].dtype == torch.float64
        w2, info2 = stein_importance_weights(T, S, iters=8, bandwidth=h2, kernel=kernel)
        assert torch.equal(w2, w) and set(info2) == {"ksd2", "ksd2_uniform", "gap"}
        assert all(info2[k] == info[k] for k in info2)
        wc, stats, idx, gamma = _weights(T, S, float(h2.item()), kernel, 8)
        assert np.array_equal(wc, w.cpu().numpy()) and info["ksd2"] == stats[0] and info["gap"] == stats[1] and \
            info["ksd2_uniform"] == stats[2] and np.array_equal(idx, info["idx"].cpu().numpy())
        assert info["ksd2"] < info["ksd2_uniform"]
    w0, info0 = stein_importance_weights(T, S, iters=0, bandwidth=h2)
    assert (w0 == 1.0 / n).all() and info0["ksd2"] == info0["ksd2_uniform"]
    wd, infod = stein_importance_weights(T[:40].contiguous(), S[:40].contiguous(), bandwidth=h2)    # iters=None: 4 n
    wx, infox = stein_importance_weights(T[:40].contiguous(), S[:40].contiguous(), iters=160, bandwidth=h2)
    assert torch.equal(wd, wx) and infod == infox
    with pytest.raises(ValueError, match="float32"):
        stein_importance_weights(T.bfloat16(), S.bfloat16())
    with pytest.raises(ValueError, match="iters must be"):
        stein_importance_weights(T, S, iters=-1)


def test_sampler_importance_weights_on_the_logistic_example(cuda):
    """the logistic example at its default (smallest) size, 100 particles of 55 parameters, stopped early"""
    from stein_amd.optimizers import AdamGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.scores import GlmScore
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("logistic_main", os.path.join(here, "..", "examples", "logistic_regression", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (Xtr, ytr), _ = mod.make_data(n=2000)
    X, y = torch.tensor(Xtr, dtype=torch.float32, device=cuda), torch.tensor(ytr, dtype=torch.float32, device=cuda)
    score = GlmScore("logistic", Xtr.shape[1], w_col=1, alpha_col=0, n_train=len(Xtr))
    torch.manual_seed(0)
    s = SteinSampler(100, None, AdamGradientDescent(learning_rate=1e-1), score=score, device=cuda,
                     model_vars={"model/w:0": [Xtr.shape[1], 1], "model/log_alpha:0": []})
    full = {"X": X, "y": y}
    for _ in range(10):
        s.train_on_batch(full)
    before = s.theta_matrix.clone()
    T32, G32 = s._matrix_f32(), s.score_matrix(full)
    for kw in ({"iters": 40}, {"iters": 40, "kernel": "rbf"}, {"iters": 12, "bandwidth": 2.0, "return_path": True}):
        w, info = s.importance_weights(full, **kw)
        want_w, want = stein_importance_weights(T32, G32, **kw)
        assert torch.equal(w, want_w) and info["ksd2"] == want["ksd2"] and info["gap"] == want["gap"], kw
        assert info["ksd2"] < info["ksd2_uniform"] and abs(float(w.sum()) - 1.0) < 1e-12
    assert torch.equal(s.theta_matrix, before)             # the weights move nothing
    m = R.Model(T32.cpu().numpy(), G32.cpu().numpy(), R.f32(4.0), "imq")
    stats = np.array([info["ksd2"], info["gap"], info["ksd2_uniform"]])
    _check_certificate("sampler 100x55", m, w.cpu().numpy(), stats)
    _check_forced("sampler 100x55", m, info["idx"].cpu().numpy(), info["gamma"].cpu().numpy(), w.cpu().numpy(), share=0.0)
