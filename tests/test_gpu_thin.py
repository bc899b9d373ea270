"""GPU: Stein thinning (stein_thin, include/steinhip.h; stein_amd.utilities.stein_thinning; SteinSampler.thin).

The picks are checked teacher-forced against the fp64 loop of tests/thin_ref.py, whose docstring derives the allowance: given
the GPU's own sequence, every pick lies within allow_t of the fp64 minimum and equals the fp64 argmin on every decisive
step (at least 3/4 of the steps of every case: tests/test_thin_cases.py); ksd2_out is the fp64 V-statistic of those picks
within the same allowance, and the existing kernelized_stein_discrepancy of the picked rows agrees with it.  Measured on the
MI355X (largest over the table, printed by the tests): DESIGN.md section 6g.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import thin_cases as C
import thin_ref as R
import workspace_state as wst
from stein_amd import _lib
from stein_amd.engine import HipStages
from test_gpu_ksd import TOL_F32

pytestmark = pytest.mark.gpu
ALL = [(c.name, k) for c in C.CASES for k in R.KERNELS]
KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _thin(T, G, h2, kernel, m, grid=0, want_ksd=True, ws=None):
    """the C call on device tensors -> (idx, ksd2) as NumPy (ksd2 None without it)"""
    n, d = T.shape
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=T.device)
    if ws is None:
        ws = torch.zeros(_lib.thin_workspace_bytes(n, d), dtype=torch.uint8, device=T.device)
    idx = torch.full((m,), -7, dtype=torch.int64, device=T.device)
    ksd2 = torch.full((m,), float("nan"), dtype=torch.float64, device=T.device) if want_ksd else None
    _lib.debug_thin_grid(grid)
    try:
        HipStages().thin(T, G, n, d, h2_t, KERNEL_IDS[kernel], m, idx, ksd2, ws)
    finally:
        _lib.debug_thin_grid(0)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), ksd2.cpu().numpy() if want_ksd else None


def _check_forced(tag, X, G, h2, kernel, idx, ksd2):
    """the teacher-forced check and the running statistic; returns thin_ref.teacher_forced of the GPU's picks"""
    n = X.shape[0]
    assert idx.min() >= 0 and idx.max() < n, tag
    f = R.teacher_forced(X, G, h2, kernel, idx)
    late = f.allow > 0                                   # (the first pick has no kernel row behind it: allow_1 ~ 0, gap_1 = 0)
    r_gap = float((f.gap[late] / f.allow[late]).max()) if late.any() else 0.0
    r_ksd = float((np.abs(ksd2 - f.ksd2) / f.ksd2_allow).max())
    print("thin %s: decisive %.3f  largest gap / allow_t %.3g  largest |ksd2 err| / allowance %.3g" %
          (tag, f.decisive.mean(), r_gap, r_ksd))
    assert (f.gap <= f.allow).all(), (tag, np.flatnonzero(f.gap > f.allow))
    assert (idx[f.decisive] == f.argmin[f.decisive]).all(), (tag, np.flatnonzero(f.decisive & (idx != f.argmin)))
    assert f.decisive.mean() >= C.DECISIVE_SHARE, tag
    assert (np.abs(ksd2 - f.ksd2) <= f.ksd2_allow).all(), tag
    return f


@pytest.mark.parametrize("name,kernel", ALL)
def test_case_table(cuda, name, kernel):
    c = C.BY_NAME[name]
    X, G, h2, ref_picks, _ = C.reference(name, kernel)
    T, S = _dev(cuda, X, G)
    n, d = X.shape
    idx, ksd2 = _thin(T, S, h2, kernel, c.m)
    _check_forced("%s %s" % (name, kernel), X, G, h2, kernel, idx, ksd2)
    if n == 1:
        assert (idx == 0).all()
    if c.m > n:
        assert len(set(idx.tolist())) < c.m
    if c.dup:                 # equal objectives: never the copy
        assert idx.max() < c.n and np.isin(idx, c.dup).sum() >= 3
    for grid in C.grids(n, d):            # the cross-workgroup argmin at any grid: the same bits
        i2, k2 = _thin(T, S, h2, kernel, c.m, grid=grid)
        assert np.array_equal(i2, idx) and np.array_equal(k2, ksd2), grid


def _h_of(h2):
    """a float h whose square rounds to the fp32 value h2 (what bandwidth=h hands the library)"""
    h = float(np.sqrt(h2))
    for _ in range(8):
        if R.f32(h * h) == h2:
            return h
        h = float(np.nextafter(h, np.inf if R.f32(h * h) < h2 else -np.inf))
    raise AssertionError("no float squares to %r in fp32" % h2)


@pytest.mark.parametrize("name", ["20x3_m40", "50x6_m24_dup", "513x33_m64", "257x130_m64", "2500x7_m40"])
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_final_statistic_against_the_discrepancy_that_predates_thinning(cuda, name, kernel):
    """ksd2_out[m - 1] is the V-statistic of the picked rows, repeats included: kernelized_stein_discrepancy of theta[idx],
    score[idx] at the same bandwidth, within that call's own tolerance (TOL_F32 of the magnitudes' sum) and the allowance"""
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    c = C.BY_NAME[name]
    X, G, h2, _, _ = C.reference(name, kernel)
    T, S = _dev(cuda, X, G)
    idx, ksd2 = _thin(T, S, h2, kernel, c.m)
    f = R.teacher_forced(X, G, h2, kernel, idx)
    sel = torch.from_numpy(idx).to(cuda)
    got = ksd(T[sel].contiguous(), S[sel].contiguous(), "v", bandwidth=_h_of(h2), kernel=kernel)
    err, tol = abs(got - ksd2[-1]), f.ksd2_allow[-1] + TOL_F32 * f.scale[-1] / c.m ** 2
    print("thin %s %s: |KSD^2_V of theta[idx] - ksd2_out[m - 1]| / tolerance %.3g" % (name, kernel, err / tol))
    assert err <= tol


@pytest.mark.parametrize("name,kernel", [("2500x7_m40", "imq"), ("96x515_m32", "rbf"), ("80x256_m16", "imq"),
                                         ("20x3_m40", "rbf")])
def test_bit_identical(cuda, name, kernel):
    c = C.BY_NAME[name]
    X, G, h2, _, _ = C.reference(name, kernel)
    T, S = _dev(cuda, X, G)
    n, d = X.shape
    idx, ksd2 = _thin(T, S, h2, kernel, c.m)
    for _ in range(2):                                     # on repeat
        i2, k2 = _thin(T, S, h2, kernel, c.m)
        assert np.array_equal(i2, idx) and np.array_equal(k2, ksd2)
    ws = torch.empty(_lib.thin_workspace_bytes(n, d), dtype=torch.uint8, device=cuda)
    for pattern in ("ones", "large"):                      # on a workspace of NaNs, of huge values
        wst.poison(types.SimpleNamespace(ws=ws, _offs=[0] * _lib.WS_NSECTIONS), pattern, keep_select=False)
        i2, k2 = _thin(T, S, h2, kernel, c.m, ws=ws)
        assert np.array_equal(i2, idx) and np.array_equal(k2, ksd2), pattern
    i2, k2 = _thin(T, S, h2, kernel, c.m, want_ksd=False)  # with ksd2_out = NULL
    assert k2 is None and np.array_equal(i2, idx)
    for m in (1, 5):                                       # every prefix is the greedy choice of its own length
        i2, k2 = _thin(T, S, h2, kernel, m)
        assert np.array_equal(i2, idx[:m]) and np.array_equal(k2, ksd2[:m])


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_rows_that_do_not_start_on_16_bytes_take_the_4_byte_arm(cuda, kernel):
    X, G, h2, _, _ = C.reference("90x8_m16", kernel)
    n, d = X.shape
    bufs = [torch.zeros(n * d + 1, dtype=torch.float32, device=cuda) for _ in range(2)]
    T, S = (b[1:].view(n, d) for b in bufs)
    T.copy_(torch.from_numpy(X)), S.copy_(torch.from_numpy(G))
    assert T.data_ptr() % 16 == 4 and T.is_contiguous() and C.arm(d, aligned=False) == (False, 8, 1)
    idx, ksd2 = _thin(T, S, h2, kernel, 16)
    _check_forced("90x8 off 16 bytes %s" % kernel, X, G, h2, kernel, idx, ksd2)


def test_bandwidth_forms(cuda):
    from stein_amd.stream_engine import StreamEngine
    from stein_amd.utilities import stein_thinning
    X, G, _, _, _ = C.reference("300x5_m64", "imq")
    T, S = _dev(cuda, X, G)
    n, d = X.shape
    h2 = StreamEngine(n, d, device=cuda, h2="median").refresh_bandwidth(T).clone()
    for kernel in R.KERNELS:
        idx, ksd2 = stein_thinning(T, S, 32, kernel=kernel, return_ksd=True)          # bandwidth="median"
        assert idx.dtype == torch.int64 and idx.shape == (32,) and idx.device == T.device
        assert ksd2.dtype == torch.float64 and ksd2.shape == (32,) and ksd2.device == T.device
        i2, k2 = stein_thinning(T, S, 32, bandwidth=h2, kernel=kernel, return_ksd=True)
        assert torch.equal(i2, idx) and torch.equal(k2, ksd2)
        assert torch.equal(stein_thinning(T, S, 32, bandwidth=h2, kernel=kernel), idx)  # a tensor alone without return_ksd
        i3 = stein_thinning(T, S, 32, bandwidth=_h_of(float(h2.item())), kernel=kernel)
        assert torch.equal(i3, idx)
        _check_forced("utility %s" % kernel, X, G, float(h2.item()), kernel, idx.cpu().numpy(), ksd2.cpu().numpy())
    assert not torch.equal(stein_thinning(T, S, 32, kernel="rbf"), stein_thinning(T, S, 32))     # the default is "imq"
    with pytest.raises(ValueError, match="n >= 2"):
        stein_thinning(T[:1], S[:1], 3)
    assert stein_thinning(T[:1], S[:1], 3, bandwidth=1.0).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="float32"):
        stein_thinning(T.bfloat16(), S.bfloat16(), 3)
    with pytest.raises(ValueError, match="m must be"):
        stein_thinning(T, S, 0)


def test_sampler_thin_on_the_linear_regression_fixture(cuda, golden):
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.utilities import stein_thinning
    g = golden("g6_linear_regression.npz")
    Xd, y = torch.tensor(g["X"], dtype=torch.float64), torch.tensor(g["y"], dtype=torch.float64)
    A, b = float((Xd * Xd).sum()), float((Xd[:, 0] * y).sum())

    def score(theta, feed):
        return b - (A + 1.0) * theta

    n = 50
    T0 = np.random.default_rng(5).normal(size=(n, 1)) * 0.01
    s = SteinSampler(n, None, AdagradGradientDescent(learning_rate=1e-3), theta=T0.copy(), score=score, device=cuda,
                     dtype=torch.float64, bandwidth="median", kernel="imq")
    for _ in range(5):
        s.train_on_batch(None)
    before = s.theta_matrix.clone()
    T32, G32 = s._matrix_f32(), s.score_matrix(None)
    for kw in ({}, {"kernel": "rbf"}, {"bandwidth": 0.02}):
        idx, ksd2 = s.thin(12, return_ksd=True, **kw)
        want_i, want_k = stein_thinning(T32, G32, 12, return_ksd=True, **kw)
        assert torch.equal(idx, want_i) and torch.equal(ksd2, want_k), kw
        assert torch.equal(s.thin(12, **kw), idx)
    assert torch.equal(s.theta_matrix, before)             # thinning moves nothing
    f = R.teacher_forced(T32.cpu().numpy(), G32.cpu().numpy(), R.f32(0.02 ** 2), "imq", idx.cpu().numpy())
    assert (f.gap <= f.allow).all() and (np.abs(ksd2.cpu().numpy() - f.ksd2) <= f.ksd2_allow).all()


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_thinned_set_beats_the_first_m(cuda, kernel):
    c = C.BY_NAME["2500x7_m40"]
    X, G, h2, _, _ = C.reference(c.name, kernel)
    T, S = _dev(cuda, X, G)
    idx, ksd2 = _thin(T, S, h2, kernel, c.m)
    first = R.teacher_forced(X, G, h2, kernel, np.arange(c.m)).ksd2[-1]
    print("thin 2500x7 %s: KSD^2_V of the %d picks %.4e, of theta[:%d] %.4e" % (kernel, c.m, ksd2[-1], c.m, first))
    assert ksd2[-1] < first
    assert (np.diff(ksd2[5:]) < 0).mean() > 0.8            # and it falls as the set grows
