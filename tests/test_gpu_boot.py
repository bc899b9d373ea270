"""GPU: the KSD goodness-of-fit test (stein_ksd_boot, include/steinhip.h; stein_amd.utilities.ksd_quadratic_forms and
stein_goodness_of_fit; SteinSampler.goodness_of_fit).

Every quadratic form is checked against the fp64 pair sums of tests/boot_ref.py within the allowance its docstring derives
from the kernel's arithmetic, on a NaN-filled workspace; the exact properties (a negated row, a row's position, a repeat,
every forced j split) bit for bit; the p-values against the fp64 reference's on the cases tests/test_boot_cases.py proves
decisive, with the same weights on both sides.  Measured on the MI355X (largest error over allowance, printed by the tests):
DESIGN.md section 6h.
"""

import numpy as np
import pytest
import torch

import boot_cases as C
import boot_ref as R
from stein_amd import _lib
from stein_amd.engine import HipStages
from stein_amd.utilities import ksd_quadratic_forms, stein_goodness_of_fit
from test_gpu_ksd import TOL_F32

pytestmark = pytest.mark.gpu
KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _forms(T, G, h2, kernel, W, jsplit=0, want_diag=True, fill=float("nan")):
    """the C call on device tensors, on a workspace filled with `fill` -> (q, diag) as NumPy (diag None without it)"""
    n, d = T.shape
    reps = W.shape[0]
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=T.device)
    q = torch.full((reps,), float("nan"), dtype=torch.float64, device=T.device)
    diag = torch.full((1,), float("nan"), dtype=torch.float64, device=T.device) if want_diag else None
    _lib.debug_boot_jsplit(jsplit)
    try:
        ws = torch.full((_lib.ksd_boot_workspace_bytes(n, d, reps) // 4,), fill, dtype=torch.float32, device=T.device)
        HipStages().ksd_boot(T, G, n, d, h2_t, KERNEL_IDS[kernel], W, reps, q, diag, ws.view(torch.uint8))
    finally:
        _lib.debug_boot_jsplit(0)
    torch.cuda.synchronize()
    return q.cpu().numpy(), float(diag.item()) if want_diag else None


def _check(tag, q, f):
    ratio = np.abs(q - f.q) / f.allow
    print("boot %s: largest |err| / allowance %.3g  (allowance / scale %.3g)" % (tag, ratio.max(), (f.allow / f.scale).max()))
    assert np.isfinite(q).all(), tag
    assert (ratio <= 1.0).all(), (tag, np.flatnonzero(ratio > 1.0), ratio.max())


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_case_table(cuda, name):
    c = C.BY_NAME[name]
    X, G, h2, W, f = C.reference(name)
    T, S, Wd = _dev(cuda, X, G, W)
    q, diag = _forms(T, S, h2, c.kernel, Wd)
    _check(name, q, f)
    assert abs(diag - f.diag) <= (c.d + 8) * 2.0 ** -50 * f.diag
    q_zero, _ = _forms(T, S, h2, c.kernel, Wd, fill=0.0)           # whatever the workspace held: the same bits
    assert np.array_equal(q, q_zero)
    for k in c.splits():                                           # every j split: within the allowance, the same bits again
        qk, dk = _forms(T, S, h2, c.kernel, Wd, jsplit=k)
        _check("%s jsplit %d" % (name, k), qk, f)
        qk2, dk2 = _forms(T, S, h2, c.kernel, Wd, jsplit=k)
        assert np.array_equal(qk, qk2) and dk == dk2 == diag, k
    if c.pvalue:                                                   # decisive in fp64: the same p-value, replicate by replicate
        assert np.array_equal(q[1:] >= q[0], f.q[1:] >= f.q[0])
        assert R.p_value(q) == R.p_value(f.q)


def _h_of(h2):
    """a float h whose square rounds to the fp32 value h2 (what bandwidth=h hands the library)"""
    h = float(np.sqrt(h2))
    for _ in range(8):
        if R.f32(h * h) == h2:
            return h
        h = float(np.nextafter(h, np.inf if R.f32(h * h) < h2 else -np.inf))
    raise AssertionError("no float squares to %r in fp32" % h2)


@pytest.mark.parametrize("name", ["129x33_r33_imq", "129x33_r33_rbf", "300x260_r129_imq", "300x260_r129_rbf", "257x33_r257_rbf"])
def test_ones_row_against_the_discrepancy_that_predates_the_test(cuda, name):
    """row 0 is all ones: Q_0 = n^2 KSD^2_V, which kernelized_stein_discrepancy gives by the streaming step's row sums --
    within that call's own tolerance (TOL_F32 of the magnitudes' sum) plus the allowance"""
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    c = C.BY_NAME[name]
    X, G, h2, W, f = C.reference(name)
    T, S, Wd = _dev(cuda, X, G, W)
    q, _ = _forms(T, S, h2, c.kernel, Wd)
    got = ksd(T, S, "v", bandwidth=_h_of(h2), kernel=c.kernel) * c.n ** 2
    err, tol = abs(got - q[0]), f.allow[0] + TOL_F32 * f.scale[0]
    print("boot %s: |n^2 KSD^2_V - Q_0| / tolerance %.3g" % (name, err / tol))
    assert err <= tol


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_negated_and_repeated_rows_give_the_same_bits(cuda, kernel):
    """Q is even in the row, bit for bit, and does not depend on the row's
    position: column 1 against column 200 (another wave, another 128-block) and column 300 (another workgroup).
    (The matrix cores' sums are not sign-symmetric: contracted as given, the negated row came out one ulp of one fp32
    partial away, 1792.0936050415039 against 1792.093635559082.  stein_ksd_boot contracts every row in the sign that makes
    its first nonzero entry positive, so the two are one operand.)"""
    rng = np.random.default_rng(11)
    n, d, reps = 257, 7, 301
    X = (rng.standard_normal((n, d)) + 0.2).astype(np.float32)
    G = (-X + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    W = R.sign_rows(reps, n, 12)
    W[2] = rng.standard_normal(n).astype(np.float32) * 0.5          # general weights within the signs' magnitude
    W[200], W[300], W[37], W[150] = W[1], W[1], -W[1], -W[2]
    h2 = R.median_h2(X)
    T, S, Wd = _dev(cuda, X, G, W)
    q, _ = _forms(T, S, h2, kernel, Wd)
    _check("257x7 r301 %s" % kernel, q, R.quadratic_forms(X, G, h2, kernel, W))
    q2, _ = _forms(T, S, h2, kernel, Wd)
    assert np.array_equal(q, q2)
    print("boot 257x7 r301 %s: row 1 %.17g, at column 200 %.17g, at column 300 %.17g, negated %.17g; row 2 %.17g, negated %.17g"
          % (kernel, q[1], q[200], q[300], q[37], q[2], q[150]))
    assert q[1] == q[200] and q[1] == q[300], "the same row at another column"
    assert q[1] == q[37] and q[2] == q[150], "a negated row"


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("exp", [10, -10])
def test_scores_of_any_range(cuda, kernel, exp):
    """scores times 2^10: u_p reaches 10^6 and more, beyond fp16 -- a missing image scale gives inf; times 2^-10: the
    score terms fall 2^-20 below the kernel's own"""
    rng = np.random.default_rng(21)
    n, d, reps = 200, 5, 40
    X = rng.standard_normal((n, d)).astype(np.float32)
    G = (-X * 2.0 ** exp).astype(np.float32)
    W = R.sign_rows(reps, n, 22)
    W[0] = 1.0
    h2 = R.median_h2(X)
    U = R.pairwise_u(X, G, h2, kernel)
    if exp > 0:
        assert np.abs(U).max() > 65504.0
    T, S, Wd = _dev(cuda, X, G, W)
    q, _ = _forms(T, S, h2, kernel, Wd)
    _check("200x5 scores x 2^%d %s" % (exp, kernel), q, R.quadratic_forms(X, G, h2, kernel, W))


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_misaligned_bases_and_no_diagonal(cuda, kernel):
    """theta, score and the weights 4 bytes past a 16-byte boundary (d % 4 == 0: the split's 16-byte loads must not be taken);
    diag_out = NULL gives the same Q"""
    rng = np.random.default_rng(31)
    n, d, reps = 150, 8, 36
    X = (rng.standard_normal((n, d)) + 0.1).astype(np.float32)
    G = -X
    W = R.sign_rows(reps, n, 32)
    W[0] = 1.0
    h2 = R.median_h2(X)
    f = R.quadratic_forms(X, G, h2, kernel, W)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device=cuda)
        buf[1:] = torch.from_numpy(a.reshape(-1)).to(cuda)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4
        return v
    T, S, Wd = _dev(cuda, X, G, W)
    q, _ = _forms(T, S, h2, kernel, Wd)
    qs, _ = _forms(shifted(X), shifted(G), h2, kernel, shifted(W))
    _check("150x8 misaligned %s" % kernel, qs, f)
    q_nodiag, none = _forms(T, S, h2, kernel, Wd, want_diag=False)
    assert none is None and np.array_equal(q, q_nodiag)


def test_python_forms_and_u_statistic(cuda):
    c = C.BY_NAME["129x33_r33_imq"]
    X, G, h2, W, f = C.reference(c.name)
    T, S, Wd = _dev(cuda, X, G, W)
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=cuda)
    q, diag = ksd_quadratic_forms(T, S, Wd, bandwidth=h2_t, kernel="imq")
    assert q.dtype == torch.float64 and q.shape == (33,) and diag.shape == (1,) and q.is_cuda
    _check("python forms", q.cpu().numpy(), f)
    # weights=: the caller's rows behind the all-ones row -> the same Q, both statistics from it
    sv, pv, reps_v = stein_goodness_of_fit(T, S, n_boot=32, bandwidth=h2_t, weights=Wd[1:].contiguous(), return_samples=True)
    n = c.n
    assert abs(sv - f.q[0] / n ** 2) <= f.allow[0] / n ** 2
    assert np.all(np.abs(reps_v.cpu().numpy() * n ** 2 - f.q[1:]) <= f.allow[1:])
    # the U-statistic: sign rows, the diagonal removed from the statistic and from every replicate
    gen = torch.Generator(device=cuda).manual_seed(5)
    su, pu, reps_u = stein_goodness_of_fit(T, S, n_boot=31, bandwidth=h2_t, statistic="u", generator=gen, return_samples=True)
    assert abs(su - (f.q[0] - f.diag) / (n * (n - 1))) <= (f.allow[0] + 1e-12 * f.diag) / (n * (n - 1))
    gen = torch.Generator(device=cuda).manual_seed(5)
    sv2, pv2, reps_v2 = stein_goodness_of_fit(T, S, n_boot=31, bandwidth=h2_t, statistic="v", generator=gen, return_samples=True)
    assert torch.allclose(reps_u * (n * (n - 1)) + diag, reps_v2 * n ** 2, rtol=1e-12, atol=0)
    assert 0.0 < pu <= 1.0 and 0.0 < pv2 <= 1.0 and 0.0 < pv <= 1.0


def test_p_value_through_python_matches_the_reference(cuda):
    """the decisive cases through the public function, with the reference's weights: the fp64 p-value exactly"""
    for c in C.P_CASES:
        X, G, h2, W, f = C.reference(c.name)
        T, S, Wd = _dev(cuda, X, G, W)
        stat, p = stein_goodness_of_fit(T, S, n_boot=c.reps - 1, bandwidth=_h_of(h2), kernel=c.kernel, weights=Wd[1:].contiguous())
        print("boot %s: p %.4f  (fp64 %.4f)" % (c.name, p, R.p_value(f.q)))
        assert p == R.p_value(f.q)
        assert abs(stat - f.q[0] / c.n ** 2) <= f.allow[0] / c.n ** 2
        if c.pvalue == "shift":
            assert p == 1.0 / c.reps
    # and with the library's own signs and bandwidth: the shifted sample is rejected, the null sample is not
    X, G, _, _, _ = C.reference("192x3_r256_imq_shift")
    T, S = _dev(cuda, X, G)
    assert stein_goodness_of_fit(T, S, n_boot=199)[1] == 1.0 / 200
    X0 = np.random.default_rng(3).standard_normal((192, 3)).astype(np.float32)
    T0, S0 = _dev(cuda, X0, -X0)
    assert stein_goodness_of_fit(T0, S0, n_boot=199, generator=torch.Generator(device=cuda).manual_seed(1))[1] > 0.02


def test_flip_prob_and_generator(cuda):
    from stein_amd.utilities.stein_test import sign_processes
    g = torch.Generator(device=cuda).manual_seed(9)
    w = sign_processes(64, 4000, 0.5, cuda, g)
    assert w.dtype == torch.float32 and w.shape == (64, 4000) and set(torch.unique(w).tolist()) == {-1.0, 1.0}
    assert abs(float((w[:, 1:] != w[:, :-1]).float().mean()) - 0.5) < 0.01
    assert abs(float(w[:, 0].mean())) < 0.5
    w = sign_processes(64, 4000, 0.1, cuda, g)
    assert abs(float((w[:, 1:] != w[:, :-1]).float().mean()) - 0.1) < 0.01
    X = np.random.default_rng(8).standard_normal((130, 4)).astype(np.float32)
    T, S = _dev(cuda, X, -X)
    runs = []
    for seed in (7, 7, 8):
        g = torch.Generator(device=cuda).manual_seed(seed)
        s, p, r = stein_goodness_of_fit(T, S, n_boot=63, flip_prob=0.2, generator=g, return_samples=True, kernel="rbf")
        runs.append((s, p, r.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    assert runs[0][0] == runs[2][0] and not np.array_equal(runs[0][2], runs[2][2])       # the statistic has no randomness


def test_sampler_goodness_of_fit_on_the_linear_regression_fixture(cuda, golden):
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
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
    for kw in ({}, {"kernel": "rbf"}, {"bandwidth": 0.02, "statistic": "u", "flip_prob": 0.3}):
        got = s.goodness_of_fit(n_boot=63, generator=torch.Generator(device=cuda).manual_seed(2), **kw)
        want = stein_goodness_of_fit(T32, G32, n_boot=63, generator=torch.Generator(device=cuda).manual_seed(2), **kw)
        assert got == want and len(got) == 2 and 0.0 < got[1] <= 1.0, kw
    assert torch.equal(s.theta_matrix, before)             # the test moves nothing
    f = R.quadratic_forms(T32.cpu().numpy(), G32.cpu().numpy(), R.f32(0.02 ** 2), "imq", np.ones((1, n), np.float32))
    stat = s.goodness_of_fit(n_boot=63, bandwidth=0.02)[0]
    assert abs(stat - f.q[0] / n ** 2) <= f.allow[0] / n ** 2
