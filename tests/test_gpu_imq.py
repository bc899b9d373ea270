"""GPU: the streaming step and the Stein discrepancy under the inverse multiquadric kernel (stein_svgd_phi_imq{,_ksd}:
SvgdEngine(kernel="imq"), SteinSampler(kernel="imq"), utilities.kernelized_stein_discrepancy(kernel="imq")) against the fp64
references of tests/imq_ref.py on the device, evaluated at the engine's own h2.

phi, per column:  |err_c| <= TOL (|phi_ref_c| + |rs3 o theta_c| / (c2 n)), TOL = test_gpu_conditioning.TOL = 1e-5 -- the
streaming tests' allowance carried over to the two-term form rs3 theta - K3 theta.
S, S_diag, U, V:  error over imq_ref.pairwise_sums' scale (sum_ij of every term of u_p with its magnitude) <= TOL_F32 =
test_gpu_ksd.TOL_F32 = 1e-6.  The fp32 model of the arithmetic (tests/test_imq_ref.py, CPU) stays below 0.5e-6 at every case
here (at most 3.4e-8), so no case carries a bound of its own:

    case                                   bandwidths              model: phi / allowance   S / scale    bound
    normal (test_gpu_ksd._inputs), SHAPES  median x {0.25, 1, 4}   <= 0.17                  <= 3.4e-8    TOL, TOL_F32
    graded, test_gpu_conditioning.SHAPES   median x {0.25, 1, 4}   <= 0.18                  <= 1.3e-9    TOL, TOL_F32

Every ratio is printed (-s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import imq_ref as R  # noqa: E402
from test_gpu_conditioning import SHAPES as GRADED_SHAPES, TOL  # noqa: E402
from test_gpu_ksd import TOL_F32, _inputs  # noqa: E402

from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (20, 3), (128, 128), (129, 129), (150, 37), (257, 256), (300, 260), (384, 513), (1000, 40), (1536, 130),
          (4096, 256)]


def _f32(x):
    return float(np.float32(x))


def _imq(n, d, cuda, h2):
    eng = SvgdEngine(n, d, device=cuda, h2=h2, kernel="imq")
    assert eng.streaming and eng.kernel == "imq" and (eng.row_tiles, eng.col_groups) == ((n + 127) // 128, (d + 127) // 128)
    return eng


def _median_h2(T, cuda):
    """the streaming median's h2 of T, as a float"""
    n, d = T.shape
    return float(_imq(n, d, cuda, "median").refresh_bandwidth(T).item())


def _run(eng, T, G):
    """one discrepancy call -> clones of (phi, sums, h2)"""
    phi = eng.compute_phi(T, G, discrepancy=True)
    torch.cuda.synchronize()
    return phi.clone(), eng._sums.clone(), eng.h2.clone()


def _check(tag, eng, T, G, phi, sums=True):
    """phi and (sums) the three doubles of the engine's last call against fp64 at the engine's h2; prints and asserts;
    returns the fp64 (U, scale)"""
    torch.cuda.synchronize()
    n = T.shape[0]
    h2 = float(eng.h2.item())
    T64, G64 = T.double(), G.double()
    S, Sd, phi_ref, rs3 = R.rowsum_sums(T64, G64, h2)
    assert torch.isfinite(phi).all(), tag
    ratio = (phi.double() - phi_ref).norm(dim=0) / R.phi_allowance(phi_ref, rs3, T64, h2, TOL)
    worst = float(ratio.max())
    sq, sq_ref = float(eng.sqnorm.item()), float((phi_ref * phi_ref).sum())
    if not sums:
        print("imq %s: phi error / allowance %.3f (column %d)" % (tag, worst, int(ratio.argmax())))
        assert worst <= 1.0, (tag, worst)
        assert abs(sq - sq_ref) <= 2e-5 * sq_ref, (tag, sq, sq_ref)
        return None
    S, Sd, scale = R.pairwise_sums(T64, G64, h2)
    got = eng._sums.cpu().tolist()
    v = float(eng.stein_discrepancy("v").item())
    errs = [abs(got[1] - S) / scale, abs(got[2] - Sd) / scale, abs(v - R.statistic(S, Sd, n, "v")) * n * n / scale]
    ref_u = None
    if n > 1:
        u, ref_u = float(eng.stein_discrepancy("u").item()), R.statistic(S, Sd, n, "u")
        errs.append(abs(u - ref_u) * n * (n - 1) / scale)
    print("imq %s: phi error / allowance %.3f (column %d); err/scale S %.2e S_diag %.2e V %.2e U %.2e" %
          ((tag, worst, int(ratio.argmax())) + tuple(errs) + ((0.0,) if n == 1 else ())))
    assert worst <= 1.0, (tag, worst)
    assert abs(sq - sq_ref) <= 2e-5 * sq_ref, (tag, sq, sq_ref)
    assert max(errs) <= TOL_F32, (tag, errs)
    return ref_u, scale


# ---------------------------------------------------------------------------------------------------------------
# 1. parity of phi, S, S_diag, U and V
# ---------------------------------------------------------------------------------------------------------------
def _parity(family, n, d, T, G, cuda):
    med = _median_h2(T, cuda)
    engines = [("median x%g" % m, _imq(n, d, cuda, _f32(med * m))) for m in (0.25, 1.0, 4.0)]
    engines.append(("h2=\"median\"", _imq(n, d, cuda, "median")))
    for tag, eng in engines:
        phi = eng.compute_phi(T, G, discrepancy=True)
        _check("%s %dx%d %s (plan %s)" % (family, n, d, tag, (eng.row_tiles, eng.col_groups, eng.jsplit)), eng, T, G, phi)
    assert engines[3][1].h2.item() == med
    # the bandwidth is the library's: the RBF streaming engine takes the same median of the same distances
    assert SvgdEngine(n, d, device=cuda, h2="median").refresh_bandwidth(T).item() == med


@pytest.mark.parametrize("n,d", SHAPES)
def test_parity_with_fp64(cuda, n, d):
    T, G = _inputs(n, d, n + d, cuda)
    _parity("normal", n, d, T, G, cuda)


@pytest.mark.parametrize("n,d", GRADED_SHAPES)
def test_parity_on_graded_columns(cuda, n, d):
    T64, G64 = ci.make("graded", n, d, 0)
    T = torch.tensor(T64, dtype=torch.float32, device=cuda).contiguous()
    G = torch.tensor(G64, dtype=torch.float32, device=cuda).contiguous()
    _parity("graded", n, d, T, G, cuda)


# ---------------------------------------------------------------------------------------------------------------
# 2. every j split
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(700, 300), (1536, 256)])
def test_every_j_split_is_right_and_deterministic(cuda, n, d):
    T, G = _inputs(n, d, n + d, cuda)
    h2 = _f32(_median_h2(T, cuda))
    seen = set()
    try:
        for want in (1, 2, 3, 4, 6):
            _lib.debug_stream_jsplit(want)
            eng = _imq(n, d, cuda, h2)
            if (n, d) == (700, 300):                       # six j tiles: 4 asks for ranges of two, three ranges
                assert eng.jsplit == {1: 1, 2: 2, 3: 3, 4: 3, 6: 6}[want]
            phi, sums, _ = _run(eng, T, G)
            _check("%dx%d jsplit %d (asked %d)" % (n, d, eng.jsplit, want), eng, T, G, phi)
            again = _run(eng, T, G)
            assert torch.equal(again[0], phi) and torch.equal(again[1], sums), (want, "repeat")
            plain = _imq(n, d, cuda, h2)
            p0 = plain.compute_phi(T, G)
            torch.cuda.synchronize()
            assert torch.equal(p0, phi) and torch.equal(plain.sqnorm, sums[:1]), (want, "plain")
            seen.add(eng.jsplit)
    finally:
        _lib.debug_stream_jsplit(0)
    assert {1, 2, 3, 6} <= seen


# ---------------------------------------------------------------------------------------------------------------
# 3. bit identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,h2", [(150, 37, 11.5), (1000, 40, "median"), (300, 260, 80.0)])
def test_keyword_leaves_the_step_bit_identical(cuda, n, d, h2):
    T, G = _inputs(n, d, 7, cuda)
    plain, withk = _imq(n, d, cuda, h2), _imq(n, d, cuda, h2)
    p0 = plain.compute_phi(T, G).clone()
    p1, sums, _ = _run(withk, T, G)
    assert torch.equal(p0, p1) and torch.equal(plain.sqnorm, withk.sqnorm) and torch.equal(plain.h2, withk.h2)
    assert withk.sqnorm.data_ptr() == withk._sums.data_ptr()
    assert withk.ws_bytes == _lib.imq_ksd_workspace_bytes(n, d) > plain.ws_bytes == _lib.imq_workspace_bytes(n, d)
    # a plain call after it, on the grown workspace
    withk.phi.fill_(float("nan"))
    withk.sqnorm.fill_(float("nan"))
    p2 = withk.compute_phi(T * 1.25, G).clone()
    fresh = _imq(n, d, cuda, h2)
    p3 = fresh.compute_phi(T * 1.25, G)
    torch.cuda.synchronize()
    assert torch.equal(p2, p3) and torch.equal(withk.sqnorm, fresh.sqnorm) and torch.equal(withk.h2, fresh.h2)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        withk.stein_discrepancy()
    # phi = NULL: the same three doubles
    alone = _imq(n, d, cuda, h2)
    alone.phi.fill_(float("nan"))
    got = alone.stream_discrepancy_sums(T, G)
    torch.cuda.synchronize()
    assert torch.equal(got, sums), (got, sums)
    assert torch.isnan(alone.phi).all()                  # nothing was stored


@pytest.mark.parametrize("n,d", [(150, 37), (1024, 256)])
def test_result_does_not_depend_on_what_the_workspace_held(cuda, n, d):
    T, G = _inputs(n, d, n + d, cuda)
    h2 = _f32(_median_h2(T, cuda))
    fresh = _imq(n, d, cuda, h2)
    fresh._stream_ksd_workspace()
    fresh.ws.zero_()
    want = _run(fresh, T, G)
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
    eng = _imq(n, d, cuda, h2)
    eng._stream_ksd_workspace()
    eng.ws.fill_(0xFF)                                    # NaN bytes
    eng.phi.fill_(float("nan"))
    eng._sums.fill_(float("nan"))
    got = _run(eng, T, G)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (n, d)
    # and the plain call
    eng.ws.fill_(0xFF)
    p_nan = eng.compute_phi(T, G).clone()
    eng.ws.zero_()
    p_zero = eng.compute_phi(T, G)
    torch.cuda.synchronize()
    assert torch.equal(p_nan, p_zero) and torch.equal(p_zero, want[0])


def test_unaligned_slices_take_the_scalar_finish(cuda):
    n, d = 300, 40
    T, G = _inputs(n, d, n + d, cuda)
    h2 = _f32(_median_h2(T, cuda))
    tb, gb, pb = (torch.zeros(n * d + 4, device=cuda) for _ in range(3))
    T_un, G_un, phi_un = tb[1:1 + n * d].view(n, d), gb[1:1 + n * d].view(n, d), pb[1:1 + n * d].view(n, d)
    T_un.copy_(T)
    G_un.copy_(G)
    assert T_un.data_ptr() % 16 == 4 and T_un.is_contiguous()
    phi, sums, _ = _run(_imq(n, d, cuda, h2), T, G)
    eng = _imq(n, d, cuda, h2)
    eng.phi = phi_un
    got = _run(eng, T_un, G)                              # theta and phi off the boundary: the scalar finish
    _check("%dx%d unaligned theta / phi" % (n, d), eng, T, G, got[0])
    assert torch.equal(got[0], phi)                       # phi is formed per element: the same bits on either path
    # only the score off the boundary: the 16-byte finish with scalar loads of the score, every sum in the same order
    got2 = _run(_imq(n, d, cuda, h2), T, G_un)
    assert torch.equal(got2[0], phi) and torch.equal(got2[1], sums)


# ---------------------------------------------------------------------------------------------------------------
# 4. the bandwidth lives on the device
# ---------------------------------------------------------------------------------------------------------------
def test_bandwidth_tensor_is_read_on_the_device_every_call(cuda):
    n, d = 700, 300
    T, G = _inputs(n, d, n + d, cuda)
    base = _median_h2(T, cuda)
    values = [_f32(base), _f32(base * 0.5), _f32(base * 1.75)]
    on_device = torch.tensor(values, dtype=torch.float32, device=cuda)
    h2 = torch.empty(1, dtype=torch.float32, device=cuda)
    eng = _imq(n, d, cuda, h2)
    got = []
    for k in range(3):                 # rewritten in place by device copies: nothing here waits for the GPU
        h2.copy_(on_device[k:k + 1])
        got.append((eng.compute_phi(T, G).clone(), eng.sqnorm.clone()))
    torch.cuda.synchronize()
    assert eng.h2 is h2
    for k, v in enumerate(values):
        h2.fill_(v)
        eng.sqnorm.copy_(got[k][1])
        _check("700x300 call %d at h2 = %.6g" % (k, v), eng, T, G, got[k][0], sums=False)
    assert not torch.equal(got[0][0], got[1][0]) and not torch.equal(got[1][0], got[2][0])


# ---------------------------------------------------------------------------------------------------------------
# 5. the statistic separates a good sample from a shifted one, at a fixed bandwidth
# ---------------------------------------------------------------------------------------------------------------
def test_statistic_separates_a_good_sample_from_a_shifted_one(cuda):
    n, d, h2 = 1000, 10, 3.0
    X = torch.tensor(np.random.default_rng(3).normal(size=(n, d)), dtype=torch.float32, device=cuda)
    got, ref, tol = {}, {}, {}
    for shift in (0.0, 2.0):
        Xs = X + shift
        eng = _imq(n, d, cuda, h2)
        phi = eng.compute_phi(Xs, -Xs, discrepancy=True)            # the score of N(0, I)
        ref_u, scale = _check("shift %g" % shift, eng, Xs, -Xs, phi)
        got[shift], ref[shift] = float(eng.stein_discrepancy("u").item()), ref_u
        tol[shift] = TOL_F32 * scale / (n * (n - 1))         # what the bound allows U to be off by
        print("imq shift %g: U %.6e (fp64 %.6e)" % (shift, got[shift], ref_u))
    # the fp64 statistic separates the two samples; the device's ratio is the fp64 ratio to within what the bound allows:
    # |a/b - A/B| <= (|a - A| + |A / B| |b - B|) / b
    ratio_ref = ref[0.0] / ref[2.0]
    assert ref[2.0] > 0.0 and abs(ratio_ref) < 1e-2, ref
    slack = (tol[0.0] + abs(ratio_ref) * tol[2.0]) / (ref[2.0] - tol[2.0])
    assert abs(got[0.0] / got[2.0] - ratio_ref) <= slack, (got, ref, slack)


# ---------------------------------------------------------------------------------------------------------------
# 6. the sampler, the standalone call, the refusals
# ---------------------------------------------------------------------------------------------------------------
def test_sampler_on_the_linear_regression_fixture(cuda, golden):
    """SteinSampler(bandwidth="median", kernel="imq", ksd_every=5), 50 particles, 60 Adagrad steps, against the same loop in
    fp64 (imq_ref.pair_phi at the fp64 median heuristic's bandwidth of the fp32-rounded particles), step for step, with the
    tolerance form of test_gpu_stream.py::test_sampler_with_a_fixed_bandwidth.  Every fifth step's statistic is the
    standalone call's on that step's particles, bit for bit (that call is held to fp64 in test_standalone_call), and held in
    between.  Its error against the fp64 pair sum is printed, not bounded, here: these particles sit up to six of their
    standard deviations from the origin (r_i / D_ij ~ 20 - 40 from step 40 on), and the library's distance r_i + r_j -
    2 x_i.x_j in fp32 carries eps32 (r_i + r_j) / D_ij of relative error -- measured 1.5e-6 of the scale at step 45, where
    the inputs of the parity tests (centred at the origin, r / D ~ 1/2) give at most 1.7e-7.
    The learning rate is 1e-3: Adagrad divides phi by the root of its running square, so a step is about lr whatever phi
    is, and with the stiff score here (d score / dw = -1001) lr = 1e-2 has the particles oscillate about the mode from
    step 16 on -- the fp64 loop itself then turns a relative perturbation of 3e-6 of phi into 4e-4 of theta after 60
    steps, 3e-3 into 3e-6 and 1e-3 into 1.5e-6 (measured on the reference loop alone, on the CPU).  A step-for-step
    comparison at 1e-5 needs the well-conditioned loop."""
    from oracle import svgd_oracle as orc
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    g = golden("g6_linear_regression.npz")
    X, y = torch.tensor(g["X"], dtype=torch.float64), torch.tensor(g["y"], dtype=torch.float64)
    A, b = float((X * X).sum()), float((X[:, 0] * y).sum())      # d log p / dw = X^T (y - X w) - w = b - (A + 1) w
    n, lr = 50, 1e-3
    T0 = np.random.default_rng(5).normal(size=(n, 1)) * 0.01

    def score(theta, feed):
        return b - (A + 1.0) * theta

    s = SteinSampler(n, None, AdagradGradientDescent(learning_rate=lr), theta=T0.copy(), score=score, device=cuda,
                     dtype=torch.float64, bandwidth="median", kernel="imq", ksd_every=5)
    assert s.engine.kernel == "imq" and s.engine.median_every == 1 and s.kernel is None
    with pytest.raises(RuntimeError, match="ksd_every"):
        s.stein_discrepancy()
    theta, gd = torch.tensor(T0), orc.AdagradState(learning_rate=lr)
    worst = worst_u = 0.0
    for it in range(60):
        before = s.theta_matrix.clone()
        s.train_on_batch(None)
        T32, G32 = theta.float().double(), score(theta, None).float().double()      # what the kernel path is fed
        phi = R.pair_phi(T32, G32, R.median_h2(T32)).numpy()
        theta = theta + torch.tensor(gd.update(phi * orc.clip_scale(float(np.sum(phi * phi)))))
        e = ci.frobenius_error(s.samples, theta.numpy())
        worst = max(worst, e)
        assert e <= 1e-5, (it, e)
        if it % 5 == 0:
            B32, S32 = before.float().contiguous(), score(before, None).float().contiguous()
            held = s.stein_discrepancy("u")
            assert held == ksd(B32, S32, statistic="u", bandwidth="median", kernel="imq"), it
            assert s.stein_discrepancy("v") == ksd(B32, S32, statistic="v", bandwidth="median", kernel="imq"), it
            S, Sd, scale = R.pairwise_sums(B32.double(), S32.double(), float(s.engine.h2.item()))
            worst_u = max(worst_u, abs(held - R.statistic(S, Sd, n, "u")) * n * (n - 1) / scale)
        else:
            assert s.stein_discrepancy("u") == held             # held in between
    print("imq sampler, linear regression, 60 steps: worst theta error against the fp64 loop %.2e; worst U error / scale %.2e"
          % (worst, worst_u))
    assert float(s.samples.mean()) > float(T0.mean()) + 0.03                   # (60 steps of ~lr towards the posterior mean)
    # state_dict / load_state_dict: a restored sampler continues with the same bits
    state = s.state_dict()
    s2 = SteinSampler(n, None, AdagradGradientDescent(learning_rate=lr), theta=np.zeros_like(T0), score=score, device=cuda,
                      dtype=torch.float64, bandwidth="median", kernel="imq", ksd_every=5)
    s2.load_state_dict(state)
    for _ in range(2):
        s.train_on_batch(None)
        s2.train_on_batch(None)
    assert np.array_equal(s.samples, s2.samples)


def test_standalone_call(cuda):
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    n, d = 600, 33
    T, G = _inputs(n, d, 9, cuda)
    eng = _imq(n, d, cuda, "median")
    eng.compute_phi(T, G, discrepancy=True)
    for stat in ("u", "v"):
        want = float(eng.stein_discrepancy(stat).item())
        assert ksd(T, G, statistic=stat, bandwidth="median", kernel="imq") == want
        assert ksd(T, G, statistic=stat, kernel="imq") == want          # bandwidth=None means "median" here
        assert ksd(T, G, statistic=stat, bandwidth="median") != want    # the RBF statistic is another number
    h = 2.5
    S, Sd, scale = R.pairwise_sums(T.double(), G.double(), _f32(h * h))
    for stat, norm in (("u", n * (n - 1)), ("v", n * n)):
        got = ksd(T, G, statistic=stat, bandwidth=h, kernel="imq")
        assert isinstance(got, float)
        assert abs(got - R.statistic(S, Sd, n, stat)) * norm <= TOL_F32 * scale, stat
    with pytest.raises(ValueError, match="float32"):
        ksd(T.bfloat16(), G.bfloat16(), kernel="imq")
    with pytest.raises(ValueError, match="bandwidth"):
        ksd(T, G, bandwidth=-1.0, kernel="imq")
    with pytest.raises(ValueError, match="kernel must be"):
        ksd(T, G, kernel="laplace")
    with pytest.raises(ValueError, match="at least two"):
        ksd(T[:1], G[:1], bandwidth=h, kernel="imq")


def test_what_is_refused_and_what_the_default_keeps(cuda):
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    n, d = 100, 10
    T, G = _inputs(n, d, 1, cuda)
    with pytest.raises(ValueError, match="h2=\"median\""):
        SvgdEngine(n, d, device=cuda, kernel="imq")                      # no stored-D IMQ path
    with pytest.raises(ValueError, match="group"):
        SvgdEngine(n, d, device=cuda, h2=1.5, kernel="imq", group=object())
    with pytest.raises(ValueError, match="bf16"):
        SvgdEngine(n, d, device=cuda, h2=1.5, kernel="imq", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="x3=False"):
        SvgdEngine(n, d, device=cuda, h2=1.5, kernel="imq", x3=False)
    with pytest.raises(ValueError, match="ksd=True"):
        SvgdEngine(n, d, device=cuda, h2=1.5, kernel="imq", ksd=True)
    for bad in ("laplace", "IMQ", None, 1):
        with pytest.raises(ValueError, match="kernel must be"):
            SvgdEngine(n, d, device=cuda, h2=1.5, kernel=bad)
    with pytest.raises(ValueError, match="median_every"):
        SvgdEngine(n, d, device=cuda, h2=1.5, kernel="imq", median_every=3)
    eng = _imq(n, d, cuda, 1.5)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        eng.stein_discrepancy()
    eng.compute_phi(T, G)
    with pytest.raises(ValueError, match="K_out"):
        eng.compute_phi(T, G, K_out=torch.empty(n, n, device=cuda))
    with pytest.raises(ValueError, match="dist_matrix"):
        eng.dist_matrix()
    with pytest.raises(ValueError, match="refresh_bandwidth"):
        eng.refresh_bandwidth(T)
    with pytest.raises(ValueError, match="bandwidth="):
        SteinSampler(n, None, AdagradGradientDescent(), theta=T.cpu().numpy(), device=cuda, kernel="imq")
    with pytest.raises(ValueError, match="kernel must be"):
        SteinSampler(n, None, AdagradGradientDescent(), theta=T.cpu().numpy(), device=cuda, bandwidth=1.0, kernel="cauchy")
    # median_every on the IMQ engine: the bandwidth is held between refreshes
    every = _imq(n, d, cuda, "median")
    held = SvgdEngine(n, d, device=cuda, h2="median", kernel="imq", median_every=2)
    held.compute_phi(T, G)
    first = held.h2.clone()
    held.compute_phi(T * 2.0, G)
    assert torch.equal(held.h2, first)
    held.compute_phi(T * 2.0, G)
    every.compute_phi(T * 2.0, G)
    assert torch.equal(held.h2, every.h2) and not torch.equal(held.h2, first)
    # the default kernel="rbf" is the engine without the keyword, to the bit: stored-D and streaming
    for kw in ({}, {"h2": 1.5}, {"h2": "median"}):
        a, c = SvgdEngine(n, d, device=cuda, **kw), SvgdEngine(n, d, device=cuda, kernel="rbf", **kw)
        pa, pc = a.compute_phi(T, G), c.compute_phi(T, G)
        torch.cuda.synchronize()
        assert a.kernel == c.kernel == "rbf" and a.ws_bytes == c.ws_bytes
        assert torch.equal(pa, pc) and torch.equal(a.sqnorm, c.sqnorm) and torch.equal(a.h2, c.h2)
    assert not torch.equal(_imq(n, d, cuda, 1.5).compute_phi(T, G), SvgdEngine(n, d, device=cuda, h2=1.5).compute_phi(T, G))
    # one particle: V is u_11 = |g|^2 + d / c2 (k_11 = 1), U is undefined
    one = _imq(1, 3, cuda, 2.0)
    T1, G1 = _inputs(1, 3, 5, cuda)
    phi1 = one.compute_phi(T1, G1, discrepancy=True)
    _check("1x3", one, T1, G1, phi1)
    want = float((G1.double() ** 2).sum()) + 3 / 4.0
    assert abs(one.stein_discrepancy("v").item() - want) <= 1e-6 * want
    with pytest.raises(ValueError, match="at least two"):
        one.stein_discrepancy("u")
