"""GPU: the kernelized Stein discrepancy of the streaming step (stein_svgd_phi_stream_ksd: SvgdEngine.compute_phi(...,
discrepancy=True), SteinSampler(ksd_every=), utilities.kernelized_stein_discrepancy(bandwidth=)) against the fp64 pair sum
of tests/ksd_ref.py on the device, evaluated at the engine's own h2.

Inputs are test_gpu_ksd._inputs; errors are over ksd_ref's scale, sum_ij |terms of u_ij|; the bound is the stored-D
statistic's, TOL_F32 = 1e-6.  Every ratio is printed (-s).

Measured on an MI355X: at the median's bandwidth 1.4e-9 .. 9.4e-8 over the ten parity shapes, at four times it below 1e-8, at
a quarter of it 5.4e-7 .. 9.56e-7 (4096 x 256) from 128 x 128 on.  The last sits close under the bound: there the off-diagonal
k_ij are tiny, S is the diagonal's, and the streaming distance leaves D_ii slightly above 0 (the split's dropped lo.lo term is
a sum of squares on the diagonal), so k_ii is below 1 by D_ii / (2 h2) -- the kernel phi is computed with.
j splits 3.6e-8 / 6.2e-8; unaligned rows 1.0e-8; the shifted sample 7.2e-8."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksd_ref as R  # noqa: E402
from test_gpu_ksd import TOL_F32, _errors, _inputs  # noqa: E402

from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu


def _f32(x):
    return float(np.float32(x))


def _median_h2(T, cuda):
    """the streaming median's h2 of T, as a float"""
    n, d = T.shape
    eng = SvgdEngine(n, d, device=cuda, h2="median")
    return float(eng.refresh_bandwidth(T).item())


def _run(eng, T, G):
    """one discrepancy call -> clones of (phi, sums, h2)"""
    phi = eng.compute_phi(T, G, discrepancy=True)
    torch.cuda.synchronize()
    return phi.clone(), eng._sums.clone(), eng.h2.clone()


# ---------------------------------------------------------------------------------------------------------------
# 1. parity of S, S_diag, U and V
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (20, 3), (128, 128), (129, 129), (150, 37), (257, 256), (300, 260), (384, 513), (1000, 40), (4096, 256)]


@pytest.mark.parametrize("n,d", SHAPES)
def test_parity_with_fp64_pair_sum(cuda, n, d):
    T, G = _inputs(n, d, n + d, cuda)
    med = _median_h2(T, cuda)
    engines = [("median x%g" % m, SvgdEngine(n, d, device=cuda, h2=_f32(med * m))) for m in (0.25, 1.0, 4.0)]
    engines.append(("h2=\"median\"", SvgdEngine(n, d, device=cuda, h2="median")))
    for tag, eng in engines:
        eng.compute_phi(T, G, discrepancy=True)
        errs, _ = _errors(eng, T, G)
        print("stream ksd %dx%d %s (plan %s): err/scale S %.2e S_diag %.2e U %.2e V %.2e" %
              ((n, d, tag, (eng.row_tiles, eng.col_groups, eng.jsplit)) + errs))
        assert max(errs) <= TOL_F32, (tag, errs)
    assert engines[3][1].h2.item() == med


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
            eng = SvgdEngine(n, d, device=cuda, h2=h2)
            if (n, d) == (700, 300):                       # six j tiles: 4 asks for ranges of two, three ranges
                assert eng.jsplit == {1: 1, 2: 2, 3: 3, 4: 3, 6: 6}[want]
            phi, sums, _ = _run(eng, T, G)
            errs, _ = _errors(eng, T, G)
            print("stream ksd %dx%d jsplit %d (asked %d): err/scale S %.2e S_diag %.2e U %.2e V %.2e" %
                  ((n, d, eng.jsplit, want) + errs))
            assert max(errs) <= TOL_F32, (want, errs)
            again = _run(eng, T, G)
            assert torch.equal(again[0], phi) and torch.equal(again[1], sums), (want, "repeat")
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
    plain = SvgdEngine(n, d, device=cuda, h2=h2)
    withk = SvgdEngine(n, d, device=cuda, h2=h2)
    p0 = plain.compute_phi(T, G).clone()
    p1, sums, _ = _run(withk, T, G)
    assert torch.equal(p0, p1) and torch.equal(plain.sqnorm, withk.sqnorm) and torch.equal(plain.h2, withk.h2)
    assert withk.sqnorm.data_ptr() == withk._sums.data_ptr()
    assert withk.ws_bytes == _lib.stream_ksd_workspace_bytes(n, d) > plain.ws_bytes
    # a plain call after it, on the grown workspace
    withk.phi.fill_(float("nan"))
    withk.sqnorm.fill_(float("nan"))
    p2 = withk.compute_phi(T * 1.25, G).clone()
    fresh = SvgdEngine(n, d, device=cuda, h2=h2)
    p3 = fresh.compute_phi(T * 1.25, G)
    torch.cuda.synchronize()
    assert torch.equal(p2, p3) and torch.equal(withk.sqnorm, fresh.sqnorm) and torch.equal(withk.h2, fresh.h2)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        withk.stein_discrepancy()
    # phi = NULL: the same three doubles
    alone = SvgdEngine(n, d, device=cuda, h2=h2)
    alone.phi.fill_(float("nan"))
    got = alone.stream_discrepancy_sums(T, G)
    torch.cuda.synchronize()
    assert torch.equal(got, sums), (got, sums)
    assert torch.isnan(alone.phi).all()                  # nothing was stored


# ---------------------------------------------------------------------------------------------------------------
# 4. the workspace carries nothing
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(150, 37), (1024, 256)])
def test_result_does_not_depend_on_what_the_workspace_held(cuda, n, d):
    T, G = _inputs(n, d, n + d, cuda)
    h2 = _f32(_median_h2(T, cuda))
    fresh = SvgdEngine(n, d, device=cuda, h2=h2)
    fresh._stream_ksd_workspace()
    fresh.ws.zero_()
    want = _run(fresh, T, G)
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
    eng = SvgdEngine(n, d, device=cuda, h2=h2)
    eng._stream_ksd_workspace()
    eng.ws.fill_(0xFF)
    eng.phi.fill_(float("nan"))
    eng._sums.fill_(float("nan"))
    got = _run(eng, T, G)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (n, d)


# ---------------------------------------------------------------------------------------------------------------
# 5. unaligned rows with d % 4 == 0: the scalar finish
# ---------------------------------------------------------------------------------------------------------------
def test_unaligned_slices_take_the_scalar_finish(cuda):
    n, d = 300, 40
    T, G = _inputs(n, d, n + d, cuda)
    h2 = _f32(_median_h2(T, cuda))
    tb, gb, pb = (torch.zeros(n * d + 4, device=cuda) for _ in range(3))
    T_un, G_un, phi_un = tb[1:1 + n * d].view(n, d), gb[1:1 + n * d].view(n, d), pb[1:1 + n * d].view(n, d)
    T_un.copy_(T)
    G_un.copy_(G)
    assert T_un.data_ptr() % 16 == 4 and T_un.is_contiguous()
    aligned = SvgdEngine(n, d, device=cuda, h2=h2)
    phi, sums, _ = _run(aligned, T, G)
    eng = SvgdEngine(n, d, device=cuda, h2=h2)
    eng.phi = phi_un
    got = _run(eng, T_un, G)                              # theta and phi off the boundary: the scalar finish
    errs, _ = _errors(eng, T, G)
    print("stream ksd %dx%d unaligned theta / phi: err/scale S %.2e S_diag %.2e U %.2e V %.2e" % ((n, d) + errs))
    assert max(errs) <= TOL_F32, errs
    assert torch.equal(got[0], phi)                       # phi is formed per element: the same bits on either path
    # only the score off the boundary: the 16-byte finish with scalar loads of the score, every sum in the same order
    eng2 = SvgdEngine(n, d, device=cuda, h2=h2)
    got2 = _run(eng2, T, G_un)
    assert torch.equal(got2[0], phi) and torch.equal(got2[1], sums)


# ---------------------------------------------------------------------------------------------------------------
# 6. the statistic separates a good sample from a shifted one, at a fixed bandwidth
# ---------------------------------------------------------------------------------------------------------------
def test_statistic_separates_a_good_sample_from_a_shifted_one(cuda):
    n, d, h2 = 1000, 10, 3.0
    X = torch.tensor(np.random.default_rng(3).normal(size=(n, d)), dtype=torch.float32, device=cuda)
    got, ref, tol = {}, {}, {}
    for shift in (0.0, 2.0):
        Xs = X + shift
        eng = SvgdEngine(n, d, device=cuda, h2=h2)
        eng.compute_phi(Xs, -Xs, discrepancy=True)            # the score of N(0, I)
        errs, (ref_u, _, scale) = _errors(eng, Xs, -Xs)
        print("stream ksd shift %g: err/scale S %.2e S_diag %.2e U %.2e V %.2e; U %.6e (fp64 %.6e)" %
              ((shift,) + errs + (float(eng.stein_discrepancy("u").item()), ref_u)))
        assert max(errs) <= TOL_F32, errs
        got[shift], ref[shift] = float(eng.stein_discrepancy("u").item()), ref_u
        tol[shift] = TOL_F32 * scale / (n * (n - 1))         # what the bound allows U to be off by
    # the fp64 statistic separates the two samples; the device's ratio is the fp64 ratio to within what the bound allows:
    # |a/b - A/B| <= (|a - A| + |A / B| |b - B|) / b
    ratio_ref = ref[0.0] / ref[2.0]
    assert ref[2.0] > 0.0 and abs(ratio_ref) < 1e-2, ref
    slack = (tol[0.0] + abs(ratio_ref) * tol[2.0]) / (ref[2.0] - tol[2.0])
    assert abs(got[0.0] / got[2.0] - ratio_ref) <= slack, (got, ref, slack)


# ---------------------------------------------------------------------------------------------------------------
# 7. the sampler, the standalone call, the refusals
# ---------------------------------------------------------------------------------------------------------------
def test_sampler_reports_every_kth_step(cuda):
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    n, d, h = 300, 7, 1.3
    T, G = _inputs(n, d, 21, cuda)
    s = SteinSampler(n, None, AdagradGradientDescent(learning_rate=1e-2), theta=T.cpu().numpy(), device=cuda, bandwidth=h,
                     ksd_every=3)
    with pytest.raises(RuntimeError, match="ksd_every"):
        s.stein_discrepancy()
    last = None
    for update in range(1, 8):
        before = s.theta_matrix.clone()
        score = G - 0.1 * update * before
        s.update_particles(score)
        if update in (1, 4, 7):
            last = {stat: ksd(before, score, statistic=stat, bandwidth=h) for stat in ("u", "v")}
        for stat in ("u", "v"):
            assert s.stein_discrepancy(stat) == last[stat], (update, stat)      # bit for bit; held in between
    with pytest.raises(ValueError, match="'u' or 'v'"):
        s.stein_discrepancy("w")


def test_standalone_call_at_a_bandwidth(cuda):
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    n, d = 600, 33
    T, G = _inputs(n, d, 9, cuda)
    eng = SvgdEngine(n, d, device=cuda, h2="median")
    eng.compute_phi(T, G, discrepancy=True)
    for stat, norm in (("u", n * (n - 1)), ("v", n * n)):
        assert ksd(T, G, statistic=stat, bandwidth="median") == float(eng.stein_discrepancy(stat).item())
    h = 2.5
    S, Sd, scale = R.pairwise_sums(T.double(), G.double(), _f32(h * h))
    for stat, norm in (("u", n * (n - 1)), ("v", n * n)):
        got = ksd(T, G, statistic=stat, bandwidth=h)
        assert isinstance(got, float)
        assert abs(got - R.statistic(S, Sd, n, stat)) * norm <= TOL_F32 * scale, stat
    with pytest.raises(ValueError, match="float32"):
        ksd(T.bfloat16(), G.bfloat16(), bandwidth=h)
    with pytest.raises(ValueError, match="bandwidth"):
        ksd(T, G, bandwidth=-1.0)
    with pytest.raises(ValueError, match="at least two"):
        ksd(T[:1], G[:1], bandwidth=h)


def test_what_is_refused(cuda):
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    n, d = 64, 4
    T, G = _inputs(n, d, 1, cuda)
    eng = SvgdEngine(n, d, device=cuda, h2=1.5)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        eng.stein_discrepancy()
    eng.compute_phi(T, G)
    with pytest.raises(RuntimeError, match="discrepancy=True"):
        eng.stein_discrepancy()
    eng.compute_phi(T, G, discrepancy=True)
    assert np.isfinite(eng.stein_discrepancy("u").item()) and np.isfinite(eng.stein_discrepancy("v").item())
    with pytest.raises(ValueError, match="'u' or 'v'"):
        eng.stein_discrepancy("w")
    with pytest.raises(ValueError, match="ksd.*discrepancy=True"):
        SvgdEngine(n, d, device=cuda, h2=1.5, ksd=True)
    stored = SvgdEngine(n, d, device=cuda)
    with pytest.raises(ValueError, match="ksd=True"):
        stored.compute_phi(T, G, discrepancy=True)
    with pytest.raises(ValueError, match="ksd_every"):
        SteinSampler(n, None, AdagradGradientDescent(), theta=T.cpu().numpy(), device=cuda, ksd_every=2)
    # one particle: V is u_11 = |g|^2 + d / h2 (k_11 = 1), U is undefined
    one = SvgdEngine(1, 3, device=cuda, h2=2.0)
    T1, G1 = _inputs(1, 3, 5, cuda)
    one.compute_phi(T1, G1, discrepancy=True)
    want = float((G1.double() ** 2).sum()) + 3 / 2.0
    assert abs(one.stein_discrepancy("v").item() - want) <= 1e-6 * want
    with pytest.raises(ValueError, match="at least two"):
        one.stein_discrepancy("u")
