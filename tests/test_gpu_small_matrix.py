"""GPU: the one-kernel path (csrc/stein_small.hip, k_svgd_small, n <= 160) across its whole dispatch domain.

The kernel's code shape is chosen at run time from n and d (tests/small_cases.py restates the choices; tests/
test_small_cases.py asserts that the tables used here reach every one of them and that the library takes this path at each):
distances<1..5>, phi_rows<2 | 4 | 8 | 10, 8 | 16 | 32> per workgroup, one to 128 passes of the theta chunk loop with a
ragged last pass, one workgroup (which writes |phi|^2 itself) or up to 1024 (summed by a second kernel), with and without
the Stein discrepancy sums.  Every test asserts `eng._one_kernel` (or its negation) first, so that no case can silently
test the other path.

Yardsticks: oracle.svgd_oracle in fp64 on the fp32-rounded inputs, tests/ksd_ref.py for the Stein discrepancy, an exact
int64 sort (tests/select_inputs.py) for the bandwidth on integer lattices.  theta = normal * s_T and score = normal * s_G
with s_T drawn from [0.3, 3] and s_G from [0.1, 10], seeded from (n, d).  Bounds: the ones tests/test_gpu_small.py and
tests/test_gpu_random_shapes.py hold this path to (TOL below).

Wide d (WIDE_CASES, up to 32768 columns): row norms and dot products are fp32 sums of up to 32768 terms, where 1e-5 cannot be
derived by reading; per case and quantity the allowance is max(TOL, 4 x the error of the project's own fp32 oracle against
its fp64 run on the same inputs) -- the kernel accumulates sequentially with FMA, in another order than NumPy, and a factor
of a few is what order alone can cost.  Every case prints its error over allowance (-s).
Worst error over allowance observed on an MI355X: the comment above test_wide_d.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksd_ref as R  # noqa: E402
import select_inputs as si  # noqa: E402
import small_cases as sc  # noqa: E402
from test_gpu_ksd import TOL_F32  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import HipStages, SvgdEngine  # noqa: E402
from stein_amd.optimizers import AdagradGradientDescent  # noqa: E402

pytestmark = pytest.mark.gpu

# h2 relative; phi as norm-relative error and as max-abs over max |phi|; |phi|^2 relative; K absolute (K <= 1); dK over its
# largest entry
TOL = dict(h2=4e-6, phi=1e-5, phi_max=1e-5, sqnorm=2e-5, K=1e-5, dK=1e-5)


def _inputs(n, d, salt=0):
    """fp32 theta and score, seeded from (n, d)"""
    rng = np.random.default_rng([n, d, salt])
    T = (rng.normal(size=(n, d)) * rng.uniform(0.3, 3.0)).astype(np.float32)
    G = (rng.normal(size=(n, d)) * rng.uniform(0.1, 10.0)).astype(np.float32)
    return T, G


_REFS = {}


def _ref(n, d):
    """inputs and the fp64 oracle's step on them: computed once per shape, shared by the tests, never written to"""
    if (n, d) not in _REFS:
        T, G = _inputs(n, d)
        T64, G64 = T.astype(np.float64), G.astype(np.float64)
        step = orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)
        K, dK = orc.kernel_and_grad(T64, np.float64)
        _REFS[(n, d)] = dict(T=T, G=G, h2=float(step["h2"]), phi=step["phi"], sqnorm=float(step["sqnorm"]), K=K, dK=dK)
    return _REFS[(n, d)]


def _measures(h2, phi, sqnorm, K, dK, ref):
    """the errors TOL bounds, of a result (NumPy / floats) against an fp64 reference"""
    phi = np.asarray(phi, dtype=np.float64)
    out = dict(h2=abs(float(h2) - ref["h2"]) / ref["h2"],
               phi=float(np.linalg.norm(phi - ref["phi"]) / np.linalg.norm(ref["phi"])),
               phi_max=float(np.abs(phi - ref["phi"]).max() / np.abs(ref["phi"]).max()),
               sqnorm=abs(float(sqnorm) - ref["sqnorm"]) / ref["sqnorm"])
    if K is not None:
        out["K"] = float(np.abs(np.asarray(K, dtype=np.float64) - ref["K"]).max())
    if dK is not None:
        out["dK"] = float(np.abs(np.asarray(dK, dtype=np.float64) - ref["dK"]).max() / np.abs(ref["dK"]).max())
    return out


def _run(eng, T, G, want_K, want_dK, dev):
    n, d = T.shape
    K = torch.full((n, n), float("nan"), device=dev) if want_K else None
    dK = torch.full((n, d), float("nan"), device=dev) if want_dK else None
    eng.phi.fill_(float("nan"))
    phi = eng.compute_phi(torch.tensor(T, device=dev), torch.tensor(G, device=dev), K_out=K, dK_out=dK)
    torch.cuda.synchronize()
    return (float(eng.h2.item()), phi.cpu().numpy(), float(eng.sqnorm.item()),
            K.cpu().numpy() if want_K else None, dK.cpu().numpy() if want_dK else None)


def _assert_within(errs, allow, tag):
    print("small %s: %s" % (tag, "  ".join("%s %.2e/%.1e" % (q, e, allow[q]) for q, e in errs.items())))
    bad = {q: (e, allow[q]) for q, e in errs.items() if not e <= allow[q]}       # (not <=: a NaN fails)
    assert not bad, (tag, bad)


# ---- a: every code shape against fp64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", sc.MATRIX_CASES)
def test_matrix_against_fp64(cuda, n, d):
    """EDGE, CHUNK and RANDOM cases.  K_out on every second case and dK_out on every second pair of cases: all four
    combinations, so the `K_out && blockIdx.x == 0` and `dK_out` branches are taken and skipped at multi-workgroup shapes."""
    idx = sc.MATRIX_CASES.index((n, d))
    eng = SvgdEngine(n, d, device=cuda)
    assert eng._one_kernel
    ref = _ref(n, d)
    got = _run(eng, ref["T"], ref["G"], idx % 2 == 1, (idx // 2) % 2 == 1, cuda)
    _assert_within(_measures(*got, ref), TOL, (n, d))


# ---- b: wide d ----------------------------------------------------------------------------------------------------------
# Worst error over allowance on an MI355X (the allowance was TOL everywhere: the fp32 oracle is within 4e-7 of fp64 in every
# quantity): h2 0.048 (3 x 20000), phi 0.013 as norm and 0.022 as maximum (13 x 13000), |phi|^2 0.004 (3 x 20000),
# K 0.011 (8 x 30000), dK 0.024 (13 x 13000)
@pytest.mark.parametrize("n,d", sc.WIDE_CASES)
def test_wide_d(cuda, n, d, record_property):
    eng = SvgdEngine(n, d, device=cuda)
    assert eng._one_kernel and sc.classify(n, d)["blocks"] > 100
    ref = _ref(n, d)
    T64, G64 = ref["T"].astype(np.float64), ref["G"].astype(np.float64)
    o32 = orc.svgd_step(T64, G64, orc.AdagradState(), np.float32)                 # the project's fp32 oracle, same inputs
    K32, dK32 = orc.kernel_and_grad(T64, np.float32)
    oracle = _measures(o32["h2"], o32["phi"], o32["sqnorm"], K32, dK32, ref)
    allow = {q: max(TOL[q], 4.0 * oracle[q]) for q in TOL}
    h2, phi, sqnorm, K, dK = _run(eng, ref["T"], ref["G"], True, True, cuda)
    errs = _measures(h2, phi, sqnorm, K, dK, ref)
    ratios = {q: errs[q] / allow[q] for q in errs}
    print("wide %dx%d error over allowance: %s   (fp32 oracle's own error: %s)" % (
        n, d, "  ".join("%s %.3f" % i for i in ratios.items()), "  ".join("%s %.1e" % i for i in oracle.items())))
    record_property("error_over_allowance", str(ratios))
    # the partials of up to 1024 workgroups are doubles, summed in double: no excuse there
    exact = float(np.sum(phi.astype(np.float64) ** 2))
    assert abs(sqnorm - exact) <= 1e-12 * exact, (n, d, sqnorm, exact)
    _assert_within(errs, allow, (n, d, "wide"))


# ---- c: three steps with drift --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", sc.RANDOM_CASES)
def test_three_steps_with_drift(cuda, n, d):
    """compute_phi + Adagrad three times on one engine, re-synchronised to the oracle's particles after every step (as
    tests/test_gpu_random_shapes.py does for the tiled path): nothing of a step lives on into the next"""
    T0, G0 = _inputs(n, d)
    theta, score = torch.tensor(T0, device=cuda), torch.tensor(G0, device=cuda)
    eng = SvgdEngine(n, d, device=cuda)
    assert eng._one_kernel
    gd = AdagradGradientDescent(learning_rate=1e-2)
    gd_o = orc.AdagradState(learning_rate=1e-2, alpha=0.9)
    th, G64 = T0, G0.astype(np.float64)
    for step in range(3):
        phi = eng.compute_phi(theta, score)
        ref = orc.svgd_step(th.astype(np.float64), G64, gd_o, np.float64)
        torch.cuda.synchronize()
        errs = _measures(eng.h2.item(), phi.cpu().numpy(), eng.sqnorm.item(), None, None,
                         dict(h2=float(ref["h2"]), phi=ref["phi"], sqnorm=float(ref["sqnorm"])))
        _assert_within(errs, TOL, (n, d, "step %d" % step))
        gd.apply_(theta, phi, eng.sqnorm)
        th = ref["theta_new"].astype(np.float32)
        assert not np.array_equal(th, T0)
        theta.copy_(torch.tensor(th, device=cuda))                 # both trajectories stay on the same particles


# ---- d: both sides of the path's edge -------------------------------------------------------------------------------------
@pytest.mark.parametrize("on,off", sc.EDGE_OF_PATH, ids=lambda v: "%dx%d" % v)
def test_both_sides_of_the_edge(cuda, on, off):
    """On the path: against fp64 and against the tiled kernels (small=False) on the same inputs; one step off it: the default
    engine takes the tiled kernels and meets the same fp64 bounds.
    (2, 32768) is the widest shape of the path: 128 chunks of 256 columns, 1024 workgroups."""
    n, d = on
    small, tiled = SvgdEngine(n, d, device=cuda), SvgdEngine(n, d, device=cuda, small=False)
    assert small._one_kernel and not tiled._one_kernel
    ref = _ref(n, d)
    got = _run(small, ref["T"], ref["G"], True, True, cuda)
    got_t = _run(tiled, ref["T"], ref["G"], False, True, cuda)
    _assert_within(_measures(*got, ref), TOL, (n, d, "on the path"))
    # the two paths on the same inputs: the tiled kernels' result as the reference of the one kernel's
    as_ref = dict(h2=got_t[0], phi=got_t[1].astype(np.float64), sqnorm=got_t[2], dK=got_t[4].astype(np.float64))
    _assert_within(_measures(got[0], got[1], got[2], None, got[4], as_ref), TOL, (n, d, "against the tiled kernels"))
    n2, d2 = off
    beyond = SvgdEngine(n2, d2, device=cuda)
    assert not beyond._one_kernel
    ref2 = _ref(n2, d2)
    _assert_within(_measures(*_run(beyond, ref2["T"], ref2["G"], False, True, cuda), ref2), TOL, (n2, d2, "off the path"))


def test_one_particle_is_refused_before_any_launch(cuda):
    d = 5
    T, G = torch.randn(1, d, device=cuda), torch.randn(1, d, device=cuda)
    phi, h2 = torch.full((1, d), -7.0, device=cuda), torch.full((1,), -7.0, device=cuda)
    sq = torch.full((1,), -7.0, dtype=torch.float64, device=cuda)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match=r"libsteinhip error -1: .*ln\(n\)"):
        HipStages().svgd_phi(T, G, 1, d, phi, h2, sq, None, None, ws, _lib.FLAG_X3)
    torch.cuda.synchronize()
    assert bool((phi == -7.0).all()) and float(h2) == -7.0 and float(sq) == -7.0      # nothing ran
    with pytest.raises(ValueError, match="need n >= 2"):
        SvgdEngine(1, d, device=cuda)


# ---- e: the KSD instantiation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", sc.KSD_CASES)
def test_ksd_instantiation(cuda, n, d):
    """k_svgd_small<true> at every R, RW and CLW of the last workgroup, on one and on several workgroups: S and S_diag against
    the fp64 pair sum at the engine's own bandwidth, and the step itself bit-identical to k_svgd_small<false>'s"""
    T, G = (torch.tensor(a, device=cuda) for a in _inputs(n, d))
    plain, withk = SvgdEngine(n, d, device=cuda), SvgdEngine(n, d, device=cuda, ksd=True)
    assert plain._one_kernel and withk._one_kernel
    p0 = plain.compute_phi(T, G).clone()
    p1 = withk.compute_phi(T, G)
    torch.cuda.synchronize()
    S, Sd, scale = R.pairwise_sums(T.double(), G.double(), float(withk.h2.item()))
    sums = withk._sums.cpu().tolist()
    errs = (abs(sums[1] - S) / scale, abs(sums[2] - Sd) / scale)
    print("small ksd %dx%d: err/scale S %.2e S_diag %.2e" % ((n, d) + errs))
    assert max(errs) <= TOL_F32, errs
    assert torch.equal(p0, p1) and torch.equal(plain.h2, withk.h2), (n, d)
    assert plain._sums[0].item() == withk._sums[0].item(), (n, d)


# ---- f: bit-level invariants -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", sc.BIT_CASES)
def test_bit_level_invariants(cuda, n, d):
    Tn, Gn = _inputs(n, d)
    T, G = torch.tensor(Tn, device=cuda), torch.tensor(Gn, device=cuda)
    G2 = torch.tensor(_inputs(n, d, salt=1)[1], device=cuda)
    eng = SvgdEngine(n, d, device=cuda)
    assert eng._one_kernel
    phi0, h0, s0 = eng.compute_phi(T, G).clone(), eng.h2.clone(), eng.sqnorm.clone()
    assert bool(torch.isfinite(phi0).all()) and float(h0) > 0
    Ks, dKs = [], []
    for want_K, want_dK in ((False, False), (True, False), (False, True), (True, True)):     # the first: a repeated call
        K = torch.full((n, n), float("nan"), device=cuda) if want_K else None
        dK = torch.full((n, d), float("nan"), device=cuda) if want_dK else None
        eng.phi.fill_(float("nan"))
        phi = eng.compute_phi(T, G, K_out=K, dK_out=dK)
        assert torch.equal(phi, phi0) and torch.equal(eng.h2, h0) and torch.equal(eng.sqnorm, s0), (n, d, want_K, want_dK)
        Ks += [K] if want_K else []
        dKs += [dK] if want_dK else []
    assert torch.equal(Ks[0], Ks[1]) and torch.equal(dKs[0], dKs[1])
    K = Ks[0]
    assert bool(torch.isfinite(K).all()) and torch.equal(K, K.T)
    # D_ii is exactly 0 (both norms and the dot product of a row with itself run the same FMA chain), K_ii = exp2(kc * 0)
    assert bool((K.diagonal() == 1.0).all())
    assert bool(torch.isfinite(dKs[0]).all())
    # another score: the kernel matrix and the bandwidth are theta's alone
    K2 = torch.full((n, n), float("nan"), device=cuda)
    phi2 = eng.compute_phi(T, G2, K_out=K2)
    assert torch.equal(eng.h2, h0) and torch.equal(K2, K) and not torch.equal(phi2, phi0)


# ---- g: the exact select where the distance stage is distances<3>, and across its edges ---------------------------------------
SELECT_CASES = [(f, n) for n in sc.SELECT_N for f in si.families_at(n)]


@pytest.mark.parametrize("family,n", SELECT_CASES, ids=lambda v: str(v))
def test_lds_select_is_exact(cuda, family, n):
    """integer lattices: every distance an integer that fp32 holds exactly, the bandwidth that of the int64-sorted median to
    the bit (as tests/test_gpu_select_lattice.py asserts for n = 7, 8, 129, 160)"""
    ref = si.lattice_ref(family, n)
    d = ref.P.shape[1]
    T = torch.tensor(ref.P, dtype=torch.float32, device=cuda)
    G = torch.tensor(si.gaussian_scores(n, d), device=cuda)
    for ksd in (False, True) if family in ("line", "simplex4_128_1") else (False,):
        eng = SvgdEngine(n, d, device=cuda, ksd=ksd)
        assert eng._one_kernel
        for step in range(2):
            eng.h2.fill_(float("nan"))
            eng.compute_phi(T, G)
            assert float(eng.h2) == float(ref.h2), (family, n, ksd, step, float(eng.h2), float(ref.h2), ref.lo, ref.hi)
