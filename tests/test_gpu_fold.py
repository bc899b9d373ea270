"""GPU: the folded contraction of the fused call (STEIN_FLAG_FOLD; stein_x3.hip, "folded operand").

phi_i = (sum_j K_ij w_j + rowsum_i theta_i / h2) / n with w_j = g_j - theta_j / h2: K meets ONE matrix, W, whose operand planes
are built behind the median.  By default only large blocks take the form; every test here forces it (fold=True) on the
small shapes of the other modules unless it says otherwise, and holds it to the checks and tolerances those modules apply
to the unfolded path (imported from them, not restated).

Bounds that are not imported: the folded path's error against fp64 on sampled rows is held to twice the unfolded path's
own on the same rows (both paths carry 2^-38 of max|g| + max|theta| / h2 per column; a factor of two
covers one path drawing the worse roundings) and in any case to the project's 1e-5.  Run with -s to see every figure."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import test_gpu_conditioning as tc  # noqa: E402
import test_gpu_x3 as tx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = tc.TOL


def _folded(n, d, cuda, **kw):
    eng = SvgdEngine(n, d, device=cuda, fold=True, small=False, **kw)
    assert eng.fold, "fold=True did not select the folded contraction"
    return eng


# ---------------------------------------------------------------------------------------------------------------
# 1. parity with the fp64 oracle on the path itself
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", tx.SHAPES)
def test_parity_normal_inputs(cuda, n, d):
    T64, G64 = tx._inputs(n, d)
    T64, G64 = ci.f32(T64), ci.f32(G64)
    ref = orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    eng = _folded(n, d, cuda)
    dK = torch.full((n, d), float("nan"), device=cuda)
    tag = "fold normal %dx%d" % (n, d)
    terms = ref["K"].sum(1)[:, None] / ref["h2"]
    for call in range(3):       # radix select first, the speculative window later
        phi = eng.compute_phi(T, G, dK_out=dK)
        torch.cuda.synchronize()
        tc._check_bandwidth(tag, eng.h2, eng.dist_matrix(), ref, n)
        tc._check_columns(tag, tc._np(phi), ref["phi"], T64, "phi")
        tc._check_columns(tag, tc._np(dK), ref["dK"], T64, "dK", scale_terms=terms)
        assert abs(eng.sqnorm.item() - ref["sqnorm"]) <= 2e-5 * ref["sqnorm"], tag


PARITY = [(f, n, d) for f in ci.FAMILIES for (n, d) in tc.SHAPES]


@pytest.mark.parametrize("family,n,d", PARITY, ids=["%s-%dx%d" % c for c in PARITY])
def test_parity_per_column(cuda, family, n, d):
    """test_gpu_conditioning.test_parity_per_column, path "fused", on the folded contraction"""
    T64, G64, ref = tc._case(family, n, d)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    tag = "fold %s %dx%d" % (family, n, d)
    is_far = family.startswith("far")
    terms = ref["K"].sum(1)[:, None] / ref["h2"]
    eng = _folded(n, d, cuda)
    dK = torch.full((n, d), float("nan"), device=cuda)
    skip = (ci.FAR_ROW,) if is_far else ()
    for call in range(3):
        phi = eng.compute_phi(T, G, dK_out=dK)
        torch.cuda.synchronize()
        Dg = eng.dist_matrix()
        h2 = tc._check_bandwidth(tag, eng.h2, Dg, ref, n)
        p = tc._np(phi)
        tc._check_columns(tag, p, ref["phi"], T64, "phi", skip)
        tc._check_columns(tag, tc._np(dK), ref["dK"], T64, "dK", skip, scale_terms=terms)
        assert np.isfinite(eng.sqnorm.item()), tag
        if not is_far:
            assert abs(eng.sqnorm.item() - ref["sqnorm"]) <= 2e-5 * ref["sqnorm"], tag
        else:
            tc._check_far_row(tag, p[ci.FAR_ROW], G64, n, h2, float(Dg[ci.FAR_ROW, ci.FAR_ROW]), ref, True)


@pytest.mark.parametrize("n,d", tc.SHAPES)
def test_offset_cluster(cuda, n, d):
    """the yardstick of test_gpu_conditioning.test_offset_cluster_on_the_split_path"""
    T64, G64 = ci.offset(n, d, 0)
    ref64 = orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)
    ref32 = orc.svgd_step(T64, G64, orc.AdagradState(), np.float32)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    phi = tc._np(_folded(n, d, cuda).compute_phi(T, G))
    plain = tc._np(SvgdEngine(n, d, device=cuda, fold=False, small=False).compute_phi(T, G))
    e_gpu, e_o32 = ci.frobenius_error(phi, ref64["phi"]), ci.frobenius_error(ref32["phi"], ref64["phi"])
    print("fold offset %dx%d: folded %.2e, unfolded %.2e, fp32 oracle %.2e (all against fp64)" %
          (n, d, e_gpu, ci.frobenius_error(plain, ref64["phi"]), e_o32))
    assert np.isfinite(phi).all()
    assert e_gpu <= max(5 * e_o32, 1e-5), (e_gpu, e_o32)


# ---------------------------------------------------------------------------------------------------------------
# 2. folded against unfolded at the sizes the gate is about
# ---------------------------------------------------------------------------------------------------------------
def _sampled_fp64(T, G, h2, rows):
    """phi of the sampled rows in torch fp64 on the device, from the engine's bandwidth (what bench.parity_sample does)"""
    n = T.shape[0]
    Td, Gd = T.double(), G.double()
    Ts = Td[rows]
    D = (Ts * Ts).sum(1)[:, None] + (Td * Td).sum(1)[None, :] - 2.0 * Ts @ Td.T
    K = torch.exp(-D / (2.0 * h2))
    return (K @ Gd + (K.sum(1)[:, None] * Ts - K @ Td) / h2) / n


@pytest.mark.parametrize("n,d", [(4096, 256), (16384, 256)])
def test_folded_against_unfolded(cuda, n, d):
    gen = torch.Generator(device="cpu").manual_seed(3)
    T = torch.randn(n, d, generator=gen).to(cuda)
    G = torch.randn(n, d, generator=gen).to(cuda)
    a, b = SvgdEngine(n, d, device=cuda, fold=True), SvgdEngine(n, d, device=cuda, fold=False)
    assert a.fold and not b.fold
    pa, pb = a.compute_phi(T, G).clone(), b.compute_phi(T, G).clone()
    assert torch.equal(a.h2, b.h2)
    rows = torch.arange(0, n, n // 48, device=cuda)[:48]
    ref = _sampled_fp64(T, G, float(a.h2.item()), rows)
    ea = ((pa[rows].double() - ref).norm() / ref.norm()).item()
    eb = ((pb[rows].double() - ref).norm() / ref.norm()).item()
    diff = ((pa - pb).double().norm() / pb.double().norm()).item()
    print("fold %dx%d: against fp64 on 48 rows folded %.3e, unfolded %.3e; folded - unfolded (Frobenius) %.3e" % (n, d, ea, eb, diff))
    assert ea <= min(2.0 * eb, 1e-5), (ea, eb)


# ---------------------------------------------------------------------------------------------------------------
# 3. bit-identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(700, 300), (1024, 256), (1536, 130), (640, 2001)])
def test_bit_identity(cuda, n, d):
    T64, G64, ref = tc._case("graded", n, d) if (n, d) in tc.SHAPES else (None, None, None)
    if T64 is None:
        T64, G64 = ci.make("graded", n, d, 0)
        ref = orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    plain, withdk, withksd, miss = _folded(n, d, cuda), _folded(n, d, cuda), _folded(n, d, cuda, ksd=True), _folded(n, d, cuda, window=False)
    dK = torch.full((n, d), float("nan"), device=cuda)
    for call in range(3):
        p0 = plain.compute_phi(T, G).clone()
        p0b = plain.compute_phi(T, G).clone()
        p1 = withdk.compute_phi(T, G, dK_out=dK).clone()
        p2 = withksd.compute_phi(T, G).clone()
        p3 = miss.compute_phi(T, G).clone()
        torch.cuda.synchronize()
        assert torch.equal(p0, p0b), "same inputs, different bits"
        assert torch.equal(p0, p1) and torch.equal(plain.h2, withdk.h2) and torch.equal(plain.sqnorm, withdk.sqnorm), "dK_out changes phi"
        assert torch.equal(p0, p2) and torch.equal(plain.h2, withksd.h2) and torch.equal(plain.sqnorm, withksd.sqnorm), "ksd changes phi"
        assert torch.equal(p0, p3) and torch.equal(plain.h2, miss.h2), "window hit and miss differ"
    terms = ref["K"].sum(1)[:, None] / ref["h2"]
    tc._check_columns("fold graded %dx%d" % (n, d), tc._np(dK), ref["dK"], T64, "dK", scale_terms=terms)


@pytest.mark.parametrize("family", ["graded", "spike"])
@pytest.mark.parametrize("n,d", tc.SHAPES)
def test_ksd(cuda, family, n, d):
    """test_gpu_conditioning.test_ksd_on_graded_and_spiked_scores on the folded contraction: K.G is no longer held, the
    statistic's og is ow + ot / h2 in fp64"""
    from test_gpu_ksd import TOL_F32, _errors
    T64, G64 = ci.make(family, n, d, 0)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    withk = _folded(n, d, cuda, ksd=True)
    for call in range(3):
        withk.compute_phi(T, G)
    errs, _ = _errors(withk, T, G)
    print("fold ksd %s %dx%d: err/scale S %.2e S_diag %.2e U %.2e V %.2e" % ((family, n, d) + errs))
    assert max(errs) <= TOL_F32, errs


# ---------------------------------------------------------------------------------------------------------------
# 4. exact power-of-two equivariance: theta * 2^a, score * 2^-a  =>  W * 2^-a, phi * 2^-a
# ---------------------------------------------------------------------------------------------------------------
def test_power_of_two_scaling_moves_exponents_only(cuda):
    n, d = 1024, 256
    T64, G64 = ci.make("graded", n, d, 0)
    eng = _folded(n, d, cuda)
    base = eng.compute_phi(tc._dev(T64, cuda), tc._dev(G64, cuda)).clone()
    h2 = eng.h2.clone()
    assert torch.isfinite(base).all()
    for a in (-30, -7, 9, 30):
        T2, G2 = ci.f32(T64 * 2.0 ** a), ci.f32(G64 * 2.0 ** -a)
        assert np.array_equal(T2 * 2.0 ** -a, T64) and np.array_equal(G2 * 2.0 ** a, G64)
        got = eng.compute_phi(tc._dev(T2, cuda), tc._dev(G2, cuda))
        assert torch.equal(eng.h2, h2 * float(4.0 ** a)), a
        assert torch.equal(got * float(2.0 ** a), base), (a, int((got * float(2.0 ** a) != base).sum()))


# ---------------------------------------------------------------------------------------------------------------
# 5. degenerate inputs
# ---------------------------------------------------------------------------------------------------------------
def test_identical_particles_give_nan(cuda):
    n, d = 700, 300
    rng = np.random.default_rng(7)
    T = tc._dev(np.tile(rng.normal(size=(1, d)), (n, 1)), cuda)
    G = tc._dev(rng.normal(size=(n, d)), cuda)
    for kw in ({}, {"ksd": True}):
        eng = _folded(n, d, cuda, **kw)
        dK = torch.zeros(n, d, device=cuda)
        phi = eng.compute_phi(T, G, dK_out=dK)
        torch.cuda.synchronize()
        print("identical particles: h2 = %r" % eng.h2.item())
        assert torch.isnan(phi).all(), "h2 = 0 must give NaN phi, as on every other path"
    other = SvgdEngine(n, d, device=cuda, fold=False, small=False)
    assert torch.isnan(other.compute_phi(T, G)).all()


def test_zero_score_column_and_constant_theta_column(cuda):
    n, d = 1024, 256
    T64, G64, ref = tc._case("zero_const", n, d)
    eng = _folded(n, d, cuda)
    dK = torch.empty(n, d, device=cuda)
    phi = tc._np(eng.compute_phi(tc._dev(T64, cuda), tc._dev(G64, cuda), dK_out=dK))
    err, live = ci.column_errors(phi, ref["phi"])
    zs, ct = ci.zero_score_cols(d), ci.constant_theta_cols(T64)
    print("fold zero_const: zero score columns %s err %s; constant theta columns %s err %s" % (zs, err[zs], list(ct), err[ct]))
    assert np.isfinite(phi).all() and err[live].max() <= TOL
    assert not tc._np(dK)[:, ci.ZERO_THETA_COL].any()


# ---------------------------------------------------------------------------------------------------------------
# 6. the gate
# ---------------------------------------------------------------------------------------------------------------
def test_default_gate(cuda):
    """A default engine folds at C3 and does not at 2048 x 32, nor at any shape of the fused-vs-staged bit-identity tests;
    bf16 inputs, the fp32-MFMA kernels and row blocks never do.  Told by stein_layout_folds and, after a step, by the
    workspace word the call leaves (include/steinhip.h, STEIN_FLAG_FOLD)."""
    def folds(n, d, flags=_lib.FLAG_X3, dtype=_lib.F32, nl=None):
        return int(_lib.layout_folds(nl or n, n, d, dtype, flags))
    assert folds(16384, 256) == 1 and folds(131072, 256) == 1
    for n, d in ((2048, 32), (4608, 24), (2304, 24), (1536, 256)):
        assert folds(n, d) == 0, (n, d)
        assert folds(n, d, _lib.FLAG_X3 | _lib.FLAG_FOLD) == 1
    assert folds(4096, 256) == 1 and folds(8192, 2001) == 1
    assert folds(8192, 128) == 0 and folds(4096, 128) == 0      # one 128-column block: nothing to halve (measured slower)
    assert folds(16384, 256, _lib.FLAG_X3 | _lib.FLAG_NO_FOLD) == 0
    assert folds(16384, 256, 0) == 0 and folds(16384, 256, _lib.FLAG_X3 | _lib.FLAG_FOLD, _lib.BF16) == 0
    assert folds(16384, 256, _lib.FLAG_X3 | _lib.FLAG_FOLD | _lib.FLAG_TILED, nl=8192) == 0
    assert folds(100, 10, _lib.FLAG_X3 | _lib.FLAG_FOLD) == 0          # the one-kernel path
    for n, d, want in ((16384, 256, 1), (2048, 32, 0)):
        eng = SvgdEngine(n, d, device=cuda)
        assert eng.fold == bool(want)
        eng.compute_phi(torch.randn(n, d, device=cuda), torch.randn(n, d, device=cuda))
        word = eng.select_state_bytes(_lib.FUSE_FOLDED_OFFSET, 4).view(torch.int32).item()
        assert word == want, (n, d, word)
    # the default gate never grows a workspace or moves a section
    for n, d in ((16384, 256), (131072, 256), (8192, 2001), (4096, 256), (8192, 256)):
        a, b = _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3), _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_NO_FOLD)
        assert a[:2] == b[:2], (n, d)
