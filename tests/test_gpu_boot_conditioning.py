"""GPU: stein_ksd_boot and stein_ksd_matmul on badly scaled, degenerate and non-finite inputs (include/steinhip.h;
stein_amd/csrc/stein_boot.hip).

1. The families of tests/conditioning_inputs.py (graded, zero_const, spike, far10, far100, offset) and a plain translation
   N(0, I) + 10 with G = -X, at 129 x 33 and 150 x 5, a row of ones plus seven sign rows, the median bandwidth: every
   quadratic form and every product is finite and inside boot_ref's / weights_ref's allowance, unchanged.
   The element extraction of test_gpu_stein_u_elements.py at 129 x 33, with the same factor-5 yardstick against the
   fp32-faithful model.  ON offset AND far100 THIS IS THE ONLY CHECK THAT SAYS ANYTHING: there the allowance is 0.06 to 5500
   times |Q_b| itself (an SVGD posterior is exactly such a tight cluster away from the origin, where D = r_i + r_j - 2 x_i.x_j
   and the b_i cancel), while the model is within 10^-3 of |Q_b| (tests/test_stein_u_model.py).
   Measured (allowance / scale and error / scale per family, printed; run with -s): DESIGN.md section 6h.
2. Powers of two.  u_p is not equivariant under conditioning_inputs.pow2's per-column score exponents (g_i.g_j mixes the
   columns), so those inputs are one more family held to the allowance.  What the code does guarantee: theta times 2^a, the
   score times 2^-a and h2 times 2^(2a) multiply every term of u_p by 2^(-2a) exactly -- every operand's scale exponent moves,
   no significand does, the image's scale follows its bound -- so q_out, diag_out and out are the unscaled call's bits with
   another exponent.  Asserted exactly, for a = 7 and -9 (no term leaves the normal range; the scale exponents stay inside
   their clamps).
3. Non-finite inputs never give a finite answer (the header's contract: every output NaN, status STEIN_OK): one NaN in
   score[p], one in theta[p], one +Inf in score[p], p in the first tile, in the last ragged tile and at n - 1, at 129 x 3 and
   257 x 33; h2 = 0 and h2 = NaN; a finite theta row whose |x|^2 overflows fp32.  The guard behind `out` stays untouched
   (_products asserts it); stein_goodness_of_fit returns a NaN p-value, not the 1 / (n_boot + 1) of "no replicate >= NaN".  Before k_boot_scale
   poisoned the out-scale, the element function's clamp turned such an entry into a finite +-60000 of the image.
"""
import functools

import numpy as np
import pytest

import boot_ref as B
import conditioning_inputs as ci
import stein_u_model as S
import weights_ref as R
from test_gpu_boot import _forms
from test_gpu_kernel_products import _dev, _products
from test_gpu_stein_u_elements import check_elements, extract
from test_stein_u_model import COND_SHAPES, FAMILIES, eight_rows, family_inputs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(family, n, d, kernel):
    """(X, G, h2, W, forms, model, products, allowance) in fp64, computed once and shared -- read-only"""
    X, G, h2 = family_inputs(family, n, d)
    W = eight_rows(n)
    m = R.Model(X, G, h2, kernel)
    out, allow = m.products(W)
    return X.astype(np.float32), G.astype(np.float32), h2, W, B.quadratic_forms(X, G, h2, kernel, W), m, out, allow


def _check_both(tag, cuda, X, G, h2, kernel, W, f, want, allow):
    T, Sc, Wd = _dev(cuda, X, G, W)
    q, diag = _forms(T, Sc, h2, kernel, Wd)
    out = _products(T, Sc, h2, kernel, Wd).astype(np.float64)
    rq, ro = np.abs(q - f.q) / f.allow, np.abs(out - want) / allow
    print("conditioning %s: forms allowance / scale %.2g, |err| / scale %.2g, |err| / |Q| %.2g, |err| / allowance %.2g;  "
          "products |err| / allowance %.2g"
          % (tag, (f.allow / f.scale).max(), (np.abs(q - f.q) / f.scale).max(), (np.abs(q - f.q) / np.abs(f.q)).max(), rq.max(),
             ro.max()))
    assert np.isfinite(q).all() and np.isfinite(out).all() and np.isfinite(diag), tag
    assert (rq <= 1.0).all(), (tag, rq.max())
    assert (ro <= 1.0).all(), (tag, ro.max())
    assert abs(diag - f.diag) <= (X.shape[1] + 8) * 2.0 ** -50 * f.diag
    return q, diag, out


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", COND_SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_forms_and_products_inside_their_allowance(cuda, family, n, d, kernel):
    X, G, h2, W, f, m, want, allow = reference(family, n, d, kernel)
    _check_both("%s %dx%d %s" % (family, n, d, kernel), cuda, X, G, h2, kernel, W, f, want, allow)


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_element_against_the_fp32_model(cuda, family, kernel):
    """on offset and far100 the only check that says anything (module docstring)"""
    n, d = 129, 33
    X, G, h2, W, f, m, want, allow = reference(family, n, d, kernel)
    T, Sc = _dev(cuda, X, G)
    check_elements("elements %s %dx%d %s" % (family, n, d, kernel), extract(T, Sc, h2, kernel),
                   S.model_u(X, G, h2, kernel), m.U, m.M, S.model_u(X, G, h2, kernel, mfma_chain=True))


@pytest.mark.parametrize("kernel", B.KERNELS)
def test_per_column_powers_of_two_inside_the_allowance(cuda, kernel):
    n, d = 150, 5
    T0, G0 = ci.make("graded", n, d)
    X, G, b = ci.pow2(T0, G0, -7, lo=-20, hi=20)     # on top of graded's own 2^-20 .. 2^-16: |g|^2 stays inside fp32
    h2 = B.median_h2(X)
    W = eight_rows(n)
    want, allow = R.Model(X, G, h2, kernel).products(W)
    _check_both("pow2 %dx%d %s" % (n, d, kernel), cuda, X.astype(np.float32), G.astype(np.float32), h2, kernel, W,
                B.quadratic_forms(X, G, h2, kernel, W), want, allow)


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("family", ["graded", "offset", "+10"])
def test_a_uniform_power_of_two_moves_exponents_only(cuda, family, kernel):
    n, d = 129, 33
    X, G, h2, W, f, m, want, allow = reference(family, n, d, kernel)
    T, Sc, Wd = _dev(cuda, X, G, W)
    q, diag = _forms(T, Sc, h2, kernel, Wd)
    out = _products(T, Sc, h2, kernel, Wd)
    for a in (7, -9):
        Xa, Ga, h2a = (X * np.float32(2.0 ** a)), (G * np.float32(2.0 ** -a)), h2 * 2.0 ** (2 * a)
        assert np.array_equal(np.frexp(Xa)[0], np.frexp(X)[0]) and np.array_equal(np.frexp(Ga)[0], np.frexp(G)[0])
        assert B.f32(h2a) == h2a
        Ta, Sa = _dev(cuda, Xa, Ga)
        qa, diag_a = _forms(Ta, Sa, h2a, kernel, Wd)
        out_a = _products(Ta, Sa, h2a, kernel, Wd)
        assert np.array_equal(qa * 2.0 ** (2 * a), q), a
        assert diag_a * 2.0 ** (2 * a) == diag
        assert np.array_equal(out_a.astype(np.float64) * 2.0 ** (2 * a), out.astype(np.float64)), a


# ---- non-finite inputs ---------------------------------------------------------------------------------------------------
def _all_nan(tag, cuda, X, G, h2, kernel):
    n = X.shape[0]
    W = eight_rows(n)
    T, Sc, Wd = _dev(cuda, X, G, W)
    q, diag = _forms(T, Sc, h2, kernel, Wd)
    assert np.isnan(q).all() and np.isnan(diag), (tag, q, diag)
    out = _products(T, Sc, h2, kernel, Wd)             # (asserts the guard behind out)
    assert np.isnan(out).all(), (tag, int(np.isfinite(out).sum()))
    Vd, = _dev(cuda, S.unit_rows(n))
    for k in (0, 1, 3):
        assert np.isnan(_products(T, Sc, h2, kernel, Vd, jsplit=k)).all(), (tag, k)


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", [(129, 3), (257, 33)])
def test_a_non_finite_entry_gives_nan_everywhere(cuda, n, d, kernel):
    X0, G0, h2 = S.plain_inputs(n, d)
    # the first tile, a middle tile (n = 257), the last ragged tile -- one row at these n, which is also row n - 1
    for p in sorted({5, n // 2 + 2, (n - 1) // 128 * 128, n - 1}):
        for what, value in (("score", np.nan), ("theta", np.nan), ("score", np.inf)):
            X, G = X0.copy(), G0.copy()
            (G if what == "score" else X)[p, d // 2] = value
            _all_nan("%dx%d %s %s[%d] = %r" % (n, d, kernel, what, p, value), cuda, X, G, h2, kernel)
    # and the unpoisoned inputs still give what they gave: finite, and NaN does not linger in any state
    T, Sc, Wd = _dev(cuda, X0, G0, eight_rows(n))
    assert np.isfinite(_forms(T, Sc, h2, kernel, Wd)[0]).all() and np.isfinite(_products(T, Sc, h2, kernel, Wd)).all()


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("h2", [0.0, float("nan")])
def test_a_zero_or_nan_bandwidth_gives_nan_everywhere(cuda, kernel, h2):
    X, G, _ = S.plain_inputs(129, 3)
    _all_nan("129x3 %s h2 = %r" % (kernel, h2), cuda, X, G, h2, kernel)


@pytest.mark.parametrize("kernel", B.KERNELS)
def test_a_row_norm_beyond_fp32_gives_nan_everywhere(cuda, kernel):
    """finite theta whose |x_p|^2 overflows fp32 while its score row is zero: under IMQ neither |g_p|^2 nor g_p.x_p shows
    it, only r_p = inf does -- and D = inf would make k = 0 and 3 k^2 e a NaN that the clamp turns finite"""
    n, d = 129, 3
    X, G, h2 = S.plain_inputs(n, d)
    X, G = X.copy(), G.copy()
    X[70, 1] = 1e20
    G[70] = 0.0
    _all_nan("129x3 %s |x_70|^2 = inf" % kernel, cuda, X, G, h2, kernel)


@pytest.mark.parametrize("kernel", B.KERNELS)
def test_the_p_value_of_a_sample_with_a_nan_is_nan(cuda, kernel):
    """every form is NaN, so no replicate compares >= the statistic: (1 + 0) / (n_boot + 1) would read as a rejection"""
    import math

    from stein_amd.utilities import stein_goodness_of_fit
    X, G, h2 = S.plain_inputs(129, 3)
    G = G.copy()
    G[5, 1] = np.nan
    T, Sc = _dev(cuda, X, G)
    for statistic in ("v", "u"):
        stat, p = stein_goodness_of_fit(T, Sc, n_boot=31, bandwidth=math.sqrt(h2), kernel=kernel, statistic=statistic)
        assert math.isnan(stat) and math.isnan(p), (statistic, stat, p)
    stat, p = stein_goodness_of_fit(*_dev(cuda, X, -X), n_boot=31, bandwidth=math.sqrt(h2), kernel=kernel)
    assert math.isfinite(stat) and 0.0 < p <= 1.0
