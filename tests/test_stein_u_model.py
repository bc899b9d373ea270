"""CPU: what tests/stein_u_model.py claims, so that the tolerance the GPU element tests derive from it is attainable.

1. The model stays inside boot_ref's per-element allowance a_ij everywhere: on the plain inputs at the extraction's shapes
   and on every conditioning family, with both Gram models.
2. Its error against fp64 is where an fp32 evaluation belongs.  Between the inputs and one element the kernel rounds about
   sixteen times (r_i, r_j, their sum, S, dv, the exponent's product, exp2 or rsq and its powers, the score Gram, b_i, b_j,
   their sum, three additions in the bracket, the product with k; the image's 2^-22 counts as four), each by at most 2^-24
   of a term's magnitude: 16 x 2^-24 |M|_F in the worst case.  Measured on the plain inputs: 0.4 to 1.9 x 2^-24 |M|_F, three
   orders of magnitude below a_ij (largest |err| / a_ij 0.25 at 129 x 3, below 0.04 elsewhere).
3. What fp32 can deliver on the conditioning families, per family: the model's |Q_b - Q_b(fp64)| / |Q_b| for a row of ones
   plus seven sign rows at the median bandwidth, beside allowance / |Q_b|.  Printed (run with -s), asserted inside the
   allowance.  Measured at 129 x 33 and 150 x 5: graded, zero_const, spike, far10, far100 at most 4.1e-7; the +10
   translation 1.4e-5; offset 2.6e-4, where the allowance is 0.16 to 4.9 (IMQ) and 47 to 5500 (RBF) times |Q_b| and says
   nothing.
"""
import functools

import numpy as np
import pytest

import boot_ref as B
import conditioning_inputs as ci
import stein_u_model as S

FAMILIES = ci.FAMILIES + ("offset", "+10")
COND_SHAPES = [(129, 33), (150, 5)]
ROUNDINGS = 16


def family_inputs(family, n, d):
    X, G = S.translated(n, d) if family == "+10" else ci.make(family, n, d)
    return X, G, B.median_h2(X)


def eight_rows(n):
    """a row of ones plus seven sign rows"""
    W = B.sign_rows(8, n, 77)
    W[0] = 1.0
    return W


@functools.lru_cache(maxsize=None)
def _both(kind, n, d, kernel):
    X, G, h2 = S.plain_inputs(n, d) if kind == "plain" else family_inputs(kind, n, d)
    return X, G, h2, B.element_model(X, G, h2, kernel)


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", S.SHAPES)
def test_plain_inputs_inside_the_allowance_and_at_fp32_level(n, d, kernel):
    X, G, h2, (U, M, a) = _both("plain", n, d, kernel)
    for chain in (False, True):
        Um = S.model_u(X, G, h2, kernel, mfma_chain=chain)
        err = np.linalg.norm(Um - U) / (S.U32 * np.linalg.norm(M))
        print("model %dx%d %s %s: |U_model - U_64| = %.3g x 2^-24 |M|, largest |err| / a_ij %.3g"
              % (n, d, kernel, "chain" if chain else "once", err, (np.abs(Um - U) / a).max()))
        assert np.all(np.abs(Um - U) <= a)
        assert err <= ROUNDINGS
    # without the image the values are fp32; with it they are what hi + lo fp16 hold: within 2^-22 of each other
    u32 = S.model_u(X, G, h2, kernel, with_image=False)
    assert np.array_equal(u32.astype(np.float32).astype(np.float64), u32)
    Um = S.model_u(X, G, h2, kernel)
    assert np.all(np.abs(Um - u32) <= 2.0 ** -22 * np.abs(u32) + 2.0 ** -37 * B.device_bound(X, G, h2, kernel))
    once = S.model_u(X, G, h2, kernel, mfma_chain=False)
    assert np.array_equal(once, once.T)          # rounded once, the model is symmetric; the chained Grams need not be


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", COND_SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_conditioning_families_inside_the_allowance(family, n, d, kernel):
    X, G, h2, (U, M, a) = _both(family, n, d, kernel)
    W = eight_rows(n)
    f = B.quadratic_forms(X, G, h2, kernel, W)
    for chain in (False, True):
        Um = S.model_u(X, G, h2, kernel, mfma_chain=chain)
        assert np.isfinite(Um).all()
        assert np.all(np.abs(Um - U) <= a), (family, (np.abs(Um - U) / a).max())
        q = S.forms(Um, W)
        print("model %s %dx%d %s %s: |Q_model - Q_64| / |Q| %.2g (/ scale %.2g);  allowance / |Q| %.2g .. %.2g (/ scale %.2g);  "
              "|U_model - U_64| = %.3g x 2^-24 |M|"
              % (family, n, d, kernel, "chain" if chain else "once", (np.abs(q - f.q) / np.abs(f.q)).max(),
                 (np.abs(q - f.q) / f.scale).max(), (f.allow / np.abs(f.q)).min(), (f.allow / np.abs(f.q)).max(),
                 (f.allow / f.scale).max(), np.linalg.norm(Um - U) / (S.U32 * np.linalg.norm(M))))
        assert np.all(np.abs(q - f.q) <= f.allow)


def test_the_split_restatement_and_the_wave_sum():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((5, 130)).astype(np.float32) * 37.0
    hi, lo, s = S.split_planes(A)
    assert 2.0 ** 13 <= np.abs(A).max() * 2.0 ** s < 2.0 ** 14
    back = (hi + lo) * 2.0 ** -s
    assert np.all(np.abs(back - A) <= 2.0 ** -22 * np.abs(A) + 2.0 ** -38 * np.abs(A).max())
    assert np.array_equal(hi.astype(np.float16).astype(np.float64), hi) and np.array_equal(lo.astype(np.float16).astype(np.float64), lo)
    got = S.wave_dot(A.astype(np.float64), A.astype(np.float64))
    want = (A.astype(np.float64) ** 2).sum(1)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
    assert np.all(np.abs(got - want) <= (3 + 6) * 2.0 ** -24 * want)       # three fmas per lane, six shuffle additions
    # small integers: every sum is exact
    Z = rng.integers(-4, 5, (3, 70)).astype(np.float64)
    assert np.array_equal(S.wave_dot(Z, Z), (Z * Z).sum(1))
    # one model of the Gram or the other: the same values where nothing rounds
    p = S.split_planes(Z)[:2]
    assert np.array_equal(S.gram(p, p, True), S.r32(S.gram(p, p, False)))
    assert S.MFMA_PASS == 8 and 32 % S.MFMA_PASS == 0


def test_unit_rows_and_the_block_report():
    n = 130
    rng = np.random.default_rng(2)
    U64 = rng.standard_normal((n, n))
    M = np.abs(U64) + 1.0
    model = U64 + 1e-6 * rng.standard_normal((n, n))
    assert np.array_equal(S.unit_rows(3), np.eye(3, dtype=np.float32))
    rep = S.block_report(model, model, U64, M)
    assert len(rep.blocks) == 4 and abs(rep.ratio_whole - 1.0) < 1e-12 and abs(rep.ratio_blocks - 1.0) < 1e-12
    S.assert_within("self", rep)
    # one bad entry in the ragged corner block: the whole matrix dilutes it, its block does not
    bad = model.copy()
    bad[129, 129] += 1e-4
    rep = S.block_report(bad, model, U64, M)
    assert rep.whole[0] <= rep.whole[1]
    with pytest.raises(AssertionError):
        S.assert_within("corner", rep)
    # the floor: a model that happens to be exact demands one fp32 rounding of the magnitudes, not zero
    rep = S.block_report(U64 + S.U32 * M, U64, U64, M)
    S.assert_within("floor", rep)
