"""CPU: the planted inputs of tests/planted_cases.py give an answer that is exact in every bit, for any order of the sums.

Per case: the fp64 reference (boot_ref.pairwise_u) and the kernel's own algebra in fp32 (stein_u_model.model_u, both Gram
models) equal the closed form bit for bit; every Gram, every element's terms as the kernel forms them, every replicate's
contraction and both tails add multiples of one quantum whose magnitudes sum to less than 2^24 quanta -- the condition under
which an fp32 sum is exact whatever its order.  A case that missed the condition would get smaller integers, never a
relaxed condition."""
import numpy as np
import pytest

import boot_ref as B
import planted_cases as P
import stein_u_model as S


def _multiples(x, q=P.QUANTUM):
    return bool(np.all(np.asarray(x, np.float64) / q == np.round(np.asarray(x, np.float64) / q)))


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", P.SHAPES)
def test_the_reference_and_the_fp32_algebra_equal_the_closed_form(n, d, kernel):
    X, G = P.inputs(n, d)
    assert np.all(X == X[:1]) and X.any() and np.all(X % 2 == 0) and np.abs(X).max() <= 4
    assert np.all(G == np.round(G)) and np.abs(G).max() <= 3 and len(np.unique(G)) == 7
    U = P.closed_form(G, kernel)
    assert _multiples(U)
    assert np.array_equal(B.pairwise_u(X, G, P.H2, kernel), U)
    assert np.array_equal(S.model_u(X, G, P.H2, kernel, mfma_chain=False), U)
    assert np.array_equal(S.model_u(X, G, P.H2, kernel, mfma_chain=True), U)
    # which entries need the image's lo plane: at 257 x 130 under IMQ some do, in both 16-row blocks of a wave
    uv = U * 2.0 ** S.image_exponent(X, G, P.H2, kernel)
    needs_lo = uv.astype(np.float16).astype(np.float64) != uv
    if (n, d, kernel) == (257, 130, "imq"):
        rows = np.flatnonzero(needs_lo.any(1))
        assert (rows % 32 < 16).any() and (rows % 32 >= 16).any() and len(set(rows // 128)) == 3
    total = np.abs(U).sum()
    print("planted %dx%d %s: sum_ij |u_ij| = %.3g (budget %.3g)" % (n, d, kernel, total, P.BUDGET))


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", P.SHAPES)
def test_every_sum_stays_inside_the_exact_range(n, d, kernel):
    X, G = P.inputs(n, d)
    X64, G64 = X.astype(np.float64), G.astype(np.float64)
    # the per-particle sums and the Grams: integers (the planes' power-of-two scales apart) whose magnitudes sum below 2^24
    Wm = G64 - X64 / P.H2
    assert _multiples(Wm, 1.0)
    for a in (X64, G64, Wm):
        assert d * np.abs(a).max() ** 2 < 2.0 ** 24
    r, gx = (X64 * X64).sum(1), (G64 * X64).sum(1)
    assert np.all(r % 4 == 0) and np.all(gx % 2 == 0)
    assert _multiples(gx / P.H2 - r / (2.0 * P.H2 ** 2)) and _multiples(d / (2.0 * P.H2))
    # an element's terms, as the kernel forms them
    Mt = P.term_magnitudes(X, G, kernel)
    U = P.closed_form(G, kernel)
    assert np.all(Mt >= np.abs(U)) and Mt.max() < P.BUDGET
    # the image: u needs no more than the 22 bits hi + lo hold
    assert np.abs(U).max() / P.QUANTUM < 2.0 ** 21
    aU = np.abs(U)
    for reps in P.REPS:
        W, V = P.weights(n, reps), P.factors(n, reps)
        assert set(np.unique(W)) <= {-1.0, 1.0} and np.all(W[0] == 1.0) and set(np.unique(V)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        aw, av = np.abs(W).astype(np.float64), np.abs(V).astype(np.float64)
        # contraction and the forms' tail: every partial sum of sum_ij w_bi w_bj u_ij is bounded by the sum of magnitudes
        assert ((aw @ aU) * aw).sum(1).max() < P.BUDGET
        # the products' row sums sum_j V_bj u_ij, and the result as a float
        assert (av @ aU).max() < P.BUDGET
        assert _multiples(P.expected_forms(U, W)) and _multiples(P.expected_products(U, V))
        assert np.array_equal(P.expected_products(U, V).astype(np.float32).astype(np.float64), P.expected_products(U, V))
