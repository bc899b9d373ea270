"""GPU: the Stein-kernel matrix k_ksd_boot forms, read out of the device element by element, and planted inputs whose
answer is exact in every bit (stein_ksd_matmul and stein_ksd_boot, include/steinhip.h; stein_amd/csrc/stein_boot.hip).

1. With V = I (reps = n, row b = e_b) stein_ksd_matmul returns out[b][i] = u_p(x_i, x_b): one nonzero product per sum, so
   the contraction is exact and `out` is the device's element function after the hi + lo image -- every one of the n^2 lane
   positions of every tile by itself.  It is held to the fp32-faithful model of tests/stein_u_model.py, per 128 x 128 block
   (row tile x j tile) and for the whole matrix, in Frobenius norm:
       |U_gpu - U_64| <= 5 max(|U_model - U_64|, 2^-24 |M|)
   (U_64: boot_ref.pairwise_u; M: boot_ref.element_model's magnitudes; 5: the project's factor for "GPU against the
   fp32-faithful model's own error").  tests/test_stein_u_model.py shows the model within 16 x 2^-24 |M|, so this is about
   three orders of magnitude below the worst-case allowance test_gpu_kernel_products.py holds the same kernel to: a wrong
   constant at the 10^-6 level, a lane that reads its neighbour's b_j or a lo plane dropped in one block fails it.
   On the same extraction, exactly: every forced j split returns the default plan's bits (the other ranges' partials are
   exact zeros), and the same e_b at three rows of V (another wave, another 128-block, another column group) returns the
   same row three times.  Within the blocks' tolerance: the diagonal against the rows' shares |g_i|^2 + d / h2 (or d / 2 h2)
   of stein_ksd_boot's diag_out, and U_gpu against its transpose (element (i, j) and (j, i) come from different waves and
   tiles): twice the block's tolerance.
   Shapes: n = 2, 129, 257, 300 (one, two and three row tiles with ragged last rows; reps = n reaches three 128-blocks and
   two column groups), d = 1, 3, 33, 130 (one, two and five k tiles).
2. The planted inputs of tests/planted_cases.py (proved on the CPU by test_planted_cases.py): q_out and out equal the
   integer reference exactly, at the default plan and at j splits 1, 2 and 3, for reps = 1, 33, 129, 257.  This pins the
   contraction, the row and column masks, the j split sum and both tails.
Measured on the MI355X (printed; run with -s): DESIGN.md section 6i.
"""
import functools

import numpy as np
import pytest

import boot_ref as B
import planted_cases as P
import stein_u_model as S
from test_gpu_boot import _forms
from test_gpu_kernel_products import _dev, _products

pytestmark = pytest.mark.gpu
SPLITS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def reference(n, d, kernel):
    """(X, G, h2, U_64, M, U_model, the chained diagnostic), computed once and shared -- read-only"""
    X, G, h2 = S.plain_inputs(n, d)
    U, M, _ = B.element_model(X, G, h2, kernel)
    return X, G, h2, U, M, S.model_u(X, G, h2, kernel), S.model_u(X, G, h2, kernel, mfma_chain=True)


def extract(T, Sc, h2, kernel, jsplit=0):
    """U_gpu [n, n]: element (i, j) = out[j][i] of the product with V = I"""
    V, = _dev(T.device, S.unit_rows(T.shape[0]))
    return _products(T, Sc, h2, kernel, V, jsplit=jsplit).T.astype(np.float64)


def check_elements(tag, U_gpu, U_model, U64, M, U_chain=None):
    """the block-wise yardstick against U_model (Grams rounded once), then the transpose within twice it; U_chain: the
    model with the matrix cores' roundings, printed beside it and not asserted"""
    assert np.isfinite(U_gpu).all(), tag
    if U_chain is not None:
        diag = S.block_report(U_gpu, U_chain, U64, M)
        print("%s, against the chained Grams (not asserted): largest block %.3g, whole matrix %.3g;  bit-equal elements %.3f"
              % (tag, diag.ratio_blocks, diag.ratio_whole, (U_gpu == U_chain).mean()))
    rep = S.block_report(U_gpu, U_model, U64, M)
    S.assert_within(tag, rep)
    for ti, tj, _, tol in rep.blocks:
        s = (slice(ti * S.TILE, (ti + 1) * S.TILE), slice(tj * S.TILE, (tj + 1) * S.TILE))
        asym = np.linalg.norm(U_gpu[s] - U_gpu.T[s])
        assert asym <= 2.0 * tol, (tag, "transpose", ti, tj, asym / tol)
    return rep


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", S.SHAPES)
def test_every_element_against_the_fp32_model(cuda, n, d, kernel):
    X, G, h2, U64, M, Um, Uc = reference(n, d, kernel)
    T, Sc = _dev(cuda, X, G)
    tag = "elements %dx%d %s" % (n, d, kernel)
    U_gpu = extract(T, Sc, h2, kernel)
    rep = check_elements(tag, U_gpu, Um, U64, M, Uc)
    for k in SPLITS:                             # the other ranges' partials are exact zeros: the same bits
        assert np.array_equal(U_gpu, extract(T, Sc, h2, kernel, jsplit=k)), k
    # the diagonal against the per-row shares of diag_out, tile by tile within the diagonal block's tolerance
    share = (G.astype(np.float64) ** 2).sum(1) + d / (h2 if kernel == "rbf" else 2.0 * h2)
    tols = {(ti, tj): tol for ti, tj, _, tol in rep.blocks}
    for t in range((n + S.TILE - 1) // S.TILE):
        s = slice(t * S.TILE, (t + 1) * S.TILE)
        assert np.linalg.norm(np.diag(U_gpu)[s] - share[s]) <= tols[(t, t)], (tag, "diagonal", t)
    W, = _dev(cuda, np.ones((1, n), np.float32))
    _, diag = _forms(T, Sc, h2, kernel, W)
    assert abs(diag - share.sum()) <= (d + 8) * 2.0 ** -50 * share.sum()
    assert abs(np.diag(U_gpu).sum() - diag) <= np.sqrt(n) * sum(tols[(t, t)] for t in range((n + S.TILE - 1) // S.TILE))


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", [(300, 33), (257, 130), (129, 3)])
def test_a_unit_row_gives_the_same_bits_at_every_row_of_v(cuda, n, d, kernel):
    """e_b at row 1, row 200 and row 290 of V (n = 300; scaled down for the smaller n): another wave, another 128-block,
    another column group -- and at every forced j split"""
    X, G, h2 = reference(n, d, kernel)[:3]
    T, Sc = _dev(cuda, X, G)
    U_gpu = extract(T, Sc, h2, kernel)
    rows = (1, 200, 290) if n >= 291 else (1, n // 2, n - 1)
    V = S.unit_rows(n).copy()
    cols = (7, n - 1, n // 2 + 1)                # a column of the first j tile, the last ragged one, one in between
    for k in (0,) + SPLITS:
        for b in cols:
            V[list(rows)] = 0.0
            V[list(rows), b] = 1.0
            Vd, = _dev(cuda, V)
            out = _products(T, Sc, h2, kernel, Vd, jsplit=k).astype(np.float64)
            for row in rows:
                assert np.array_equal(out[row], U_gpu[:, b]), (k, b, row)


@pytest.mark.parametrize("kernel", B.KERNELS)
@pytest.mark.parametrize("n,d", P.SHAPES)
def test_planted_inputs_exactly(cuda, n, d, kernel):
    X, G = P.inputs(n, d)
    U = P.closed_form(G, kernel)
    T, Sc = _dev(cuda, X, G)
    assert np.array_equal(extract(T, Sc, P.H2, kernel), U)
    for reps in P.REPS:
        W, V = P.weights(n, reps), P.factors(n, reps)
        Wd, Vd = _dev(cuda, W, V)
        want_q, want_out = P.expected_forms(U, W), P.expected_products(U, V)
        for k in P.SPLITS:
            q, diag = _forms(T, Sc, P.H2, kernel, Wd, jsplit=k)
            assert np.array_equal(q, want_q), (reps, k, np.flatnonzero(q != want_q)[:8])
            assert diag == np.trace(U)
            out = _products(T, Sc, P.H2, kernel, Vd, jsplit=k)
            assert out.dtype == np.float32
            assert np.array_equal(out.astype(np.float64), want_out), (reps, k, np.argwhere(out != want_out)[:8])
