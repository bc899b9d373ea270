"""CPU: the row-sum form of the Stein discrepancy sums (tests/stream_ksd_ref.py, what stein_svgd_phi_stream_ksd evaluates
from K.W, rowsum(K) and rowsum(K o D), without K.theta) against the fp64 pair sum of tests/ksd_ref.py.

Errors are over ksd_ref's scale, sum_ij |terms of u_ij|.  In fp64 the two forms agree to rounding (bound 1e-12: n^2 d
terms of relative error 2^-53 each would give ~1e-13 at the largest shape if they all added up).  With the distances and
the three fp32 sums of the library rounded to fp32 (each a relative 2^-24 = 6e-8 on a quantity of at most the scale's size)
the bound is 1e-7.  This emulation gives at most 4.0e-8 (129 x 1 at a quarter of the median's h2; below 5e-9 elsewhere): it
rounds the distances that are exponentiated, which weighs most where h2 is small and n is (an emulation with 2^-22 noise on
K, W and S instead gave at most 1.3e-8 on the same shapes)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksd_ref as R  # noqa: E402
import stream_ksd_ref as SR  # noqa: E402
from test_gpu_ksd import _inputs  # noqa: E402

SHAPES = [(129, 1), (130, 5), (257, 129), (384, 260)]
FACTORS = (0.25, 1.0, 4.0)


@pytest.fixture(scope="module")
def cases():
    """shape -> (theta, score, median h2, {factor: (S, S_diag, scale)}), computed once"""
    out = {}
    for n, d in SHAPES:
        T, G = _inputs(n, d, n + d, "cpu")
        T, G = T.double(), G.double()
        med = R.median_h2(T)
        out[(n, d)] = (T, G, med, {f: R.pairwise_sums(T, G, f * med) for f in FACTORS})
    return out


@pytest.mark.parametrize("n,d", SHAPES)
def test_row_sum_form_is_the_pair_sum_in_fp64(cases, n, d):
    T, G, med, refs = cases[(n, d)]
    for f in FACTORS:
        S, Sd, scale = refs[f]
        gS, gSd = SR.rowsum_sums(T, G, f * med)
        print("identity %dx%d h2 x%g: S %.2e S_diag %.2e of the scale" % (n, d, f, abs(gS - S) / scale, abs(gSd - Sd) / scale))
        assert abs(gS - S) <= 1e-12 * scale and abs(gSd - Sd) <= 1e-12 * scale, (n, d, f)


@pytest.mark.parametrize("n,d", SHAPES)
def test_fp32_sums_keep_the_statistic(cases, n, d):
    T, G, med, refs = cases[(n, d)]
    for f in FACTORS:
        S, Sd, scale = refs[f]
        gS, gSd = SR.rowsum_sums(T, G, f * med, round32=True)
        print("fp32 sums %dx%d h2 x%g: S %.2e of the scale" % (n, d, f, abs(gS - S) / scale))
        assert abs(gS - S) <= 1e-7 * scale and abs(gSd - Sd) <= 1e-12 * scale, (n, d, f)


def test_u_statistic_of_one_pair_by_hand():
    """n = 2, d = 1: x = (0, 1), g = (1, -1), h2 = 1: k = exp(-1/2), u_12 = k (g1 g2 + (g1 - g2)(x1 - x2) + 1 - 1) = -3 k"""
    X, G = torch.tensor([[0.0], [1.0]]), torch.tensor([[1.0], [-1.0]])
    S, Sd = SR.rowsum_sums(X, G, 1.0)
    k = float(torch.exp(torch.tensor(-0.5, dtype=torch.float64)))
    assert abs(Sd - 4.0) < 1e-14            # u_ii = g_i^2 + d / h2 = 2 each
    assert abs((S - Sd) - 2.0 * (-3.0 * k)) < 1e-14
