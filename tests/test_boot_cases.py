"""CPU: the KSD-test case table (tests/boot_cases.py) reaches every arm of stein_ksd_boot, its p-value cases are decisive
under the fp64 reference, and the reference itself (tests/boot_ref.py) holds together: the all-ones row is the pair sum of
the Stein kernel that tests/imq_ref.py and the RBF statistic's identity (tests/ksd_ref.py's form) give, and the quantities
the kernel is built from reproduce u_p."""
import numpy as np
import pytest
import torch

import boot_cases as C
import boot_ref as R
import imq_ref

from stein_amd import _lib


def test_the_table_reaches_every_arm():
    arms = [C.arm(c.n, c.d, c.reps) for c in C.CASES]
    assert {a[0] for a in arms} >= {1, 2, 3}                      # row tiles
    assert {a[1] for a in arms} >= {1, 2, 9}                      # k tiles of the Gram products
    assert {a[2] for a in arms} >= {1, 2, 3}                      # replicate blocks: an odd count leaves four waves idle
    assert {a[3] for a in arms} >= {1, 2}                         # column groups
    assert {c.n for c in C.CASES} >= {2, 3, 127, 128, 129, 257, 300}
    assert {c.d for c in C.CASES} >= {1, 3, 31, 32, 33, 260}
    assert {c.reps for c in C.CASES} >= {1, 2, 31, 32, 33, 128, 129, 257}
    for kernel in R.KERNELS:
        assert sum(c.kernel == kernel for c in C.CASES) >= 10
    assert any(c.multinomial for c in C.CASES) and any(c.flip_prob != 0.5 for c in C.CASES)
    assert 20 <= len(C.CASES) <= 30


def test_forced_splits_give_the_plans_the_table_names():
    lib = _lib.load()
    seen = set()
    try:
        for c in C.CASES:
            rt, _, cb, cg = C.arm(c.n, c.d, c.reps)
            for k in c.splits():
                assert lib.stein_debug_boot_jsplit(k) == _lib.OK
                got = _lib.ksd_boot_plan(c.n, c.d, c.reps)
                assert got[:2] == (rt, cg) and 1 <= got[2] <= min(k, rt)
                seen.add(got[2])
    finally:
        assert lib.stein_debug_boot_jsplit(0) == _lib.OK
    assert seen == {1, 2, 3}


@pytest.mark.parametrize("name", [c.name for c in C.P_CASES])
def test_p_value_cases_are_decisive(name):
    c = C.BY_NAME[name]
    _, _, _, W, f = C.reference(name)
    assert np.all(W[0] == 1.0)
    assert R.undecided(f.q, f.allow) == 0
    p = R.p_value(f.q)
    if c.pvalue == "null":
        assert 0.1 < p < 0.9, p
    else:
        assert p == 1.0 / c.reps, p


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_reference_agrees_with_the_other_references(kernel):
    rng = np.random.default_rng(4)
    X = (rng.standard_normal((37, 5)) + 0.3).astype(np.float32)
    G = (-X + 0.1 * rng.standard_normal((37, 5))).astype(np.float32)
    h2 = R.median_h2(X)
    U = R.pairwise_u(X, G, h2, kernel)
    assert np.allclose(U, U.T, rtol=1e-12, atol=1e-12)
    assert abs(np.trace(U) - R.diag_sum(G, h2, kernel)) <= 1e-12 * np.trace(U)
    if kernel == "imq":
        ref = imq_ref.pairwise_u(torch.tensor(X), torch.tensor(G), h2).numpy()
        assert np.allclose(U, ref, rtol=1e-12, atol=1e-12)
    else:   # the identity the kernel evaluates: u = k (w_i.w_j - D / (2 h2^2) + b_i + b_j + d / h2)
        Xd, Gd = X.astype(np.float64), G.astype(np.float64)
        Wm = Gd - Xd / h2
        r = (Xd * Xd).sum(1)
        b = (Gd * Xd).sum(1) / h2 - r / (2.0 * h2 ** 2)
        D = r[:, None] + r[None, :] - 2.0 * Xd @ Xd.T
        alt = np.exp(-D / (2.0 * h2)) * (Wm @ Wm.T - D / (2.0 * h2 ** 2) + b[:, None] + b[None, :] + 5 / h2)
        assert np.allclose(U, alt, rtol=1e-10, atol=1e-10)
    W = R.sign_rows(6, 37, 1)
    W[0] = 1.0
    f = R.quadratic_forms(X, G, h2, kernel, W)
    assert abs(f.q[0] - U.sum()) <= 1e-12 * np.abs(U).sum()
    assert np.all(f.allow > 0) and np.all(f.allow < 1e-3 * f.scale) and np.all(f.scale >= np.abs(f.q))
    assert np.all(np.abs(U) <= R.element_model(X, G, h2, kernel)[1] * (1 + 1e-12))
    assert np.all(np.abs(U) <= R.device_bound(X, G, h2, kernel))       # the scale's bound is a bound


def test_sign_rows_follow_flip_prob():
    W = R.sign_rows(64, 4000, 5, 0.5)
    assert set(np.unique(W)) == {-1.0, 1.0} and abs(W[:, 0].mean()) < 0.5
    assert abs((W[:, 1:] != W[:, :-1]).mean() - 0.5) < 0.01
    W = R.sign_rows(64, 4000, 5, 0.1)
    assert abs((W[:, 1:] != W[:, :-1]).mean() - 0.1) < 0.01
