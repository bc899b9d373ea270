"""CPU: the Stein thinning case table (tests/thin_cases.py) does what it claims -- in every case at least 3/4 of the steps
are decisive under the allowance of tests/thin_ref.py, and between them the cases reach every arm of k_thin_step, repeats
and the lowest-index tie rule -- and the reference itself is sound."""
import numpy as np
import pytest

import imq_ref
import thin_cases as C
import thin_ref as R

ALL = [(c.name, k) for c in C.CASES for k in R.KERNELS]


@pytest.mark.parametrize("name,kernel", ALL)
def test_at_least_three_quarters_of_the_steps_are_decisive(name, kernel):
    X, G, h2, picks, forced = C.reference(name, kernel)
    share = float(forced.decisive.mean())
    print("%s %s: decisive share %.3f" % (name, kernel, share))
    assert share >= C.DECISIVE_SHARE
    # the fp64 loop passes its own teacher-forced check with nothing to spare
    assert (forced.gap == 0).all() and (forced.argmin == picks).all()
    assert (forced.allow[1:] > 0).all() and (np.diff(forced.allow) >= 0).all()


def test_the_cases_reach_every_arm_of_the_kernel():
    arms = {C.arm(c.d) for c in C.CASES}
    for vec in (False, True):
        assert {lg for v, lg, _ in arms if v == vec} == {1, 2, 4, 8, 16, 32, 64}, vec
        assert {min(ch, 2) for v, _, ch in arms if v == vec} == {1, 2}, vec       # one chunk, and more than one
    assert any(ch > 2 for _, _, ch in arms)
    assert {c.d % 4 for c in C.CASES} == {0, 1, 2, 3}
    # a chunk that is not full, in either unit
    assert any(c.d > C.CHUNK and c.d % C.CHUNK for c in C.CASES if c.d % 4 == 0)
    assert any(c.d > C.CHUNK and c.d % C.CHUNK for c in C.CASES if c.d % 4)
    # more than one workgroup by the default rule; fewer rows than one workgroup takes; n = 1
    assert any(c.n > 4 * C.rows_per_workgroup(c.d) for c in C.CASES)
    assert any(c.n < C.rows_per_workgroup(c.d) for c in C.CASES)
    assert any(c.n == 1 for c in C.CASES)
    for c in C.CASES:       # the forced grids: one workgroup that strides over all rows ... more workgroups than rows fill
        g = C.grids(c.n + len(c.dup), c.d)
        assert g[:3] == (1, 2, 3) and g[3] % 2 == 1 and g[3] > (c.n + len(c.dup)) / C.rows_per_workgroup(c.d)


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_the_cases_reach_repeats_and_the_tie_rule(kernel):
    c = C.BY_NAME["20x3_m40"]
    picks = C.reference(c.name, kernel)[3]
    assert c.m > c.n and 26 <= c.m - len(set(picks.tolist())) <= 29
    assert (C.reference("1x3_m5", kernel)[3] == 0).all()
    # duplicates: a copy never wins over its original, and the originals are picked -- on steps that are exact ties
    c = next(c for c in C.CASES if c.dup)
    X, G, h2, picks, forced = C.reference(c.name, kernel)
    assert all(np.array_equal(X[c.n + i], X[r]) for i, r in enumerate(c.dup))
    assert picks.max() < c.n
    tied = np.isin(picks, c.dup)
    assert tied.sum() >= 3 and not forced.decisive[tied].any()
    for t in np.flatnonzero(tied):      # (the tie is exact in fp64 as well: the copy's objective equals the original's)
        u = R.teacher_forced(X, G, h2, kernel, np.concatenate([picks[:t], [c.n + c.dup.index(int(picks[t]))]]))
        assert u.gap[t] == 0.0


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_reference_matches_the_pairwise_stein_kernel(kernel):
    """thin_ref.stein_row against the n x n matrix (IMQ: imq_ref.pairwise_u, the header's formula), and the running
    statistic against the V-statistic of the picked set, duplicates included"""
    X, G, h2, picks, forced = C.reference("20x3_m40", kernel)
    X64, G64 = X.astype(np.float64), G.astype(np.float64)
    n, d = X.shape
    if kernel == "imq":
        U = imq_ref.pairwise_u(X64, G64, h2).numpy()
    else:
        diff = X64[:, None, :] - X64[None, :, :]
        D = (diff ** 2).sum(-1)
        cross = ((G64[:, None, :] - G64[None, :, :]) * diff).sum(-1)
        U = np.exp(-D / (2 * h2)) * (G64 @ G64.T + cross / h2 + d / h2 - D / h2 ** 2)
    for s in (0, 7, n - 1):
        u, M, allow = R.stein_row(X, G, s, h2, kernel)
        np.testing.assert_allclose(u, U[s], rtol=1e-12, atol=1e-12 * M.max())
        assert (M >= np.abs(u) * (1 - 1e-12)).all() and (allow > 0).all() and (allow < 1e-3 * M).all()
    np.testing.assert_allclose(2 * R.diag_half(G, h2, kernel), np.diag(U), rtol=1e-12)
    for t in (1, 2, 17, 40):
        sub = U[np.ix_(picks[:t], picks[:t])]
        assert abs(forced.ksd2[t - 1] - sub.sum() / t ** 2) <= 1e-11 * np.abs(sub).sum() / t ** 2
        assert forced.scale[t - 1] >= np.abs(sub).sum() * (1 - 1e-12)


def test_teacher_forcing_catches_a_wrong_pick():
    X, G, h2, picks, forced = C.reference("130x2_m40", "imq")
    t = int(np.flatnonzero(forced.decisive)[5])
    bad = picks.copy()
    bad[t] = (picks[t] + 1) % X.shape[0]
    r = R.teacher_forced(X, G, h2, "imq", bad)
    assert r.gap[t] > r.allow[t] and r.argmin[t] == picks[t] and (r.gap[:t] == 0).all()
    # a dense 1-d cloud is mostly near-ties: no case
    dense = C.Case(700, 1, 40)
    Xd, Gd, hd = dense.inputs()
    p, _ = R.greedy(Xd, Gd, hd, "imq", dense.m)
    assert R.teacher_forced(Xd, Gd, hd, "imq", p).decisive.mean() < C.DECISIVE_SHARE
