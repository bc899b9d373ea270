"""CPU: what the case table of the Stein importance weights' tests claims (tests/weights_cases.py), proved on the fp64
reference alone (tests/weights_ref.py): the cases reach every arm of k_weights_step, every kind of step length, and at least
DECISIVE_SHARE of every case's steps are decisive under the derived allowance."""
import numpy as np
import pytest

import weights_cases as C
import weights_ref as R

STEPPING = [c for c in C.CASES if c.iters > 0]


def test_the_cases_reach_every_arm():
    assert {c.kernel for c in C.CASES} == set(R.KERNELS)
    arms = {C.arm(c.d) for c in C.CASES}
    assert {lg for vec, lg, _ in arms if vec} == {1, 2, 4, 8, 16, 32, 64}          # 16-byte units, every group width
    assert {lg for vec, lg, _ in arms if not vec} == {1, 2, 4, 8, 16, 32, 64}      # 4-byte units (d % 4 != 0)
    assert {(vec, ch) for vec, _, ch in arms} >= {(True, 2), (False, 2)}            # d past the LDS chunk of 512, both units
    assert any((c.d - 512) % 4 for c in C.CASES if c.d > 512)                       # ... and a ragged last chunk
    n_parts = [C.parts(c.n + len(c.dup), c.d) for c in C.CASES]
    assert min(n_parts) == 1 and max(n_parts) > 3                                   # one workgroup, and more than any forced grid below it
    for c in C.CASES:
        g = C.grids(c.n + len(c.dup), c.d)
        assert g[0] == 1 and g[-1] > C.parts(c.n + len(c.dup), c.d)                # fewer workgroups than virtual ones, and more
    assert any(c.iters == 0 for c in C.CASES) and min(c.n + len(c.dup) for c in C.CASES) == 2


def test_the_cases_reach_every_kind_of_step():
    gam = {c.name: C.reference(c.name).gamma for c in STEPPING}
    assert any((g == 1.0).any() for g in gam.values())                              # all the mass to one vertex
    assert any(((g > 0.0) & (g < 1.0)).any() for g in gam.values())                 # an interior line search
    for c in STEPPING:
        if c.kind == "near":                                                        # gamma = 1, then converged: 0 for good
            g = gam[c.name]
            assert g[0] == 1.0 and (g[1:] == 0.0).all() and len(set(C.reference(c.name).idx.tolist())) == 1, c.name
        else:
            assert ((gam[c.name] > 0.0) & (gam[c.name] < 1.0)).all(), c.name


def test_the_duplicate_is_picked_and_the_lower_index_wins():
    c = next(c for c in C.CASES if c.dup)
    r = C.reference(c.name)
    assert np.array_equal(r.X[c.n], r.X[C.DUP_ROW])
    assert (r.idx == C.DUP_ROW).sum() >= 1 and r.idx.max() < c.n                    # np.argmin: the lowest index; never the copy
    tie = r.idx == C.DUP_ROW
    assert not r.forced.decisive[tie].any()                                         # a tie is no decisive step


@pytest.mark.parametrize("name", [c.name for c in STEPPING])
def test_the_fp64_path_is_decisive_and_consistent(name):
    r = C.reference(name)
    f = r.forced
    print("weights %s: decisive %.3f of %d steps, f / f(uniform) %.4f, first step -%.1f %%" %
          (name, f.decisive.mean(), r.idx.size, r.f[-1] / r.f[0], 100.0 * (1.0 - r.f[1] / r.f[0])))
    assert f.decisive.mean() >= C.DECISIVE_SHARE
    assert (f.gap == 0.0).all() and np.array_equal(f.argmin, r.idx)                 # its own path: the argmin itself
    assert ((r.gamma >= f.g_lo) & (r.gamma <= f.g_hi)).all()                        # ... and its step inside its interval
    assert (np.diff(r.f) <= 1e-12 * r.f[0]).all()                                   # f never increases
    assert np.allclose(f.f, r.f, rtol=1e-9, atol=0) and abs(r.w.sum() - 1.0) < 1e-12 and (r.w >= 0).all()


@pytest.mark.parametrize("case", C.PATH_CASES, ids=lambda c: c.name)
def test_the_weights_lower_the_discrepancy_with_a_wide_margin(case):
    """the four specified shapes: 4 n steps lower f by more than 100 x the largest initial allowance, the first step alone and
    the case's own short path by more than 10 x: "f(w) < f(uniform)" is decided far above anything the arithmetic can move"""
    r = C.reference(case.name)
    w, idx, gam, fs = R.frank_wolfe(r.model, 4 * case.n)
    a0 = r.model.cast_allow(np.full(case.n, 1.0 / case.n))[1].max()
    print("weights %s: f(4 n steps) / f(uniform) %.4f, first step -%.1f %%, largest A_0 / f(uniform) %.2e" %
          (case.name, fs[-1] / fs[0], 100.0 * (1.0 - fs[1] / fs[0]), a0 / fs[0]))
    assert fs[0] - fs[-1] > 100.0 * a0 and fs[0] - fs[1] > 10.0 * a0
    assert fs[0] - r.f[-1] > 10.0 * a0                                              # ... and so does the case's own short path
