"""CPU: the fp64 references of the weighted predictive summaries and their fp32 allowance (tests/predict_weighted_ref.py) and
the case tables of tests/test_gpu_predict_weighted_matrix.py (tests/predict_weighted_cases.py).

(a) the tables reach every (arm x weighted) path of csrc/stein_predict.hip, and the zero-slice and first-live-particle
    branches, asserted from predict_cases.plan;
(b) a NumPy float32 evaluation in the kernel's order stays inside the allowance on every case small enough for the CPU;
(c) a naive fp32 sum w f^2 - (sum w f)^2 and an un-shifted weighted log sum exp LEAVE the allowance on var_offset and
    lpd_range, and on var_offset the variance allowance is below half the variance;
(d) the reference agrees with np.average and a direct fp64 evaluation, and integer counts agree with the unweighted
    reference on the repeated sample."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_ref as pr  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import predict_weighted_ref as pwr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_PAIRS = [p for p in pwc.CROSSED + [pwc.SUBSET] if pc.cpu_sized(p[0])]
SUMMARIES = ("mean", "var", "lpd")


def _source():
    """the summary kernels' source and, ahead of it, the header it shares with the rank-counting kernels"""
    csrc = os.path.join(ROOT, "stein_amd", "csrc")
    return open(os.path.join(csrc, "stein_predict_fwd.h")).read() + open(os.path.join(csrc, "stein_predict.hip")).read()


# ---- (a) ------------------------------------------------------------------------------------------
def test_the_source_has_the_weighted_paths_the_tables_assume():
    src = _source()
    assert src.count("constexpr int PW_HEAD = ") == 1 and "constexpr int PW_HEAD = %d;" % pwc.PW_HEAD in src
    assert src.count("PW_HEAD + 3 * slices") == 1
    assert "template <bool WEIGHTED>" in src and "template <int NIN, bool WEIGHTED>" in src
    assert "PR_LAUNCH_BNN_AS(NIN, true)" in src and "PR_LAUNCH_GLM(true," in src and "k_predict_finish<true>" in src
    assert re.search(r"q >= FLT_MIN \? q : 0\.f", src)     # the flush the reference charges


def test_tables_reach_every_arm_weighted_and_every_pattern():
    seen = {pwc.pair_id(p) for p in pwc.CROSSED}
    assert len(seen) == len(pwc.CROSSED)
    by_case = {}
    for case, pat in pwc.CROSSED:
        by_case.setdefault(case["name"], set()).add(pat)
    assert set(by_case) == {c["name"] for c in pc.CASES}                 # at least one pattern per case
    for case in pc.COUNTS + pc.COND:                                     # every pattern that exists for the case
        assert by_case[case["name"]] == {p for p in pwc.PATTERNS if pwc.applies(case, p)}, case["name"]
    arms = [c for c, _ in pwc.CROSSED if c in pc.ARMS]
    assert {c["n_in"] for c in arms if c["model"] == "bnn"} == {1, 2, 3, 4}          # the four weighted network kernels
    assert {pc.glm_arm(c["F"]) for c in arms if c["model"] != "bnn"} == {"whole", "chunked"}
    assert {pat for c, pat in pwc.CROSSED if c in pc.ARMS + pc.ROWS} >= set(pwc.PATTERNS) - {"zero_slices"}
    # the cases every pattern must reach: past the slice cap, 223 slices over several row tiles, both conditioning flavors
    for name in ("n17403_logistic", "n17403_bnn", "want228", "var_offset", "var_offset_bnn", "lpd_range"):
        assert by_case[name] == set(pwc.PATTERNS), name
    # where zero_slices does not exist there is no slice strictly inside, or no second particle in one
    for case in pc.CASES:
        _, slices, per = pc.plan(case["n"], case["B"])
        assert pwc.applies(case, "zero_slices") == (slices >= 3 and per >= 2)


def test_zero_slices_reach_the_skip_and_first_live_particle_branches():
    G = 16                                                 # PF_GROUPS
    assert _source().count("PF_ROWS = 16, PF_GROUPS = 16") == 1
    whole_group_dead = dead_inside_group = False
    for case, pat in pwc.CROSSED:
        if pat != "zero_slices":
            continue
        n = case["n"]
        _, slices, per = pc.plan(n, case["B"])
        w = pwc.weights(case, pat)
        sums = [w[s * per:(s + 1) * per].sum() for s in range(slices)]
        dead = [s for s in range(slices) if sums[s] == 0]
        assert dead == pwc.dead_slices(case) and 0 in dead and slices - 1 in dead and len(dead) < slices
        for s in range(slices):                            # a live slice's first particle is dead, a later one sets the state
            if s not in dead:
                assert w[s * per] == 0 and (w[s * per + 1:(s + 1) * per] > 0).any()
        per_g = -(-slices // G)
        groups = [list(range(g * per_g, min(slices, (g + 1) * per_g))) for g in range(G)]
        for g in groups:
            if g and all(s in dead for s in g):
                whole_group_dead = True                    # the group merge meets an empty group, group 0 among them
            if len(g) > 1 and any(s in dead for s in g) and any(s not in dead for s in g):
                dead_inside_group = True
        if slices <= G:                                    # one slice per group: group 0 is empty
            assert all(s in dead for s in groups[0])
    assert whole_group_dead and dead_inside_group


def test_wide_weights_flush_leading_slices_and_start_inside_one():
    case = next(c for c in pc.COUNTS if c["name"] == "n17403_logistic")
    _, slices, per = pc.plan(case["n"], case["B"])
    vh = pwr.lane_weights(pwc.weights(case, "wide"))
    assert (vh[:per] == 0).all() and (vh[-per:] > 0).all()                  # whole slices under the flush, at the front
    first = int(np.argmax(vh > 0))
    assert first % per != 0                                                  # the first live particle lies inside its slice
    w = pwc.weights(case, "wide")
    assert w[first - 1] > 0 and w.min() == 2.0 ** -150 and w.max() == 1.0


def test_one_hot_positions_and_lpd_range_weights():
    for case in pc.COUNTS + pc.COND:
        n = case["n"]
        _, slices, per = pc.plan(n, case["B"])
        p = pwc.ragged_index(case)
        L = n - (slices - 1) * per
        assert (slices - 1) * per + (L - 1) // pc.PR_PASS * pc.PR_PASS <= p < n
        for pat, q in (("one_hot_first", 0), ("one_hot_last", n - 1), ("one_hot_ragged", p)):
            w = pwc.weights(case, pat)
            assert w.sum() == 1.0 and w[q] == 1.0
    assert any((case["n"] - (pc.plan(case["n"], case["B"])[1] - 1) * pc.plan(case["n"], case["B"])[2]) % pc.PR_PASS
               for case in pc.COUNTS)                                        # ragged last passes exist
    case = next(c for c in pc.COND if c["name"] == "lpd_range")
    a = pc.args(case)
    w = pwc.weights(case, "positive", a)
    l = np.asarray(pc.reference(case, a)["l"])
    assert int(np.argmax(w)) == int(np.argmin(l[:, 0])) and w.max() > 40 * np.sort(w)[-2]


# ---- (b) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", CPU_PAIRS, ids=pwc.pair_id)
def test_fp32_evaluation_stays_inside_the_allowance(pair):
    case, pat = pair
    a = pc.args(case)
    w = pwc.weights(case, pat, a)
    ref = pwc.reference(case, a, w)
    got = pwc.emulate_f32(case, a, w)
    for k in SUMMARIES:
        val, allow = ref[k]
        assert np.isfinite(val).all() and np.isfinite(allow).all() and (allow >= 0).all(), k
        assert np.isfinite(got[k]).all(), k
        err = np.abs(got[k].astype(np.float64) - val)
        pos = allow > 0
        print("%-28s %-4s fp32 emulation max |err| / allowance = %.3f" % (pwc.pair_id(pair), k, (err[pos] / allow[pos]).max() if pos.any() else 0.0))
        assert (err <= allow).all(), (k, (err[pos] / allow[pos]).max())
    if pat.startswith("one_hot"):
        p = int(np.argmax(w))
        assert (got["mean"] == got["pred"][p]).all() and (got["var"] == 0).all() and (got["lpd"] == got["l"][p]).all()
        assert pwr.ess(w)[0] == 1.0


# ---- (c) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["var_offset", "var_offset_bnn"])
@pytest.mark.parametrize("pat", ["positive", "counts", "uniform"])
def test_a_raw_moment_weighted_variance_leaves_the_allowance(name, pat):
    case = next(c for c in pc.COND if c["name"] == name)
    a = pc.args(case)
    w = pwc.weights(case, pat, a)
    ref = pwc.reference(case, a, w)
    f = pc.emulate_f32(case, a)["pred"]
    vh = pwr.lane_weights(w)[:, None]
    naive = (vh * f * f).sum(0, dtype=np.float32) - (vh * f).sum(0, dtype=np.float32) ** 2
    assert naive.dtype == np.float32
    err = np.abs(naive.astype(np.float64) - ref["var"][0])
    assert (err > ref["var"][1]).all() and np.median(err) > 100.0 * np.median(ref["var"][1])   # every row leaves it, most by far
    assert (ref["var"][1] < 0.5 * ref["var"][0]).all()     # while the allowance resolves the variance itself


@pytest.mark.parametrize("pat", ["positive", "counts", "wide", "uniform"])
def test_an_unshifted_weighted_log_sum_exp_leaves_the_allowance(pat):
    case = next(c for c in pc.COND if c["name"] == "lpd_range")
    a = pc.args(case)
    w = pwc.weights(case, pat, a)
    ref = pwc.reference(case, a, w)
    l = pc.emulate_f32(case, a)["l"]
    with np.errstate(divide="ignore", under="ignore"):
        naive = np.log((pwr.lane_weights(w)[:, None] * np.exp(l)).sum(0, dtype=np.float32))
    assert not np.isfinite(naive).any()                    # every exp underflows: log 0
    assert (ref["lpd"][1] < 1e-2).all() and np.isfinite(ref["lpd"][0]).all()


# ---- (d) ------------------------------------------------------------------------------------------
def test_reference_statistics_are_numpys_own():
    rng = np.random.default_rng(3)
    f, l = rng.normal(size=(23, 5)), -3.0 * rng.uniform(size=(23, 5))
    w = rng.exponential(size=23)
    w[[0, 7, 22]] = 0.0
    f[7], l[7] = np.nan, np.inf                            # weight zero: enters nothing, whatever it holds
    mean, _, var, _ = pwr.mean_var(f, np.zeros_like(f), w, 7, 4)
    val, _ = pwr.lpd(l, np.zeros_like(l), w, 7, 4)
    keep = w > 0
    avg = np.average(f[keep], axis=0, weights=w[keep])
    assert np.allclose(mean, avg, rtol=1e-14)
    assert np.allclose(var, np.average((f[keep] - avg) ** 2, axis=0, weights=w[keep]), rtol=1e-13)
    assert np.allclose(val, np.log((w[keep, None] * np.exp(l[keep])).sum(0) / w.sum()), rtol=1e-13)
    assert np.isclose(pwr.ess(w)[0], w.sum() ** 2 / (w ** 2).sum(), rtol=1e-15)
    assert pwr.ess(np.full(9, 3.7))[0] == pytest.approx(9.0, rel=1e-15)


def test_integer_counts_are_the_unweighted_statistics_of_the_repeated_sample():
    rng = np.random.default_rng(4)
    f, l = rng.normal(size=(40, 3)), -3.0 * rng.uniform(size=(40, 3))
    counts = np.bincount(rng.integers(0, 40, size=25), minlength=40)
    assert (counts == 0).any() and (counts > 1).any()
    mean, _, var, _ = pwr.mean_var(f, np.zeros_like(f), counts.astype(np.float64), 7, 6)
    val, _ = pwr.lpd(l, np.zeros_like(l), counts.astype(np.float64), 7, 6)
    rep = np.repeat(np.arange(40), counts)
    m0, _, v0, _ = pr.mean_var(f[rep], np.zeros((25, 3)), 7, 4)
    l0, _ = pr.lpd(l[rep], np.zeros((25, 3)), 7, 4)
    assert np.allclose(mean, m0, rtol=1e-13) and np.allclose(var, v0, rtol=1e-12) and np.allclose(val, l0, rtol=1e-13)
    assert np.isclose(pwr.ess(counts.astype(np.float64))[0], 25.0 ** 2 / (counts ** 2).sum())


def test_the_emulation_ignores_what_zero_weight_particles_hold():
    case = next(c for c in pc.COUNTS if c["name"] == "n33_logistic")
    a = pc.args(case)
    w = pwc.weights(case, "counts")
    got = pwc.emulate_f32(case, a, w)
    _, _, per = pc.plan(case["n"], case["B"])
    f, l = got["pred"].copy(), got["l"].copy()
    f[w == 0], l[w == 0] = np.nan, np.inf
    again = pwr.summaries_f32(f, l, w, per)
    for k, v in zip(SUMMARIES, again):
        assert np.array_equal(got[k], v), k
