"""CPU: the fp64 references of the predictive producers and their fp32 allowance (tests/predict_ref.py) and the case tables
of tests/test_gpu_predict_matrix.py (tests/predict_cases.py).

(a) the tables reach every instantiation and dispatch arm of csrc/stein_predict.hip, and the constants they mirror are the
    source's;
(b) a NumPy float32 evaluation in the kernel's order stays inside the allowance on every case small enough for the CPU;
(c) on the two conditioning cases an fp32 E[f^2] - E[f]^2 and an un-shifted fp32 log sum exp LEAVE the allowance: the cases
    can catch what they are there for;
(d) the reference agrees with NumPy's own mean / var and a direct log-mean-exp, and with a per-particle forward pass of the network."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = [c for c in pc.CASES + [pc.SUBSET_CASE] if pc.cpu_sized(c)]
OUTPUTS = ("pred", "mean", "var", "lpd")


def _source():
    """the summary kernels' source and, ahead of it, the header it shares with the rank-counting kernels"""
    csrc = os.path.join(ROOT, "stein_amd", "csrc")
    return open(os.path.join(csrc, "stein_predict_fwd.h")).read() + open(os.path.join(csrc, "stein_predict.hip")).read()


# ---- (a) ------------------------------------------------------------------------------------------
def test_constants_mirror_the_source():
    src = _source()
    for name in ("PR_ROWS", "PR_PASS", "PR_SLICE_CAP", "PR_TARGET_WGS", "PR_FC", "PR_HC", "PR_STATE"):
        assert len(re.findall(r"constexpr int %s = " % name, src)) == 1, name          # defined once across the two files
        assert re.search(r"constexpr int %s = %d;" % (name, getattr(pc, name)), src), name
    for idiom in ("n_feats <= PR_FC ? n_feats : PR_FC", "const int ld = fc | 1;", "if (nfc == 1) stage_x(0, F);",
                  "if (nfc > 1) stage_x(f0, len);", "h0 += PR_HC", "len4 = (len + 3) & ~3", "PF_ROWS = 16, PF_GROUPS = 16"):
        assert src.count(idiom) == 1, idiom
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "__shfl" not in code   # no float atomics anywhere: no atomics at all


def test_tables_reach_every_instantiation_and_arm():
    src = _source()
    assert sorted(int(k) for k in re.findall(r" PR_LAUNCH_BNN\((\d)\);", src)) == [1, 2, 3, 4]
    arms = [c for c in pc.ARMS]
    glm = [c for c in arms if c["model"] != "bnn"]
    bnn = [c for c in arms if c["model"] == "bnn"]
    assert sorted({c["n_in"] for c in bnn}) == [1, 2, 3, 4]
    Fs, Hs = [c["F"] for c in glm], [c["H"] for c in bnn]
    for lo, hi in pc.GLM_EDGES:
        assert lo in Fs and hi in Fs
    assert pc.glm_arm(pc.GLM_EDGES[0][0]) == "whole" and pc.glm_arm(pc.GLM_EDGES[0][1]) == "chunked"
    assert [F for F in range(1, 1024) if pc.glm_arm(F) != pc.glm_arm(F + 1)] == [pc.PR_FC]
    for lo, hi in pc.BNN_EDGES:
        assert lo in Hs and hi in Hs
    assert {1, 1024} <= set(Fs) and {1, 1024} <= set(Hs)
    assert any(F % 2 for F in Fs if F <= pc.PR_FC) and any(F % 2 == 0 for F in Fs if F <= pc.PR_FC)   # both row paddings
    assert any(H % 4 for H in Hs)                                                                      # zero-filled hidden units
    assert {(c["model"], c["output"]) for c in glm} == {("linear", "link"), ("linear", "mean"), ("logistic", "link"), ("logistic", "mean")}
    assert {c["alpha"] for c in glm} == {None, "before", "after", "last"}
    assert any(c["tau"] != 1.0 for c in glm if c["model"] == "linear")


def test_tables_reach_the_particle_and_row_edges():
    P, R = pc.PR_PASS, pc.PR_ROWS
    for m in ("logistic", "bnn"):
        ns = sorted(c["n"] for c in pc.COUNTS if c["model"] == m)
        assert ns == [1, P - 1, P, P + 1, 2 * P + 1, 17403]
    rt, slices, per = pc.plan(17403, 5)
    assert pc.PR_SLICE_CAP * P < 17403 and slices == pc.PR_SLICE_CAP and P < per <= 2 * P    # at the cap, two passes a slice
    assert pc.plan(1, 5) == (1, 1, 1) and pc.plan(P, 5) == (1, 1, P) and pc.plan(P + 1, 5) == (1, 2, 9)
    rt, slices, per = pc.plan(4000, 2049)
    assert rt == 9 and -(-pc.PR_TARGET_WGS // rt) == 228 < min(pc.PR_SLICE_CAP, -(-4000 // P)) and slices <= 228 and per == 18
    for m in ("linear", "bnn"):
        assert sorted(c["B"] for c in pc.ROWS if c["model"] == m) == [1, R - 1, R, R + 1, 2 * R + 3]
    for c in pc.CASES:                                     # every plan covers its particles exactly once
        rt, slices, per = pc.plan(c["n"], c["B"])
        assert (slices - 1) * per < c["n"] <= slices * per and rt * R >= c["B"] > (rt - 1) * R
        assert slices * pc.PR_STATE * 4 * c["B"] <= pc.workspace_bytes(c["n"], c["B"])


# ---- (b) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c["name"])
def test_fp32_evaluation_stays_inside_the_allowance(case):
    a = pc.args(case)
    ref = pc.reference(case, a)
    got = pc.emulate_f32(case, a)
    for k in OUTPUTS:
        val, allow = ref[k]
        assert np.isfinite(val).all() and np.isfinite(allow).all() and (allow > 0).all(), k
        assert np.isfinite(got[k]).all(), k
        err = np.abs(got[k].astype(np.float64) - val)
        print("%-16s %-4s fp32 emulation max |err| / allowance = %.3f" % (case["name"], k, (err / allow).max()))
        assert (err <= allow).all(), (k, (err / allow).max())
    if case["flavor"] != "plain":
        pc.check_conditioning_inputs(case, a, ref)
    if case["flavor"] == "logit_sat":
        assert (got["pred"] >= 0).all() and (got["pred"] <= 1).all()
    if case["n"] == 1:
        assert (got["var"] == 0).all() and (ref["var"][0] == 0).all()


def test_summaries_of_given_outputs_carry_the_reduction_terms_only():
    """reference(z=...) takes the linear outputs as exact: the allowance of the mean shrinks to the reduction's own terms"""
    case = pc.ARMS[2]
    a = pc.args(case)
    got = pc.emulate_f32(case, a)
    z = got["pred"].astype(np.float64)                     # output "link": pred is z
    full, own = pc.reference(case, a), pc.reference(case, a, z=z)
    assert (own["pred"][1] == 0).all() and (own["mean"][1] < 0.2 * full["mean"][1]).all()
    for k in ("mean", "var", "lpd"):
        assert (np.abs(got[k].astype(np.float64) - own[k][0]) <= own[k][1]).all(), k


# ---- (c) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["var_offset", "var_offset_bnn"])
def test_a_raw_moment_variance_leaves_the_allowance(name):
    case = next(c for c in pc.COND if c["name"] == name)
    a = pc.args(case)
    ref = pc.reference(case, a)
    f = pc.emulate_f32(case, a)["pred"]
    naive = (f * f).mean(0, dtype=np.float32) - f.mean(0, dtype=np.float32) ** 2        # E[f^2] - E[f]^2 in fp32
    assert naive.dtype == np.float32
    assert (np.abs(naive.astype(np.float64) - ref["var"][0]) > 10.0 * ref["var"][1]).all()
    assert (ref["var"][1] < 0.5 * ref["var"][0]).all()     # while the allowance resolves the variance itself


def test_an_unshifted_log_sum_exp_leaves_the_allowance():
    case = next(c for c in pc.COND if c["name"] == "lpd_range")
    a = pc.args(case)
    ref = pc.reference(case, a)
    l = pc.emulate_f32(case, a)["l"]
    with np.errstate(divide="ignore", under="ignore"):
        naive = np.log(np.exp(l).sum(0, dtype=np.float32)) - np.float32(np.log(case["n"]))
    assert not np.isfinite(naive).any()                    # every exp underflows: log 0
    assert (ref["lpd"][1] < 1e-2).all() and np.isfinite(ref["lpd"][0]).all()


# ---- (d) ------------------------------------------------------------------------------------------
def test_reference_statistics_are_numpys_own():
    rng = np.random.default_rng(3)
    f, l = rng.normal(size=(23, 5)), -3.0 * rng.uniform(size=(23, 5))
    mean, _, var, _ = pr.mean_var(f, np.zeros_like(f), 7, 4)
    val, _ = pr.lpd(l, np.zeros_like(l), 7, 4)
    assert np.allclose(mean, f.mean(0), rtol=1e-14) and np.allclose(var, np.var(f, axis=0), rtol=1e-13)
    assert np.allclose(val, np.log(np.exp(l).mean(0)), rtol=1e-13)


def test_network_reference_matches_a_per_particle_forward_pass():
    case = pc.ARMS[11]
    assert case["model"] == "bnn"
    a = pc.args(case)
    z, _, _ = pr.bnn_link(a["theta"], case["n_in"], case["H"], a["cols"], a["X"])
    c = dict(zip(pr.sr.BNN_ORDER, a["cols"]))
    ref = np.zeros_like(z)
    for i in range(case["n"]):                             # the forward pass written out per particle
        t = a["theta"][i]
        w1 = t[c["w1"]:c["w1"] + case["n_in"] * case["H"]].reshape(case["n_in"], case["H"])
        hid = np.maximum(a["X"] @ w1 + t[c["b1"]:c["b1"] + case["H"]], 0.0)
        ref[i] = hid @ t[c["w2"]:c["w2"] + case["H"]] + t[c["b2"]]
    assert np.abs(z - ref).max() <= 1e-12 * np.abs(ref).max()
