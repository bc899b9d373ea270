"""CPU: what the tables of tests/class_weighted_cases.py reach in the WEIGHTED kernels of csrc/stein_predict_softmax.hip and
csrc/stein_predict_bnn_class.hip, and that a correct fp32 evaluation in the kernels' summation order stays inside the
allowance of tests/class_weighted_ref.py on these very inputs, before a GPU sees either."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_weighted_cases as cwc  # noqa: E402
import class_weighted_ref as cwr  # noqa: E402
import netclass_cases as ncc  # noqa: E402
import softmax_cases as smc  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stein_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# the tables mirror the weighted kernels: without them in the sources nothing below says anything
SRC_WB = {"softmax": int(re.search(r"constexpr int PS_WB = (\d+);", _source("stein_predict_softmax.hip")).group(1)),
          "netclass": int(re.search(r"constexpr int PC_WB = (\d+);", _source("stein_predict_bnn_class.hip")).group(1))}


def test_the_constants_are_the_sources():
    sm, nc = _source("stein_predict_softmax.hip"), _source("stein_predict_bnn_class.hip")
    assert SRC_WB == {"softmax": cwc.PS_WB, "netclass": cwc.PC_WB}
    assert int(re.search(r"constexpr int PW_HEAD = (\d+);", _source("stein_predict_fwd.h")).group(1)) == cwc.PW_HEAD
    # the weighted kernels are instantiations of the unweighted ones' templates, and the weight pass is shared, not copied
    for src, kernel in ((sm, "k_predict_softmax"), (nc, "k_predict_bnn_class")):
        assert re.search(r"template <int CP, bool WEIGHTED>\s*__global__ __launch_bounds__\(256\) void %s\(" % kernel, src)
        assert "predict_weight_pass(pl, n, pw, workspace, s)" in src and "k_predict_wsum" not in src
    # a block of staged lane weights holds whole passes, and more particles than a network unit spans
    assert all(cwc.PS_WB % pp == 0 for pp in (1, 2, 4)) and cwc.PC_WB > 16 + 1


def test_every_pattern_and_every_padded_class_end_of_both_kernels():
    for m, mod in (("softmax", smc), ("netclass", ncc)):
        pairs = cwc.CROSSED[m]
        assert {pat for _, pat in pairs} == set(cwc.PATTERNS)
        assert {case["C"] for case, _ in pairs} >= set(mod.CLASS_COUNTS)
        assert {cwc.plan(m, case)["cp"] for case, _ in pairs} == {4, 8, 16, 32}
        # the particle-count tables: n in {1, 15, 16, 17, 40} under every pattern that applies; zero_slices on the 40s
        for case in mod.PRED_COUNTS:
            pats = {pat for c, pat in pairs if c is case}
            assert pats == {p for p in cwc.PATTERNS if cwc.applies(case, p)}
            assert ("zero_slices" in pats) == (case["n"] == mod.THREE_SLICES)
        counts_c = {case["C"] for case in mod.PRED_COUNTS}
        assert counts_c == ({3, 8, 16, 32} if m == "softmax" else {3, 32})
        assert {case["n"] for case in mod.PRED_COUNTS} == {1, 15, 16, 17, 40}


def test_ragged_last_units_and_dead_units_at_every_place():
    for m in cwc.MODELS:
        places = {}
        ragged = cut = late_start = False
        for case, pat in cwc.CROSSED[m]:
            pl, w = cwc.plan(m, case), cwc.weights(case, pat)
            for place in cwc.dead_places(m, case, w):
                places.setdefault(place, set()).add(pl["nt"] > 1)
            last = (min(case["n"], pl["per"]) * pl["nt"]) % pl["unit"]
            ragged = ragged or last != 0
            cut = cut or (pl["nt"] > 1 and pl["unit"] % pl["nt"] != 0 and bool(cwc.dead_places(m, case, w)))
            vh = cwr.lane_weights(w)
            for s in range(pl["slices"]):
                blk = vh[s * pl["per"]:(s + 1) * pl["per"]]
                late_start = late_start or (bool((blk > 0).any()) and not blk[0] > 0)
        assert set(places) == {"start", "inside", "end"}, (m, places)
        if m == "netclass":          # with more than one tile per particle, and with unit boundaries that cut a particle
            assert all(True in v for v in places.values()), places
            assert cut
        assert ragged and late_start, m


def test_zero_slices_kills_whole_slices_and_wide_flushes_leading_weights():
    for m in cwc.MODELS:
        seen = set()
        for case, pat in cwc.CROSSED[m]:
            if pat not in ("zero_slices", "wide") or case["n"] < 40:
                continue
            pl = cwc.plan(m, case)
            w = cwc.weights(case, pat)
            vh = cwr.lane_weights(w)
            dead = [not (vh[s * pl["per"]:(s + 1) * pl["per"]] > 0).any() for s in range(pl["slices"])]
            assert pl["slices"] == 3, (m, case["name"])
            if pat == "zero_slices":
                assert dead == [True, False, True]
            else:        # positive weights that the lanes hold as zero, and a first live particle inside its slice
                flushed = (w > 0) & ~(vh > 0)
                assert flushed[0] and flushed.sum() >= 2 and not dead[0], (m, case["name"])
            seen.add(pat)
        assert seen == {"zero_slices", "wide"}, m


@pytest.mark.parametrize("triple", cwc.ALL, ids=cwc.triple_id)
def test_fp32_emulation_in_kernel_order_is_inside_the_allowance(triple):
    m, case, pat = triple
    a, w = cwc.args(m, case), cwc.weights(case, pat)
    ref = cwc.reference(m, case, a, w)
    got = cwc.emulate_f32(m, case, a, w)
    for k in ("prob", "ent", "lpd"):
        val, allow = ref[k]
        assert np.isfinite(val).all() and (allow > 0).all() and np.isfinite(allow).all(), k
        err = np.abs(got[k].astype(np.float64) - val)
        assert (err <= allow).all(), "%s: ratio %.3g" % (k, float((err / allow).max()))
    # the tight allowance against fp64 statistics of the emulation's own probabilities
    own = cwr.summaries_of_probs(got["pred_mean"].astype(np.float64), a["labels"], w, cwc.plan(m, case)["per"])
    for k in ("prob", "lpd"):
        val, allow = own[k]
        assert (allow <= ref[k][1]).all(), k
        assert (np.abs(got[k].astype(np.float64) - val) <= allow).all(), k + " (own pred)"
    val, allow = ref["ess"]
    assert 1.0 - allow <= val <= case["n"] + allow


def test_one_hot_and_uniform_emulations_are_exact():
    """what the GPU tests assert bit for bit: a one-hot weight returns that particle's probabilities, and the lane weight of a
    constant weight at a power-of-two n is a power of two"""
    case = smc.PRED_COUNTS[4]
    a = cwc.args("softmax", case)
    for pat in ("one_hot_first", "one_hot_last", "one_hot_ragged"):
        w = cwc.weights(case, pat)
        got = cwc.emulate_f32("softmax", case, a, w)
        assert np.array_equal(got["prob"], got["pred_mean"][int(np.argmax(w))])
        assert cwr.ess(w)[0] == 1.0
    for n in (16, 32):
        for c in (1.0, 3.7):
            assert np.array_equal(cwr.lane_weights(np.full(n, c)), np.full(n, 1.0 / n, np.float32))
