"""CPU: the case table of the placed-window tests proves itself (tests/window_cases.py; the GPU side is
tests/test_gpu_window_placed.py).

Every expectation of the GPU module is fixed here, before a kernel runs: which outcome a placement has, which form of
spec_select_body's first pass a hit takes, that no case which is not meant to overflow can overflow a queue -- per-tile
and panel geometry, from the int64 D -- and that the model agrees with the independent NumPy implementation of the staged
protocol (oracle/staged_model.py) and with an exact sort."""
import numpy as np
import pytest
import torch

import select_inputs as si
import window_cases as wc
from oracle import staged_model as sm
from stein_amd import _lib

TABLES = {form: wc.case_table(form) for form in ("sym", "rows")}
ALL = TABLES["sym"] + TABLES["rows"]


def test_constants_come_from_the_sources_and_match_the_binding():
    c = wc.constants()
    assert c["SPEC_CAP"] == si.SPEC_CAP                                  # the lattice module's copy
    assert c["SPEC_TABLE"] == _lib.SPEC_TABLE_WORDS
    assert c["SPEC_SLOTS"] * 8 + c["SPEC_CAP"] == _lib.SPEC_TABLE_OFFSET_WORDS
    assert c["SPEC_TABLE_HDR"] == sm.NumpyStages.TABLE_HDR and c["SPEC_HW_MAX"] == sm.NumpyStages.HW_MAX
    assert 0 < c["DP_STRIP_SAFE"] <= c["DP_QCAP"] < c["SPEC_QCAP"] < c["INREG"] < c["SPEC_CAP"]


def test_scatter_384_seed_is_the_first_with_two_targets():
    for seed in range(wc.SCATTER_384_SEED + 1):
        ref = si.LatticeRef(si.scatter(384, seed))
        assert (ref.lo != ref.hi) == (seed == wc.SCATTER_384_SEED), seed


def test_sizes_and_families_are_the_lattice_module_s():
    assert {n for _, n in wc.FAMILIES} == {384, 768, 1536} <= set(si.PANEL_N)
    assert {f for f, _ in wc.FAMILIES} == {"grid", "scatter", "line", "simplex4_64_1"}
    assert "simplex4_64_1" in si.SIMPLEX
    row0, nl = wc.ROW_BLOCK
    assert row0 % 128 and (row0 + nl) <= 384 and nl % 128 and nl > 128     # off the origin, ragged, more than one row tile


def test_every_outcome_and_every_path_is_in_the_table():
    got = {c.step().outcome for c in TABLES["sym"]}
    assert got == set(wc.OUTCOMES), sorted(set(wc.OUTCOMES) - got)
    hits = {(c.step().path, c.step().two_hb) for c in TABLES["sym"] if c.step().outcome == "hit"}
    for want in (("register", False), ("register", True), ("ballot", False), ("ballot", True)):
        assert want in hits, (want, sorted(hits))
    assert any(p == "loop" for p, _ in hits), sorted(hits)
    # the fused call at n = 384, small=False, reaches solo_select behind every early exit of spec_select_body
    solo = {c.step().outcome for c in TABLES["sym"] if c.n == 384 and c.reps == 1}
    assert solo >= {"no_window", "overflow", "empty", "lo_below", "lo_above", "hi_above", "hit"}, sorted(solo)
    # and the row block, whose tally / pick have no such exit order, sees every outcome but the one that needs repetitions
    assert {c.step().outcome for c in TABLES["rows"]} >= set(wc.OUTCOMES) - {"over_capacity", "hi_above"}


def test_the_six_edge_placements_exist_and_sit_where_they_say():
    for form in ("sym", "rows"):
        for family, n in wc.FAMILIES:
            cases = {c.name: c for c in TABLES[form] if (c.family, c.n) == (family, n)}
            ent = wc.entries_of(family, n, form)
            kl, kh = ent.key_lo, ent.key_hi
            if family not in ("grid", "scatter"):
                assert not any(c.edge for c in cases.values())
                continue
            assert {"lo_first", "hi_last"} <= set(cases), (form, family, n)
            at = {name: (wc.grant(c.center, c.halfwidth)) for name, c in cases.items() if c.edge}
            assert at["lo_first"][0] == kl
            assert sum(at["hi_last"]) == kh
            if "lo_below" in at:
                assert at["lo_below"][0] == kl + 1
            if "lo_above" in at:
                assert sum(at["lo_above"]) == kl - 1
            if kl != kh:
                assert sum(at["hi_above"]) == kh - 1 and at["hi_above"][0] <= kl
                assert sum(at["lo_last"]) == kl
    edges = {c.name for c in TABLES["sym"] if c.edge}
    assert edges == set(wc.EDGES), edges
    # every edge placement at every size of the fused tests, on a family with two targets
    for n in (384, 768, 1536):
        assert {c.name for c in TABLES["sym"] if c.edge and c.n == n and c.family == "scatter"} == set(wc.EDGES), n


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_outcome_is_the_one_the_placement_was_built_for(case):
    s = case.step()
    assert case.expect is not None and s.outcome == case.expect, (case.id, s.outcome, case.expect)
    assert s.width == (0 if s.outcome == "no_window" else 2 * case.halfwidth)
    if case.total is not None:
        assert s.r0 == s.below and s.outcome == "hit"             # the case of its name: lo is the first buffered entry
    if s.outcome == "hit":
        # lo / hi of a hit are the exact order statistics of the whole multiset
        lo, hi, _ = case.targets()
        assert (float(s.lo), float(s.hi)) == (float(lo), float(hi)), case.id
        if case.total is None:
            assert (float(lo), float(hi)) == tuple(float(x) for x in si.exact_median(case.entries.values, case.entries.w)[:2])
        ref = si.lattice_ref(case.family, case.n) if (case.form == "sym" and case.total is None and
                                                      (case.family, case.n) != ("scatter", 384)) else None
        if ref is not None:
            assert (float(s.lo), float(s.hi)) == (float(ref.lo), float(ref.hi))


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_no_queue_overflows_unless_the_case_is_an_overflow(case):
    c = wc.constants()
    s = case.step("tiles")
    if case.expect == "overflow":
        assert s.max_queue > c["SPEC_QCAP"]
    else:
        assert s.max_queue <= c["SPEC_QCAP"] and not s.overflow, (case.id, s.max_queue)
    if case.form == "sym" and case.panel_ok:                      # the cases the GPU module runs on the panel kernel
        p = case.step("panel")
        if case.expect == "overflow":
            assert p.max_queue > c["DP_QCAP"]                     # overflows whichever wave draws the strip
        else:
            assert p.max_queue <= c["DP_STRIP_SAFE"] and not p.overflow, (case.id, p.max_queue)
            assert p.outcome == s.outcome and p.count == s.count and np.array_equal(p.table, s.table)


def test_the_panel_kernel_sees_every_outcome_too():
    got = {c.step("panel").outcome for c in TABLES["sym"] if c.panel_ok}
    assert got == set(wc.OUTCOMES), sorted(set(wc.OUTCOMES) - got)
    assert {c.name for c in TABLES["sym"] if c.panel_ok and c.edge and c.family == "scatter" and c.n == 768} == set(wc.EDGES)


# ---- against oracle/staged_model.py, an independent implementation of the staged protocol -----------------------------
_SPEC = torch.zeros(8 * (sm.NumpyStages.TABLE_OFF + sm.NumpyStages.TABLE_HDR + 2 * sm.NumpyStages.HW_MAX + 2), dtype=torch.uint8)


def _oracle_step(case):
    """spec_begin -> distance_block_spec -> spec_tally -> spec_pick of the NumPy stages on the case's block (weight 1 per
    entry: the full matrix holds the symmetric multiset)"""
    n = case.n
    P = wc.lattice_points(case.family, n)
    T = torch.tensor(P, dtype=torch.float32)
    row0, nl = (0, n) if case.form == "sym" else wc.ROW_BLOCK
    st = sm.NumpyStages(None)
    st._sp = dict(magic=2, center=case.center, halfwidth=case.halfwidth, last_key=0)
    hist = torch.zeros(3, 2, sm.BINS, dtype=torch.int64)
    sel = torch.zeros(192, dtype=torch.uint8)
    r, D = torch.zeros(n), torch.zeros(nl, n)
    h2, med = torch.full((1,), float("nan")), torch.full((1,), float("nan"))
    st.rownorms(T, n, P.shape[1], r)
    st.spec_begin(hist, sel, _SPEC, nl * n if case.total is None else case.total)
    st.distance_block_spec(T, r, n, P.shape[1], row0, nl, D, n, hist[0], sel, _SPEC)
    st.spec_tally(sel, _SPEC)
    table = st._table(_SPEC).copy()
    st.spec_pick(sel, _SPEC, n, h2, med)
    return st, table, h2, med


EXPRESSIBLE = [c for c in ALL if c.reps == 1 and c.expect not in ("overflow", "over_capacity")]


@pytest.mark.parametrize("case", EXPRESSIBLE, ids=lambda c: c.id)
def test_model_agrees_with_the_staged_numpy_model(case):
    """That file knows no queue and no buffer capacity, and counts every entry of the full block once: it can express
    every single-submission case that neither overflows nor exceeds the buffer, and its entry count ([2]) is the full
    block's, not the upper triangle's."""
    hdr = wc.constants()["SPEC_TABLE_HDR"]
    s = case.step()
    st, table, h2, med = _oracle_step(case)
    assert (st._sp["lo"] if s.granted else wc.NO_WINDOW_KEY, st._sp["width"]) == (s.lo_key if s.granted else wc.NO_WINDOW_KEY, s.width)
    assert int(table[0]) == s.below and int(table[1]) == int(s.table[1])
    assert np.array_equal(table[hdr:hdr + s.width + 1], s.table[hdr:])
    assert not table[hdr + s.width + 1:].any()
    if case.form == "rows":
        assert int(table[2]) == s.count
    assert bool(st._sp["hit"]) == (s.outcome == "hit"), (case.id, s.outcome)
    if s.outcome == "hit":
        assert (float(st._st.lo), float(st._st.hi)) == (float(s.lo), float(s.hi))
        want_med = np.float32(0.5) * (s.lo + s.hi) if s.r0 != s.r1 else s.lo
        assert float(med) == float(want_med) == float(case.targets()[2])
        assert float(h2) == float(si.bandwidth(want_med, case.n))


def test_predictor_replay_agrees_with_the_staged_numpy_model():
    """wc.predictor_update against NumpyStages.spec_update over the table's hits and misses, the halving included"""
    m1, m2 = wc._magic()
    cap = wc.constants()["SPEC_CAP"]
    checked = 0
    for case in [c for c in EXPRESSIBLE if c.form == "rows"][::3]:
        s = case.step()
        st, _, _, _ = _oracle_step(case)
        if s.outcome != "hit":
            st._st.lo = case.entries.lo                          # (the radix passes' answer)
        for count, earned, last in ((s.count, 0, 0x80000001), (cap // 2 + 1, 1000, case.entries.key_lo - 77), (cap // 2, 9, 0xC0000000)):
            before = dict(magic=m2, center=case.center, halfwidth=case.halfwidth, earned_hw=earned, last_key=last, n_steps=5, n_hits=2)
            sp = dict(st._sp, magic=2, earned_hw=earned, last_key=last, count=count)
            st2 = sm.NumpyStages(None)
            st2._sp, st2._st = sp, st._st
            st2.spec_update(None)
            after = wc.predictor_update(before, case.entries.key_lo, s.width, s.outcome == "hit", count)
            assert (after["center"], after["halfwidth"], after["earned_hw"], after["last_key"]) == \
                   (sp["center"], sp["halfwidth"], sp["earned_hw"], sp["last_key"]), (case.id, count)
            assert after["n_steps"] == 6 and after["n_hits"] == 2 + (s.outcome == "hit") and after["magic"] == m2
            checked += 1
    assert checked >= 30
