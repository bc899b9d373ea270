"""CPU: the case table of the streaming steps (tests/stream_cases.py) reaches every class of their run-time dispatch in every
form it applies to, and the model the classes are read from agrees with the library's own host arithmetic: the plan
(stein_stream_plan / stein_imq_plan under stein_debug_stream_jsplit) and all four workspace sizes.  The model's ranges are
shown to tile the j tiles and its workgroup map to be a bijection: that checks the description; a bad map in a kernel shows
up on the GPU as an unwritten tile (test_gpu_stream_matrix.py).  Last, the fp64 reference alone is shown to satisfy what the
GPU test divides by: no all-zero 128 x 128 tile of phi or of any range's partial sums, no all-zero row tile of a range's row
sums -- with torch in fp64 on the CPU, the very function the GPU test evaluates on the device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402
from stein_amd import _lib  # noqa: E402

IDS = [sc.case_id(c) for c in sc.CASES]

# every class of the list ("Streaming steps, every path"), by the forms it can occur in
EVERY_FORM = ["cg1", "cg>1", "d-tail-in-block", "d-tail<16", "d-tail-in-second-16", "d-tail%32==0", "d<32", "ntk==1", "ntk>8",
              "d%4==0", "d%4!=0"] + ["n%%128==%d" % r for r in sc.N_RESIDUES] + \
             ["n<128", "n==1", "one-row-tile", "many-row-tiles",
              "jsplit1-by-rule", "jsplit1-by-hook", "equal-ranges", "ragged-last-range", "hook-clamped", "empty-tails-dropped",
              "range-of-one-tile", "range-odd", "range-even",
              "nblk<8", "nblk%8==0", "nblk%8in1..4", "nblk%8in5..7",
              "vec0-by-d", "vec0-by-misalign", "vec1",
              "sq_blocks==1", "1<sq_blocks<1024", "sq_blocks==1024", "finish-grid-stride", "finish-grid-stride-with-jsplit",
              "sq_blocks>256", "other-bandwidth"]
RBF_ONLY = ["dead-half", "both-halves"]
KSD_ONLY = ["ksd-score-aligned", "ksd-score-misaligned", "phi-null", "phi-null-with-jsplit"]
REQUIRED = [(form, name) for form in sc.FORMS for name in EVERY_FORM] + \
           [(form, name) for form in ("rbf", "rbf-ksd") for name in RBF_ONLY] + \
           [(form, name) for form in ("rbf-ksd", "imq-ksd") for name in KSD_ONLY]

_PLAN = {"rbf": _lib.stream_plan, "imq": _lib.imq_plan}
_BYTES = {("rbf", False): _lib.stream_workspace_bytes, ("rbf", True): _lib.stream_ksd_workspace_bytes,
          ("imq", False): _lib.imq_workspace_bytes, ("imq", True): _lib.imq_ksd_workspace_bytes}


def test_table_has_its_stated_size_and_shape():
    assert len(sc.CASES) == len(set(sc.CASES)) == len(set(IDS)) and 45 <= len(sc.CASES) <= 60
    for c in sc.CASES:
        assert c.kind in ("rbf", "imq") and c.n >= 1 and c.d >= 1 and c.hook >= 0 and set(c.misalign) <= set("tps")
        assert not c.phi_null or (c.ksd and "p" not in c.misalign)       # phi may be NULL in the KSD forms only
        assert "s" not in c.misalign or c.ksd                            # only the KSD finish reads the score
        assert c.mult in (0.25, 1.0, 4.0)
    big = sorted({(c.n, c.d) for c in sc.CASES if c.n > 2100})
    assert big == [(4224, 1025), (4224, 2001)]                           # the only shapes above a few thousand rows
    assert sum(c.mult != 1.0 for c in sc.CASES) == 4
    for c in sc.CASES:                                                   # ... each on a shape the table has at the heuristic's h2
        assert c.mult == 1.0 or any(o.mult == 1.0 and (o.kind, o.ksd, o.n, o.d) == (c.kind, c.ksd, c.n, c.d) for o in sc.CASES)


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_model_agrees_with_the_library(case):
    c, p = case, sc.plan_of(case)
    try:
        _lib.debug_stream_jsplit(c.hook)
        assert _PLAN[c.kind](c.n, c.d) == (p["row_tiles"], p["col_units"], p["jsplit"])
        for ksd in (False, True):
            assert _BYTES[c.kind, ksd](c.n, c.d) == sc.sections(c.kind, c.n, c.d, p["jsplit"], ksd)["total"], ksd
    finally:
        _lib.debug_stream_jsplit(0)
    s = sc.sections(c.kind, c.n, c.d, p["jsplit"], True)
    order = ["r", "sc", "t3"] + ["planes%d" % k for k in range(sc.NSETS[c.kind])] + ["o%d" % k for k in range(sc.NSETS[c.kind])] + \
            ["rs", "sq", "rd", "kpart", "total"]
    assert [k for k in s] == order and all(s[a] < s[b] and s[a] % 256 == 0 for a, b in zip(order, order[1:]))
    # the KSD tail is appended: the plain form's sections are where the KSD form has them
    plain = sc.sections(c.kind, c.n, c.d, p["jsplit"], False)
    assert all(plain[k] == s[k] for k in plain if k != "total") and plain["total"] == s["rd"]
    # the plan's own invariants: the two clamps, ranges of whole j tiles that tile [0, jtiles), none empty
    assert 1 <= p["want"] <= p["jtiles"] and p["want"] == min(max(p["want_asked"], 1), p["jtiles"])
    assert p["ranges"][0][0] == 0 and p["ranges"][-1][1] == p["jtiles"] and len(p["ranges"]) == p["jsplit"]
    assert all(a[1] == b[0] for a, b in zip(p["ranges"], p["ranges"][1:])) and all(a < b for a, b in p["ranges"])
    assert all(b - a == p["jtiles_per"] for a, b in p["ranges"][:-1])
    assert p["nblk"] == p["row_tiles"] * p["col_units"] * p["jsplit"]
    assert p["jsplit"] == 1 or c.hook > 0 or p["nblk"] <= sc.RESIDENT


def test_the_hook_is_reset():
    assert _lib.stream_plan(16384, 256) == (128, 1, 2) and _lib.imq_plan(16384, 256) == (128, 2, 1)


def test_the_case_table_reads_as_stated():
    """what the table's comments and DESIGN.md say about the shapes they name"""
    lens = lambda kind, n, d, hook: [b - a for a, b in sc.plan(kind, n, d, hook)["ranges"]]   # noqa: E731
    for kind in ("rbf", "imq"):
        assert lens(kind, 640, 130, 1) == [5] and lens(kind, 640, 130, 2) == [3, 2]
        assert lens(kind, 640, 130, 3) == lens(kind, 640, 130, 4) == [2, 2, 1]
        assert lens(kind, 640, 130, 5) == lens(kind, 640, 256, 1000) == [1] * 5
        assert lens(kind, 768, 33, 4) == [2, 2, 2] and lens(kind, 1000, 300, 1) == [8]
        assert sc.plan(kind, 2100, 512)["sq_blocks"] == 1024 and 2100 * 512 > 1 << 20
    assert lens("rbf", 2100, 512, 0) == [3] * 5 + [2] and lens("imq", 2100, 512, 0) == [6, 6, 5]
    p, q = sc.plan("rbf", 4224, 2001), sc.plan("imq", 4224, 1025)
    assert (p["row_tiles"], p["col_units"], p["want_asked"], p["jsplit"]) == (33, 8, 0, 1)
    assert (q["row_tiles"], q["col_units"], q["want_asked"], q["jsplit"]) == (33, 9, 0, 1)
    # (the rule's quotient is 0 there and its first clamp acts; one row tile less at the RBF width and it is 1 by itself)
    assert sc.plan("rbf", 4096, 2001)["want_asked"] == 1
    assert sc.plan("rbf", 1000, 300)["sq_blocks"] == 293
    assert (sc.vec(32), sc.vec(32, "s"), sc.vec(260, "t"), sc.vec(260, "p"), sc.vec(256, "", True), sc.vec(5)) == (3, 1, 2, 2, 3, 2)


@pytest.mark.parametrize("form,name", REQUIRED, ids=["%s-%s" % r for r in REQUIRED])
def test_every_class_has_a_case(form, name):
    have = [sc.case_id(c) for c in sc.CASES if sc.form_of(c) == form and name in sc.classes(c)]
    assert have, "no %s case reaches the class %s" % (form, name)


def test_no_class_is_missing_and_none_is_named_that_the_list_does_not_hold():
    reached = {(sc.form_of(c), name) for c in sc.CASES for name in sc.classes(c)}
    missing = sorted(set(REQUIRED) - reached)
    assert not missing, "classes no case reaches: %s" % ", ".join("%s/%s" % m for m in missing)
    named = set(EVERY_FORM + RBF_ONLY + KSD_ONLY) | set(sc.FORMS)
    for c in sc.CASES:
        assert sc.classes(c) <= named, (sc.case_id(c), sorted(sc.classes(c) - named))


_GRIDS = sorted({sc.plan_of(c)["nblk"] for c in sc.CASES})


@pytest.mark.parametrize("nblk", _GRIDS)
def test_xcd_remap_is_a_permutation(nblk):
    assert sorted(sc.xcd_remap(b, nblk) for b in range(nblk)) == list(range(nblk))


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_the_workgroup_map_is_a_bijection(case):
    p = sc.plan_of(case)
    got = [sc.workgroup(p, sc.xcd_remap(b, p["nblk"])) for b in range(p["nblk"])]
    want = {(tm, cu, z) for tm in range(p["row_tiles"]) for cu in range(p["col_units"]) for z in range(p["jsplit"])}
    assert len(got) == len(set(got)) == len(want) and set(got) == want


_REFS = sorted({(c.kind, c.n, c.d, c.hook, c.mult) for c in sc.CASES})


@pytest.mark.parametrize("kind,n,d,hook,mult", _REFS, ids=["%s-%dx%d-hook%d-x%g" % r for r in _REFS])
def test_the_reference_alone_satisfies_the_gpu_tests_preconditions(kind, n, d, hook, mult):
    """inputs of normal fp32 values, a positive bandwidth, and nothing the GPU test divides by is zero: every 128 x 128 tile
    of phi and of its allowance, every tile of every range's partial sums and of their allowances, every row tile of every
    range's two row sums (rd: of its allowance -- rd of the range that holds only the diagonal of one particle is 0)"""
    c = sc.Case(kind, True, n, d, hook, "", False, mult)
    p = sc.plan_of(c)
    T64, G64 = sc.inputs(n, d)
    T, G = torch.tensor(T64), torch.tensor(G64)
    for X in (T, G):
        assert bool(torch.isfinite(X).all()) and float(X.abs().min()) >= 2.0 ** -126 and torch.equal(X.float().double(), X)
    h2 = sc.h2_of(c)
    assert 0.0 < h2 < float("inf")
    ref = sc.reference(kind, T, G, h2, p["ranges"])
    for what in ("phi", "phi_allow", "rs", "rd", "rd_allow"):
        assert bool(torch.isfinite(ref[what]).all()), what
    assert bool((sc.tiles(ref["phi"]) > 0).all()) and bool((sc.tiles(ref["phi_allow"]) > 0).all())
    for z in range(p["jsplit"]):
        for k in range(sc.NSETS[kind]):
            assert bool((sc.tiles(ref["o"][k][z]) > 0).all()), ("o", k, z)
            assert bool((sc.tiles(ref["o_allow"][k][z]) > 0).all()), ("o_allow", k, z)
        assert bool((sc.tiles(ref["rs"][z]) > 0).all()), ("rs", z)
        assert bool((sc.tiles(ref["rd_allow"][z]) > 0).all()), ("rd_allow", z)
