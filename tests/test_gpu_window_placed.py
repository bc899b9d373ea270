"""GPU: the speculative median window, placed by hand (the table and the model: tests/window_cases.py, proven on the CPU by
tests/test_window_cases.py).

SpecState persists in the SELECT section between calls, and median_init_body reads `magic`, `center` and `halfwidth` from
it at the start of the fused call, of stein_spec_begin and of stein_rank_begin: a test that writes those three words gets
the window it asks for.  The lattices' distances are integers every distance path computes exactly, so every key is known
from an int64 D and a window edge can be put one key beside a target.  Every expectation -- the window words, the table
word for word, hit or miss and why -- comes from the CPU model; nothing is skipped at run time.

    fused call        k_spec_select (spec_select_body, and solo_select behind each of its early exits at n = 384)
    staged calls      spec_begin -> distance_block_spec -> spec_tally -> spec_pick, symmetric / a ragged row block off the
                      origin / the per-tile kernel forced / the panel kernel forced
    rank segments     two ragged row blocks through stein_rank_*
    counts            normal inputs, 2048 x 64, the 65535-key window: the loop path of spec_select_body, more entries than the
                      buffer holds, the predictor's halving -- judged by the kernel's own stored image
"""
import numpy as np
import pytest
import torch

import select_inputs as si
import window_cases as wc
import workspace_state as wsx
from stein_amd import _lib
from stein_amd.engine import HipStages, SvgdEngine, untile_distances
from test_gpu_baseline_sizes import check_exact_bandwidth

pytestmark = pytest.mark.gpu

VARIANTS = {"x3": dict(x3=True), "fp32mfma": dict(x3=False), "bf16": dict(dtype=torch.bfloat16)}
WORDS = ("magic", "center", "halfwidth", "lo_key", "width", "count", "overflow", "hit", "earned_hw", "reserved", "total_lo",
         "total_hi", "last_key", "skip_l0", "n_steps", "n_hits")
PREDICTOR = ("magic", "center", "halfwidth", "earned_hw", "last_key", "n_steps", "n_hits")
SYM = [c for c in wc.case_table("sym")]
ROWS = [c for c in wc.case_table("rows")]
ONCE = [c for c in SYM if c.reps == 1 and c.total is None]      # what a fused call, whose total is n^2, can be given
EDGE = [c for c in ONCE if c.edge]


def _words(sel):
    u = sel[64:128].cpu().numpy().view(np.uint32)
    return {k: int(v) for k, v in zip(WORDS, u)}


def _lohi(sel):
    lo, hi = sel[40:48].view(torch.float32).cpu().numpy()
    return float(lo), float(hi)


def _place(sel, center, halfwidth):
    """magic = SPEC_MAGIC2, center, halfwidth -> bytes 64..75 of a SELECT section"""
    w = np.array([wsx.spec_magic_words()[1], center, halfwidth], dtype=np.uint32).view(np.uint8)
    sel[64:76].copy_(torch.from_numpy(w.copy()).to(sel.device))


def _inputs(family, n, device, dtype=torch.float32):
    P = wc.lattice_points(family, n)
    T = torch.tensor(P, dtype=torch.float32, device=device).to(dtype).contiguous()
    G = torch.tensor(si.gaussian_scores(n, P.shape[1]), device=device).to(dtype).contiguous()
    assert torch.equal(T.double().cpu(), torch.tensor(P, dtype=torch.float64))
    return T, G, P.shape[1]


def _h2(ent, med=None):
    return float(si.bandwidth(ent.med if med is None else med, ent.n))


_ENGINES, _STAGED_PHI = {}, {}


def _staged_phi(family, n, variant, device):
    """phi, |phi|^2 of the staged calls (radix select) on this input, their D, h2, lo, hi held to the int64 reference"""
    key = (family, n, variant)
    if key not in _STAGED_PHI:
        kw = VARIANTS[variant]
        T, G, d = _inputs(family, n, device, kw.get("dtype", torch.float32))
        ent = wc.entries_of(family, n, "sym")
        eng = SvgdEngine(n, d, device=device, small=False, **kw)
        phi = eng.compute_phi(T, G, mark=lambda label: None).clone()
        torch.cuda.synchronize()
        assert not (eng.dist_matrix().cpu().numpy() != wc.lattice_D(family, n)).any(), (key, "D is not exact on integers")
        assert float(eng.h2) == _h2(ent) and _lohi(eng.select_state) == (float(ent.lo), float(ent.hi)), key
        _STAGED_PHI[key] = (phi, eng.sqnorm.clone())
    return _STAGED_PHI[key]


def _fused_engine(family, n, variant, small, device):
    """one engine per input, its predictor initialised by one call"""
    key = (family, n, variant, small)
    if key not in _ENGINES:
        kw = VARIANTS[variant]
        T, G, d = _inputs(family, n, device, kw.get("dtype", torch.float32))
        eng = SvgdEngine(n, d, device=device, small=small, **kw)
        eng.compute_phi(T, G)
        torch.cuda.synchronize()
        assert not eng._one_kernel
        assert not (eng.dist_matrix().cpu().numpy() != wc.lattice_D(family, n)).any(), (key, "D is not exact on integers")
        _ENGINES[key] = (eng, T, G)
    return _ENGINES[key]


def _check_fused(case, variant, small, device):
    eng, T, G = _fused_engine(case.family, case.n, variant, small, device)
    ent, s = case.entries, case.step("tiles")
    sel = eng.select_state
    _place(sel, case.center, case.halfwidth)
    before = _words(sel)
    eng.h2.fill_(float("nan"))
    phi = eng.compute_phi(T, G)
    torch.cuda.synchronize()
    after = _words(sel)
    tag = (case.id, variant, small, s.outcome, after)
    print(case.id, variant, "outcome", s.outcome, "path", s.path, "two_hb", s.two_hb, "count", after["count"], "largest queue", s.max_queue)
    # the window this step had, and what the producer and the select made of it
    assert (after["lo_key"], after["width"]) == (s.lo_key, s.width), tag
    assert after["count"] == s.count and after["overflow"] == int(s.overflow), tag + (s.count,)
    assert after["hit"] == int(s.outcome == "hit"), tag
    # whatever the outcome: the int64 sort's targets and bandwidth, phi and |phi|^2 of the staged calls
    assert _lohi(sel) == (float(ent.lo), float(ent.hi)), tag
    assert float(eng.h2) == _h2(ent), tag
    if _h2(ent) > 0 and not eng.fold:
        phi_staged, sq_staged = _staged_phi(case.family, case.n, variant, device)
        assert torch.equal(phi, phi_staged) and torch.equal(eng.sqnorm, sq_staged), tag
    # the predictor, replayed from the words in front of the call (every outcome updates it, a hit inside k_spec_select)
    want = wc.predictor_update({k: before[k] for k in PREDICTOR}, ent.key_lo, s.width, s.outcome == "hit", s.count)
    assert {k: after[k] for k in PREDICTOR} == want, tag + (want,)


# ---- the fused call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONCE, ids=lambda c: c.id)
def test_fused_call_on_a_placed_window(cuda, case):
    _check_fused(case, "x3", True, cuda)


@pytest.mark.parametrize("case", [c for c in ONCE if c.n == 384], ids=lambda c: c.id)
def test_fused_call_small_false_ends_in_solo_select(cuda, case):
    """n = 384, small=False: every miss is resolved by solo_select in the same workgroup, behind whichever early exit of
    spec_select_body the placement takes (each lies behind a different number of barriers and state of its LDS arrays)"""
    _check_fused(case, "x3", False, cuda)


@pytest.mark.parametrize("variant", ["fp32mfma", "bf16"])
@pytest.mark.parametrize("case", EDGE, ids=lambda c: c.id)
def test_fused_call_edges_on_the_other_distance_paths(cuda, case, variant):
    _check_fused(case, variant, True, cuda)


# ---- the staged calls -----------------------------------------------------------------------------------------------------
class Staged:
    """one workspace, the staged window calls on a block of it"""

    def __init__(self, P, row0, nl, device, T=None, G=None):
        self.n, self.d = P.shape if T is None else T.shape
        n, d = self.n, self.d
        self.row0, self.nl, self.st = row0, nl, HipStages()
        total, offs, extra = _lib.workspace_layout(nl, n, d, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_TILED)
        self.ws = torch.zeros(total, dtype=torch.uint8, device=device)
        self.ld = extra[_lib.WSX_LD_DIST]
        rows = (nl + 127) // 128 * 128

        def view(sec, nbytes, dtype, at=0):
            return self.ws[offs[sec] + at:offs[sec] + at + nbytes].view(dtype)
        self.r = view(_lib.WS_ROWNORM, 4 * n, torch.float32)
        self.D = view(_lib.WS_DIST, rows * self.ld * 4, torch.float32).view(rows, self.ld)
        self.hist = view(_lib.WS_HIST, _lib.HIST_LEVELS * 2 * _lib.HIST_BINS * 8, torch.int64).view(_lib.HIST_LEVELS, 2, _lib.HIST_BINS)
        self.sel = view(_lib.WS_SELECT, _lib.SELECT_BYTES, torch.uint8)
        self.spec = self.ws[offs[_lib.WS_SPEC]:offs[_lib.WS_PLANES]]
        self.table = view(_lib.WS_SPEC, 8 * _lib.SPEC_TABLE_WORDS, torch.int64, 8 * _lib.SPEC_TABLE_OFFSET_WORDS)
        self.planes = self.ws[offs[_lib.WS_PLANES]:total]
        self.T = torch.tensor(P, dtype=torch.float32, device=device).contiguous() if T is None else T
        self.G = torch.tensor(si.gaussian_scores(n, d), device=device).contiguous() if G is None else G
        self.h2, self.med = torch.zeros(1, device=device), torch.zeros(1, device=device)
        self.st.rownorms(self.T, n, d, self.r)
        self.st.x3_prepare(self.T, self.G, n, d, self.planes)

    def run(self, center, halfwidth, sym, kernel, reps=1, total=None):
        """-> (table, hit): begin, `reps` submissions of the block, tally, pick; after a miss the radix passes"""
        st, n, d, nl = self.st, self.n, self.d, self.nl
        _place(self.sel, center, halfwidth)
        self.h2.fill_(float("nan")), self.med.fill_(float("nan"))
        st.spec_begin(self.hist, self.sel, self.spec, reps * nl * n if total is None else total)
        for _ in range(reps):
            st.distance_block_spec(self.T, self.r, n, d, self.row0, nl, self.D, self.ld, self.hist[0], self.sel, self.spec,
                                   planes=self.planes, kernel=kernel, symmetric=sym)
        st.spec_tally(self.sel, self.spec)
        st.spec_pick(self.sel, self.spec, n, self.h2, self.med)
        torch.cuda.synchronize()
        table = self.table.cpu().numpy().copy()
        w = _words(self.sel)
        if not w["hit"]:
            for level in range(_lib.HIST_LEVELS):
                if level > 0 or not w["skip_l0"]:
                    for _ in range(reps):      # (the ranks are those of the reps-fold multiset)
                        st.median_hist_pass(self.D, self.ld, nl, n, level, self.sel, self.hist, symmetric=sym)
                st.median_resolve(self.hist, level, n, self.sel, self.h2, self.med)
            torch.cuda.synchronize()
        return table, w

    def image(self, sym):
        return untile_distances(self.D, self.nl, self.n, upper=sym).cpu().numpy()


_STAGES = {}


def _stage(family, n, form, device):
    key = (family, n, form)
    if key not in _STAGES:
        row0, nl = (0, n) if form == "sym" else wc.ROW_BLOCK
        _STAGES[key] = Staged(wc.lattice_points(family, n), row0, nl, device)
    return _STAGES[key]


def _check_table(table, s, tag, exact_count=True):
    hdr = wc.constants()["SPEC_TABLE_HDR"]
    assert int(table[0]) == s.below and int(table[1]) == int(s.table[1]), tag + (table[:3].tolist(), s.table[:3].tolist())
    if exact_count:
        assert int(table[2]) == s.count, tag + (int(table[2]), s.count)
    assert not table[3:hdr].any(), tag
    got = table[hdr:hdr + s.width + 1]
    assert np.array_equal(got, s.table[hdr:]), tag + ("key counters", np.flatnonzero(got != s.table[hdr:])[:8].tolist())
    assert not table[hdr + s.width + 1:].any(), tag + ("a counter past the window",)


def _check_staged(case, form, kernel, device):
    geometry = "panel" if kernel == _lib.STAGE_PANEL else "tiles"
    sg = _stage(case.family, case.n, form, device)
    ent, s = case.entries, case.step(geometry)
    sym = form == "sym"
    table, w = sg.run(case.center, case.halfwidth, sym, kernel, case.reps, case.total)
    lo, hi, med = case.targets()
    tag = (case.id, geometry, s.outcome, {k: w[k] for k in ("lo_key", "width", "count", "overflow", "hit")})
    if (case.name, geometry) in (("lo_first", "tiles"), ("tie", "tiles")):
        D = wc.lattice_D(case.family, case.n)
        assert not (sg.image(sym) != D[sg.row0:sg.row0 + sg.nl]).any(), tag + ("D is not exact on integers",)
    assert (w["lo_key"], w["width"]) == (s.lo_key, s.width), tag
    _check_table(table, s, tag, exact_count=s.count_exact)
    if not s.count_exact:
        # the panel kernel's queues drop what does not fit: at least one full queue arrived, never more than there is
        assert wc.constants()["DP_QCAP"] <= int(table[2]) <= s.count, tag
        assert int(table[2]) != case.step("tiles").count, tag + ("the per-tile kernel's count: the panel kernel did not run",)
    assert w["count"] == int(table[2]) and w["overflow"] == int(s.overflow), tag
    assert w["hit"] == int(s.outcome == "hit"), tag
    assert _lohi(sg.sel) == (float(lo), float(hi)), tag
    assert float(sg.h2) == _h2(ent, med) and float(sg.med) == float(med), tag


@pytest.mark.parametrize("case", SYM, ids=lambda c: c.id)
def test_staged_symmetric(cuda, case):
    _check_staged(case, "sym", 0, cuda)


@pytest.mark.parametrize("case", ROWS, ids=lambda c: c.id)
def test_staged_row_block_off_the_origin(cuda, case):
    _check_staged(case, "rows", 0, cuda)


@pytest.mark.parametrize("case", SYM, ids=lambda c: c.id)
def test_staged_per_tile_kernel(cuda, case):
    _check_staged(case, "sym", _lib.STAGE_TILES, cuda)


@pytest.mark.parametrize("case", [c for c in SYM if c.panel_ok], ids=lambda c: c.id)
def test_staged_panel_kernel(cuda, case):
    """STAGE_PANEL takes the panel kernel whenever its restrictions hold: n, n_local and row0 multiples of 128 (asserted;
    the overflow cases also tell the kernels apart by their count: whole queues of DP_QCAP, not of SPEC_QCAP, entries)"""
    assert case.n % 128 == 0
    _check_staged(case, "sym", _lib.STAGE_PANEL, cuda)


# ---- two ragged row blocks through the rank segments ------------------------------------------------------------------------
RANK_BOUNDS = [(0, 300), (300, 468)]
RANK_CASES = [c for c in ONCE if c.n == 768]
_RANKS = {}


def _rank_blocks(family, device):
    if family not in _RANKS:
        T, G, d = _inputs(family, 768, device)
        blocks = wsx.RankBlocks(768, d, RANK_BOUNDS, device, window=True)
        res = blocks.step(T, G)
        assert not (res["D"].cpu().numpy() != wc.lattice_D(family, 768)).any()
        _RANKS[family] = (blocks, T, G, wc.entries_blocks(wc.lattice_D(family, 768), RANK_BOUNDS))
    return _RANKS[family]


@pytest.mark.parametrize("case", RANK_CASES, ids=lambda c: c.id)
def test_rank_segments_on_a_placed_window(cuda, case):
    """the same placements (the two blocks hold the symmetric multiset, every entry once) with the same three words written
    into both blocks' SELECT sections: the blocks agree, the result is exact, and the hit counter moves by the model's hit"""
    blocks, T, G, ent = _rank_blocks(case.family, cuda)
    s = wc.window_step(ent, case.center, case.halfwidth)
    assert s.outcome == case.step().outcome and (float(ent.lo), float(ent.hi)) == (float(case.entries.lo), float(case.entries.hi))
    sels = []
    for b in blocks.blocks:
        o = b._offs[_lib.WS_SELECT]
        sels.append(b.ws[o:o + _lib.SELECT_BYTES])
        _place(sels[-1], case.center, case.halfwidth)
    steps, hits = blocks.window_stats()
    res = blocks.step(T, G)
    words = [_words(sel) for sel in sels]
    tag = (case.id, s.outcome, words[0])
    # (`overflow` is a block's own word; everything else is the same on every block)
    assert [{k: v for k, v in w.items() if k != "overflow"} for w in words[1:]] == \
           [{k: v for k, v in words[0].items() if k != "overflow"}], (case.id, "the blocks' window states differ", words)
    assert (words[0]["lo_key"], words[0]["width"]) == (s.lo_key, s.width), tag
    assert words[0]["count"] == s.count and words[0]["hit"] == int(s.outcome == "hit"), tag + (s.count,)
    assert float(res["h2"]) == _h2(ent), tag
    for sel in sels:
        assert _lohi(sel) == (float(ent.lo), float(ent.hi)), tag
    assert blocks.window_stats() == (steps + 1, hits + int(s.outcome == "hit")), tag
    # the summed table, as every block holds it: [1] counts the blocks that could not tally (a block without a window, or
    # one of whose queues overflowed); the key counters are complete when no block is among them
    own = [wc.window_step(wc.entries_rows(wc.lattice_D(case.family, 768), r0, nl), case.center, case.halfwidth, total=768 * 768)
           for r0, nl in RANK_BOUNDS]
    bad = sum(int(o.table[1]) for o in own)
    assert [w["overflow"] for w in words] == [int(o.overflow) for o in own], tag
    hdr = wc.constants()["SPEC_TABLE_HDR"]
    for b in blocks.blocks:
        o = b._offs[_lib.WS_SPEC] + 8 * _lib.SPEC_TABLE_OFFSET_WORDS
        table = b.ws[o:o + 8 * _lib.SPEC_TABLE_WORDS].view(torch.int64).cpu().numpy()
        assert int(table[0]) == s.below and int(table[1]) == bad and int(table[2]) == s.count, tag + (table[:3].tolist(),)
        if not bad:
            assert np.array_equal(table[hdr:hdr + s.width + 1], s.table[hdr:]) and not table[hdr + s.width + 1:].any(), tag


# ---- counts no lattice reaches -----------------------------------------------------------------------------------------------
COUNT_N, COUNT_D = 2048, 64


def _normal(device):
    rng = np.random.default_rng([COUNT_N, COUNT_D, 17])
    T = torch.tensor(rng.normal(size=(COUNT_N, COUNT_D)), dtype=torch.float32, device=device)
    G = torch.tensor(rng.normal(size=(COUNT_N, COUNT_D)), dtype=torch.float32, device=device)
    return T, G


def test_loop_path_of_the_fused_select(cuda, record_property):
    """One fused step with more than 16 x 1024 buffered entries: pass 1 of spec_select_body takes its loop.  The 65535-key
    window is centred on the kernel's own median of the call before; the expectation is the key histogram of the image the
    step itself stored (the window tests the raw bits of the very values it stores)."""
    c = wc.constants()
    n, d = COUNT_N, COUNT_D
    T, G = _normal(cuda)
    eng = SvgdEngine(n, d, device=cuda)
    eng.compute_phi(T, G)
    torch.cuda.synchronize()
    key = int(si.f32_key(np.float32(_lohi(eng.select_state)[0])))
    _place(eng.select_state, key, c["SPEC_HW_MAX"])
    before = _words(eng.select_state)
    eng.compute_phi(T, G)
    torch.cuda.synchronize()
    after = _words(eng.select_state)
    ent = wc.entries_image(untile_distances(eng.dist, n, n, upper=True).cpu().numpy(), upper=True)
    s = wc.window_step(ent, key, c["SPEC_HW_MAX"])
    record_property("entries_largest_queue", "%d %d" % (s.count, s.max_queue))
    print("loop path: entries", s.count, "largest queue", s.max_queue)
    assert s.max_queue <= c["SPEC_QCAP"], "precondition: a 128 x 128 tile holds more window entries than a queue"
    assert s.count > c["INREG"] and s.outcome == "hit" and s.path == "loop", (s.count, s.outcome, s.path)
    assert (after["lo_key"], after["width"], after["count"], after["overflow"], after["hit"]) == (s.lo_key, s.width, s.count, 0, 1), after
    assert _lohi(eng.select_state) == (float(s.lo), float(s.hi)) == (float(ent.lo), float(ent.hi))
    check_exact_bandwidth([eng.dist], eng.select_state.view(torch.float32), n, eng.h2.item(), upper=True)
    want = wc.predictor_update({k: before[k] for k in PREDICTOR}, ent.key_lo, s.width, True, s.count)
    assert {k: after[k] for k in PREDICTOR} == want


_COUNT_STAGE = {}


def _count_stage(device):
    """the 2048 x 2048 block as a rectangular block (every entry once), its image's entries and the kernel's own median"""
    if not _COUNT_STAGE:
        T, G = _normal(device)
        sg = Staged(None, 0, COUNT_N, device, T=T, G=G)
        table, w = sg.run(wc.KEY_ZERO + 48, 0, False, 0)               # no window: the radix passes, and the image
        assert w["width"] == 0 and not w["hit"]
        ent = wc.entries_image(sg.image(False), upper=False)
        assert _lohi(sg.sel) == (float(ent.lo), float(ent.hi))
        _COUNT_STAGE.update(sg=sg, ent=ent)
    return _COUNT_STAGE["sg"], _COUNT_STAGE["ent"]


SHIFT = 5000      # the window's centre lies this many keys below lo: 4 x 5000 + 48 is more than half of SPEC_HW_MAX


def test_more_entries_than_the_buffer_holds(cuda, record_property):
    """The same row block submitted r times between one spec_begin(total = r n_local n) and one spec_tally: `count`
    accumulates and no queue overflows.  r - 1 repetitions stay under SPEC_CAP and must hit with r - 1 times the single
    table; r repetitions exceed it: [1] = 1, [2] = count, no key counter, no hit, and the radix passes deliver the median
    of the r-fold multiset, which is the block's own."""
    c = wc.constants()
    sg, ent = _count_stage(cuda)
    center, hw = ent.key_lo - SHIFT, c["SPEC_HW_MAX"]
    one = wc.window_step(ent, center, hw)
    assert one.outcome == "hit" and one.max_queue <= c["SPEC_QCAP"]
    r = c["SPEC_CAP"] // one.count + 1
    for reps, outcome in ((r - 1, "hit"), (r, "over_capacity")):
        s = wc.window_step(ent, center, hw, reps=reps)
        assert s.outcome == outcome, (reps, s.outcome, s.count)
        table, w = sg.run(center, hw, False, 0, reps)
        print("capacity:", reps, "submissions, entries", s.count, "largest queue", s.max_queue, "->", outcome)
        record_property("entries_%s" % outcome, "%d x %d, largest queue %d" % (reps, one.count, s.max_queue))
        _check_table(table, s, (reps, outcome))
        if outcome == "hit":
            hdr = c["SPEC_TABLE_HDR"]
            assert np.array_equal(table[hdr:hdr + s.width + 1], reps * one.table[hdr:]) and s.path == "loop"
        else:
            assert int(table[1]) == 1 and int(table[2]) == s.count > c["SPEC_CAP"] and not table[c["SPEC_TABLE_HDR"]:].any()
        assert w["hit"] == int(outcome == "hit") and w["count"] == s.count and w["overflow"] == 0, w
        assert _lohi(sg.sel) == (float(ent.lo), float(ent.hi)), (reps, outcome)
        check_exact_bandwidth([sg.D], sg.sel[:64].view(torch.float32), COUNT_N, sg.h2.item(), upper=False)


def test_predictor_halves_the_window_of_a_full_buffer(cuda, record_property):
    """spec_update_dev: a hit that buffered more than SPEC_CAP / 2 entries halves the next half-width (halfwidth / 2 + 1)
    when the rule would have left it larger than that; one submission fewer, just under the threshold, leaves the rule's
    value.  The prediction error is SHIFT keys, so the rule alone gives 4 x SHIFT + 48."""
    c = wc.constants()
    sg, ent = _count_stage(cuda)
    center, hw = ent.key_lo - SHIFT, c["SPEC_HW_MAX"]
    one = wc.window_step(ent, center, hw)
    r = (c["SPEC_CAP"] // 2) // one.count + 1
    for reps, halved in ((r, True), (r - 1, False)):
        s = wc.window_step(ent, center, hw, reps=reps)
        assert s.outcome == "hit" and (s.count > c["SPEC_CAP"] // 2) == halved, (reps, s.count)
        table, w = sg.run(center, hw, False, 0, reps)
        _check_table(table, s, (reps, halved))
        assert w["hit"] == 1 and w["count"] == s.count
        sg.st.spec_update(sg.sel)
        torch.cuda.synchronize()
        after = _words(sg.sel)
        print("halving:", reps, "submissions, entries", s.count, "-> half-width", after["halfwidth"])
        record_property("entries_halved_%s" % halved, "%d -> half-width %d" % (s.count, after["halfwidth"]))
        assert after["halfwidth"] == (hw // 2 + 1 if halved else 4 * SHIFT + 48), after
        assert after["earned_hw"] == 4 * SHIFT + 48
        want = wc.predictor_update({k: w[k] for k in PREDICTOR}, ent.key_lo, s.width, True, s.count)
        assert {k: after[k] for k in PREDICTOR} == want, (after, want)
