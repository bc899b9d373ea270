"""GPU: every implementation of the median select, end to end, on particles with small integer coordinates.

The squared distances of the lattices of tests/select_inputs.py are integers that every distance path computes exactly
(asserted first, against an int64 D), so the bandwidth of every step is known from an exact sort of that int64 D alone:
no GPU output enters the expectation.  The families put both targets deep inside a tie of up to 786 432 equal keys (line),
on the seam of two adjacent ties that part at radix level 0, 1 or 2 (two, simplex4), in a tie among hundreds of distinct
values (grid), or make every distance 0 (identical).  The paths:

    one-kernel path (n <= 160)            the LDS select of k_svgd_small
    small=False, n <= 512                 solo_select on the first steps and on every window miss, spec_select_body after
    small=False, window=False, n > 512    k_hist_all + chain_resolve + resolve_all_body, also with 3 and 4096 workgroups
    default engine, particles unchanged   k_spec_select: the 8192-key window (half-width 4096) of calls 2 and 3, the 96-key one after
    row blocks, window form               k_spec_tally + k_spec_pick (stein_rank_*), tables summed over the blocks
    row blocks, radix form / mark=        k_hist<LEVEL, SYM> + k_resolve behind the distance epilogues' level-0 counts

DESIGN.md section 4, "Median select, exact", says which branch each family reaches.
"""
import numpy as np
import pytest
import torch

import select_inputs as si
import workspace_state as wsx
from stein_amd import _lib
from stein_amd.engine import SvgdEngine, untile_distances

pytestmark = pytest.mark.gpu

VARIANTS = {"x3": dict(x3=True), "fp32mfma": dict(x3=False), "bf16": dict(dtype=torch.bfloat16)}


def _inputs(family, n, device, dtype=torch.float32):
    ref = si.lattice_ref(family, n)
    d = ref.P.shape[1]
    T = torch.tensor(ref.P, dtype=torch.float32, device=device).to(dtype).contiguous()
    G = torch.tensor(si.gaussian_scores(n, d), device=device).to(dtype).contiguous()
    assert torch.equal(T.double().cpu(), torch.tensor(ref.P, dtype=torch.float64))       # the coordinates survive the dtype
    return ref, T, G, d


def _lohi(select_bytes):
    lo, hi = select_bytes[40:48].view(torch.float32).cpu().numpy()                      # SelState::lo, ::hi
    return float(lo), float(hi)


def _assert_h2(h2, ref, tag):
    got = float(h2)
    assert got == float(ref.h2), (tag, "h2", got, float(ref.h2), "lo|hi %d|%d" % (ref.lo, ref.hi))


def _assert_exact_D(D, ref, tag):
    got = D.cpu().numpy()
    bad = got != ref.D                                                                   # (fp32 against int64, compared in fp64)
    assert not bad.any(), (tag, "D is not exact on integers", int(bad.sum()), float(np.abs(got - ref.D).max()))


def _spec_state(eng):
    u = eng.select_state[64:128].cpu().numpy().view(np.uint32)                           # SpecState (stein_common.h)
    return dict(width=int(u[4]), count=int(u[5]), overflow=int(u[6]), hit=int(u[7]))


_STAGED = {}


def _staged_result(family, n, variant, device):
    """phi, |phi|^2 of the staged calls (mark=) on this input, once per (family, n, variant); their own h2, lo, hi and D are
    held to the int64 reference as well"""
    key = (family, n, variant)
    if key not in _STAGED:
        kw = VARIANTS[variant]
        ref, T, G, d = _inputs(family, n, device, kw.get("dtype", torch.float32))
        eng = SvgdEngine(n, d, device=device, small=False, **kw)
        phi = eng.compute_phi(T, G, mark=lambda label: None).clone()
        torch.cuda.synchronize()
        _assert_exact_D(eng.dist_matrix(), ref, ("staged",) + key)
        _assert_h2(eng.h2, ref, ("staged",) + key)
        assert _lohi(eng.select_state) == (float(ref.lo), float(ref.hi)), ("staged",) + key
        _STAGED[key] = (phi, eng.sqnorm.clone())
    return _STAGED[key]


def _run_fused(family, n, variant, device, steps, lohi=True, ksd=False, record=None, **engine_kw):
    """`steps` fused calls on unchanged particles -> the hit word of every step.  Every step: exact D (first step), h2 of the
    int64 median, lo / hi, and phi / |phi|^2 bit-equal to the staged calls' where the bandwidth is a positive number."""
    kw = dict(VARIANTS[variant], **engine_kw)
    ref, T, G, d = _inputs(family, n, device, kw.get("dtype", torch.float32))
    eng = SvgdEngine(n, d, device=device, ksd=ksd, **kw)
    tag = (family, n, variant, tuple(sorted(engine_kw.items())))
    compare = float(ref.h2) > 0 and not eng.fold and not eng._one_kernel and not ksd
    if compare:
        phi_staged, sq_staged = _staged_result(family, n, variant, device)
    hits, notes = [], []
    for step in range(steps):
        phi = eng.compute_phi(T, G)
        torch.cuda.synchronize()
        if step == 0 and not eng._one_kernel:
            _assert_exact_D(eng.dist_matrix(), ref, tag)
        _assert_h2(eng.h2, ref, tag + (step,))
        if not eng._one_kernel:
            s = _spec_state(eng)
            hits.append(s["hit"])
            notes.append("w%d c%d o%d h%d" % (s["width"], s["count"], s["overflow"], s["hit"]))
            if lohi:
                assert _lohi(eng.select_state) == (float(ref.lo), float(ref.hi)), tag + (step, s)
        if compare:
            assert torch.equal(phi, phi_staged), tag + (step, "phi differs from the staged calls'")
            assert torch.equal(eng.sqnorm, sq_staged), tag + (step,)
        if float(ref.h2) == 0:
            assert not bool(torch.isfinite(phi).all()), tag              # exp(-0 / 0): NaN, as in the reference
    if record is not None:
        record("window_words%s" % ("_ksd" if ksd else ""), " | ".join(notes))   # width, count, overflow, hit of every step
    return hits


# ---- 6: the one-kernel path ----------------------------------------------------------------------------------------
SMALL_CASES = [(f, n) for n in si.SMALL_N for f in si.families_at(n)]


@pytest.mark.parametrize("family,n", SMALL_CASES, ids=lambda v: str(v))
def test_small_kernel_lds_select(cuda, family, n):
    ref, T, G, d = _inputs(family, n, cuda)
    eng = SvgdEngine(n, d, device=cuda)
    assert eng._one_kernel
    for step in range(2):
        eng.h2.fill_(float("nan"))
        eng.compute_phi(T, G)
        _assert_h2(eng.h2, ref, (family, n, step))
    if (family, n) in (("simplex4_128_1", 160), ("line", 129)):
        ksd = SvgdEngine(n, d, device=cuda, ksd=True)
        ksd.compute_phi(T, G)
        _assert_h2(ksd.h2, ref, (family, n, "ksd"))


# ---- 3 and 4: solo_select, then the window, n <= 512 ---------------------------------------------------------------------
SOLO_CASES = [(f, n) for n in si.SOLO_N for f in si.families_at(n)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("family,n", SOLO_CASES, ids=lambda v: str(v))
def test_solo_select_and_window_up_to_512(cuda, family, n, variant, record_property):
    hits = _run_fused(family, n, variant, cuda, steps=5, small=False, record=record_property)
    assert hits[0] == 0                                       # no prediction yet: solo_select ran
    if (family, n, variant) == ("simplex4_64_1", 384, "x3"):
        _run_fused(family, n, variant, cuda, steps=3, small=False, ksd=True)


# ---- 2: the one-launch chained select ----------------------------------------------------------------------------------
HIST_ALL_CASES = [(f, n) for n in si.HIST_ALL_N for f in (si.families_at(n) if n != 2304 else ["line"])]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("family,n", HIST_ALL_CASES, ids=lambda v: str(v))
def test_one_launch_select(cuda, family, n, variant, record_property):
    hits = _run_fused(family, n, variant, cuda, steps=3, small=False, window=False, record=record_property)
    assert hits == [0, 0, 0]
    if (family, n, variant) == ("simplex4_128_2", 768, "x3"):
        _run_fused(family, n, variant, cuda, steps=2, small=False, window=False, ksd=True)


@pytest.mark.parametrize("grid", [3, 4096])
def test_one_launch_select_with_stealing(cuda, grid):
    """three workgroups take over all 512 virtual ones; 4096 find theirs taken: the L2 straddle on 1.3 and 2.7 million ties"""
    _lib.call("stein_debug_hist_all_grid", grid)
    try:
        hits = _run_fused("simplex4_128_1", 2304, "x3", cuda, steps=2, small=False, window=False)
    finally:
        _lib.call("stein_debug_hist_all_grid", 0)
    _lib.call("stein_take_device_error")                      # nothing gave up
    assert hits == [0, 0]


# ---- 4: the single-rank window --------------------------------------------------------------------------------------
WINDOW_CASES = [(f, n) for n in si.WINDOW_N for f in si.families_at(n)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("family,n", WINDOW_CASES, ids=lambda v: str(v))
def test_window_on_unchanged_particles(cuda, family, n, variant, record_property):
    """Default engine, 8 calls, the particles do not move.  The first call records the key (no window); the second and third
    get the 8192-key window [lo - 4096, lo + 4096] around it (spec_update_dev: half-width 4096 until a window centred on a
    real prediction has measured an error); from the fourth call on the earned 96-key window (half-width 48, error 0).  The bandwidth, lo and hi are the hard assertions at every step; the window words of every step
    (width, count, overflow, hit) are printed.  For simplex4_128_1 lo | hi lie 256 keys apart: both inside the 8192-key
    window, in different high bytes of it, and outside each other's 96-key window.  A family whose lo is 0 (two,
    identical) never gets a window: median_init_body grants none at or below the key of +0.
    Observed on the MI355X, the same in all three variants and at n = 768 and 1536 (also 384 and 512, small=False):
    widths 0, 8192, 8192, 96, 96, ...; grid hits from the second call on (0 1 1 1 1 1 1 1; 1153 buffered entries at 768);
    every simplex4 and line records 0 0 0 0 0 0 0 0 with overflow set on every windowed call -- one 128 x 128 tile holds far
    more entries of lo's tie than the 1016 of a workgroup's queue (count = 1016 x the 21 / 78 upper tiles), so the radix
    select answers and the two_hb branch of spec_select_body is not reached by them.
    scatter is the family that reaches it: lo | hi on different values 1024 (n = 768) and 4096 (n = 1536) keys apart, a few
    hundred entries in the 8192-key window, far below every queue's capacity.  So the second call -- window [lo - 4096,
    lo + 4096], both targets inside, in different high bytes -- must hit (asserted: nothing in spec_select_body can refuse
    it), and from the fourth call on the 96-key window holds lo alone: hi lies above it, a miss by bb == 256 (asserted)."""
    hits = _run_fused(family, n, variant, cuda, steps=8, record=record_property)
    assert hits[0] == 0
    if family == "scatter":
        assert hits[1] == 1 and hits[2] == 1, hits          # two_hb: one low-byte histogram per target
        assert hits[3:] == [0] * 5, hits                     # hi above the earned window
    if family == "grid" and n == 768:
        assert sum(hits) >= 1, hits
    if (family, n, variant) == ("grid", 768, "x3"):
        _run_fused(family, n, variant, cuda, steps=4, ksd=True)


@pytest.mark.parametrize("family,n", si.OVER_CAPACITY, ids=lambda v: str(v))
def test_ties_at_zero_beyond_the_buffer_open_no_window(cuda, family, n, record_property):
    """More upper-triangle entries equal to lo than the window buffer holds (SPEC_CAP) -- but lo = 0, and median_init_body
    grants a window only above the key of +0: no window opens on any call (width 0, asserted), the cnt > SPEC_CAP refusal
    is NOT reached, and the one-launch radix select answers over 2.4 / 2.7 million tied upper-triangle entries."""
    hits = _run_fused(family, n, "x3", cuda, steps=4, record=record_property)
    assert sum(hits) == 0
    ref, T, G, d = _inputs(family, n, cuda)
    eng = SvgdEngine(n, d, device=cuda)
    for _ in range(3):
        eng.compute_phi(T, G)
        assert _spec_state(eng)["width"] == 0


# ---- 5 and 1: row blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [True, False], ids=["tally-pick", "radix"])
@pytest.mark.parametrize("family", si.families_at(768))
def test_two_row_blocks(cuda, family, window, record_property):
    """n = 768 as the ragged row blocks [0, 300) and [300, 768) of one process, through stein_rank_*: the window form sums the
    blocks' tables and picks (k_spec_tally / k_spec_pick), the radix form sums their histograms (k_hist<L, false> behind
    the non-symmetric epilogues' level-0 counts).  6 steps on unchanged particles."""
    n = 768
    ref, T, G, d = _inputs(family, n, cuda)
    blocks = wsx.RankBlocks(n, d, [(0, 300), (300, 468)], cuda, window)
    notes = []
    for step in range(6):
        res = blocks.step(T, G)
        if step == 0:
            _assert_exact_D(res["D"], ref, (family, "row blocks"))
        _assert_h2(res["h2"], ref, (family, window, step))
        for b in blocks.blocks:
            o = b._offs[_lib.WS_SELECT]
            assert _lohi(b.ws[o:o + 64]) == (float(ref.lo), float(ref.hi)), (family, window, step, b.row0)
        notes.append(blocks.window_stats())
    record_property("steps_hits", str(notes))
    if not window:
        assert notes[-1][1] == 0
    elif family in ("grid", "scatter"):
        # ties that fit the queues: k_spec_pick must have delivered medians itself (lo == hi for grid; scatter's second
        # and third step hold both of its targets, 1024 keys apart), not left every step to the radix select
        assert notes[-1][1] >= 2, notes


PANEL_CASES = [(f, n) for n in si.PANEL_N for f in si.families_at(n)]


@pytest.mark.parametrize("family,n", PANEL_CASES, ids=lambda v: str(v))
def test_staged_calls_behind_the_panel_kernel(cuda, family, n):
    """The staged calls with the panel-resident distance kernel forced, at every multiple of 128 this module uses and every
    family (no fused call below n = 8192 takes that kernel by itself): its epilogue's level-0 counts, then
    k_hist<1..2, true> and k_resolve; the per-tile kernel beside it."""
    ref, T, G, d = _inputs(family, n, cuda)
    eng = SvgdEngine(n, d, device=cuda, small=False)
    st = eng.stages
    st.rownorms(T, n, d, eng.rownorm)
    st.x3_prepare(T, G, n, d, eng.planes)
    for kernel in (_lib.STAGE_PANEL, _lib.STAGE_TILES):
        eng.dist.fill_(float("nan"))
        eng.h2.fill_(float("nan"))
        st.median_begin(eng.hist, eng.select_state, n * n)
        st.distance_block(T, eng.rownorm, n, d, 0, n, eng.dist, eng.ld_dist, hist0=eng.hist[0], symmetric=True,
                          planes=eng.planes, kernel=kernel)
        for level in range(_lib.HIST_LEVELS):
            if level > 0:
                st.median_hist_pass(eng.dist, eng.ld_dist, n, n, level, eng.select_state, eng.hist, symmetric=True)
            st.median_resolve(eng.hist, level, n, eng.select_state, eng.h2, eng.median)
        torch.cuda.synchronize()
        _assert_exact_D(untile_distances(eng.dist, n, n, upper=True), ref, (family, n, kernel))
        _assert_h2(eng.h2, ref, (family, n, kernel))
        assert _lohi(eng.select_state) == (float(ref.lo), float(ref.hi)), (family, n, kernel)
        assert float(eng.median) == float(ref.med)
