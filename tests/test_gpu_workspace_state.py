"""GPU: a step's result never depends on what its workspace held (include/steinhip.h: "identical either way (and for any
workspace contents)"; only the SELECT section "must persist from one call to the next"; one workspace serves call after
call).

The folded contraction parks its partial sums in storage other stages own (PART_G + PART_T, theta's row-major planes, the
score's planes and scales), which is right only while every call rewrites everything it reads, padding included.  Tests
that repeat one input on one engine cannot see a violation: what a kernel fails to write is found in the workspace, left
by the call before and equal to the right value.  Here

  (a) every path runs a sequence of different inputs (workspace_state.input_sequence) on one engine whose workspace is
      overwritten before every call -- zeros, 0xFF, 0x7B, another step's leftovers; all but SELECT, and once SELECT too --
      and every call must equal, bit for bit, a fresh engine's one call on a zeroed workspace (workspace_state.fresh_result):
      phi, h2, the sums, dK, K and the distance matrix.  An unpoisoned twin running the same sequence must count the same
      window hits: poison neither costs nor grants one.
  (b) one workspace serves changing requests (plain, dK, K, dK + K; at the ABI: FOLD, NO_FOLD, NO_WINDOW, TILE_DISTANCE
      and their combinations) on changing inputs, each call again equal to a fresh engine's.
  (c) the fresh result itself is held to the fp64 oracle by test_gpu_conditioning's checks: two sides wrong alike would
      pass (a) and (b).

Every comparison with a fresh engine is torch.equal.  The only tolerances are test_gpu_conditioning's (_check_columns,
_check_bandwidth) and, for the shape whose fold appends its storage, test_gpu_fold's bound on sampled fp64 rows.
Run with -s to see window hits and the anchor's figures."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_conditioning as tc  # noqa: E402
import test_gpu_fold as tf  # noqa: E402
import workspace_state as wsx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED = [(700, 300), (1281, 129), (1279, 257), (385, 1)]
FOLD_SHAPES = RAGGED + [(640, 2001), (1536, 130)]
APPENDED = (3072, 521)     # the fold's partial sums do not fit the storage it reuses: a forced fold appends them to PLANES
BF16 = torch.bfloat16


def _request(variant, call, n):
    """(dK, K) of call number `call`: the folded variants keep theirs, every other path alternates dK and asks for K once"""
    if variant in ("plain", "ksd", "nowindow"):
        return False, False
    if variant == "dK":
        return True, False
    if variant == "K":
        return False, True
    return call % 2 == 1, call == 2 and n <= 4096


# (id, engine arguments, request variant, shapes, steps of the wild sequence, drift steps, patterns)
PATHS = [
    ("unfolded", dict(fold=False, small=False), "mixed", RAGGED, 5, 3, wsx.PATTERNS),
    ("folded", dict(fold=True, small=False), "plain", FOLD_SHAPES, 5, 3, wsx.PATTERNS),
    ("folded-dK", dict(fold=True, small=False), "dK", FOLD_SHAPES, 5, 3, wsx.PATTERNS),
    ("folded-ksd", dict(fold=True, small=False, ksd=True), "ksd", FOLD_SHAPES, 5, 3, wsx.PATTERNS),
    ("folded-K", dict(fold=True, small=False), "K", FOLD_SHAPES, 5, 0, wsx.PATTERNS),
    ("folded-nowindow", dict(fold=True, small=False, window=False), "nowindow", FOLD_SHAPES, 5, 0, wsx.PATTERNS),
    ("appended", dict(fold=True, small=False), "mixed", [APPENDED], 5, 3, wsx.PATTERNS),
    ("default-panel", dict(), "mixed", [(4096, 256)], 5, 3, wsx.PATTERNS),
    ("C3", dict(), "mixed", [(16384, 256)], 4, 0, ("ones", "leftover")),
    ("bf16", dict(dtype=BF16, small=False), "mixed", [(4096, 128), (700, 300)], 5, 3, wsx.PATTERNS),
    ("fp32-mfma", dict(x3=False, small=False), "mixed", [(700, 300), (1153, 128)], 5, 3, wsx.PATTERNS),
    ("one-kernel", dict(), "mixed", [(100, 10), (160, 55)], 5, 0, wsx.PATTERNS),
]
CASES = [(p[0], n, d) for p in PATHS for (n, d) in p[3]]
_PATH = {p[0]: p for p in PATHS}


def _planes(which):
    """The operand images a call leaves, padding included, as test_gpu_conditioning._plane_images reads them (the two fp16
    terms of every tile; fp32 inputs).  A pad row of theta's image only feeds accumulator rows that no epilogue stores, so
    no result can tell whether it was written: the images themselves are held to a fresh engine's.
    "all": the unfolded split path -- theta, theta^T, score^T and the scales.  "w": the folded path -- W's planes only
    (theta^T is deliberately not rebuilt by a plain folded call; theta's row-major image holds K.theta and the row sums
    by the end of the call)."""
    def read(eng):
        imgs, sc, dc = tc._plane_images(eng.planes, eng.n, eng.d)
        if which == "w":
            return dict(Wt3=imgs[2])
        return dict(T3=imgs[0], Tt3=imgs[1], Gt3=imgs[2], scales=sc[:4 * dc + 3])
    return read


def _extra_of(name, kw):
    if name in ("unfolded", "staged"):
        return _planes("all")
    if name.startswith("folded") or name in ("appended", "default-panel", "C3"):
        return _planes("w")
    return None


def _engine(n, d, cuda, kw):
    return SvgdEngine(n, d, device=cuda, **kw)


def _assert_layout_of(name, n, d, eng):
    """what the path's name promises, from the layout, before anything runs: a changed gate must fail here, loudly"""
    X = _lib.FLAG_X3 | _lib.FLAG_TILED
    if name == "appended":
        grown = _lib.workspace_layout(n, n, d, _lib.F32, X | _lib.FLAG_FOLD)
        plain = _lib.workspace_layout(n, n, d, _lib.F32, X | _lib.FLAG_NO_FOLD)
        assert grown[0] > plain[0], "forcing the fold no longer grows this workspace: pick another shape"
        assert grown[1] == plain[1], "the appended storage moved a section"
        assert _lib.layout_folds(n, n, d, _lib.F32, X | _lib.FLAG_FOLD) and not _lib.layout_folds(n, n, d, _lib.F32, X)
        assert eng.fold and eng.ws.numel() == grown[0]
    elif name.startswith("folded"):
        assert eng.fold
        assert eng.ws.numel() == _lib.workspace_layout(n, n, d, _lib.F32, (eng.flags & ~_lib.FLAG_FOLD) | _lib.FLAG_NO_FOLD)[0], \
            "this shape's fold now appends its storage: it belongs to the `appended` path"
    elif name in ("default-panel", "C3"):
        assert eng.fold is True and not eng._one_kernel
    elif name == "one-kernel":
        assert eng._one_kernel
    else:
        assert not eng.fold and not eng._one_kernel


# ---------------------------------------------------------------------------------------------------------------
# (a) poisoned between calls
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,d", CASES, ids=["%s-%dx%d" % c for c in CASES])
def test_poisoned_between_calls(cuda, name, n, d):
    _, kw, variant, _, steps, drift, patterns = _PATH[name]
    dtype = kw.get("dtype", torch.float32)
    eng, twin = _engine(n, d, cuda, kw), _engine(n, d, cuda, kw)
    _assert_layout_of(name, n, d, eng)
    seq = wsx.input_sequence(n, d, seed=n + d, steps=steps, drift=drift)
    seq.append(wsx.input_sequence(n, d, seed=n + d + 1, steps=1)[0])      # the call that finds SELECT poisoned too
    Tu, Gu = (wsx.to_device(x, cuda, dtype) for x in wsx.unrelated_inputs(n, d, n + d))
    left = wsx.leftover_of(lambda: _engine(n, d, cuda, kw), lambda e: wsx.engine_call(e, Tu, Gu, dK=variant in ("dK", "mixed")))
    h2s, extra = [], _extra_of(name, kw)
    for call, (T64, G64) in enumerate(seq):
        T, G = wsx.to_device(T64, cuda, dtype), wsx.to_device(G64, cuda, dtype)
        dK, K = _request(variant, call, n)
        last = call == len(seq) - 1
        pattern = patterns[call % len(patterns)] if not last else "ones"
        tag = "%s %dx%d call %d (%s%s)" % (name, n, d, call, pattern, ", SELECT too" if last else "")
        wsx.poison(eng, pattern, keep_select=not last, leftover=left)
        got = wsx.engine_call(eng, T, G, dK, K, extra=extra)
        want = wsx.fresh_result(n, d, T, G, dK, K, extra=extra, **kw)
        wsx.assert_same(tag, got, want)
        h2s.append(float(want["h2"].item()))
        if name == "one-kernel":        # (stein_small.hip keeps no state at all: the SELECT section is never touched)
            continue
        if not last:
            wsx.engine_call(twin, T, G, dK, K)
            stats = eng.window_stats()
            assert stats == twin.window_stats(), (tag, "poison changed the window's record", stats, twin.window_stats())
        else:       # the predictor starts over, as on a fresh engine: one median recorded, no hit
            assert eng.window_stats() == (1, 0), (tag, eng.window_stats())
    wild = h2s[:steps]
    assert all(max(a, b) > 4.0 * min(a, b) for a, b in zip(wild, wild[1:])), ("the sequence's bandwidths do not move", wild)
    if name != "one-kernel":
        print("%s %dx%d: window record of the twin %s" % (name, n, d, twin.window_stats()))
        if drift and kw.get("window", True) and dtype == torch.float32:
            # the drift steps are there so that "neither costs nor grants a hit" compares something: the median of a
            # cloud that grows by a thousandth per step is what the predictor extrapolates exactly
            assert twin.window_stats()[1] >= 1, "no window hit in the whole sequence"


STAGED = [(1024, 256), (700, 300)]


@pytest.mark.parametrize("n,d", STAGED)
def test_poisoned_between_staged_calls(cuda, n, d):
    """compute_phi(mark=...): the staged calls.  SELECT carries nothing here, so all of the workspace is poisoned always."""
    kw = dict(small=False)
    eng = _engine(n, d, cuda, kw)
    Tu, Gu = (wsx.to_device(x, cuda) for x in wsx.unrelated_inputs(n, d, n + d))
    left = wsx.leftover_of(lambda: _engine(n, d, cuda, kw), lambda e: wsx.engine_call(e, Tu, Gu, dK=True, staged=True))
    for call, (T64, G64) in enumerate(wsx.input_sequence(n, d, seed=n + d, steps=6)):
        T, G = wsx.to_device(T64, cuda), wsx.to_device(G64, cuda)
        dK, K = _request("mixed", call, n)
        pattern = wsx.PATTERNS[call % 4]
        wsx.poison(eng, pattern, keep_select=False, leftover=left)
        got = wsx.engine_call(eng, T, G, dK, K, staged=True, extra=_planes("all"))
        wsx.assert_same("staged %dx%d call %d (%s)" % (n, d, call, pattern), got,
                        wsx.fresh_result(n, d, T, G, dK, K, staged=True, extra=_planes("all"), **kw))


ROW_BLOCKS = [(700, 300, [(0, 300), (300, 400)]), (1281, 129, [(0, 427), (427, 427), (854, 427)])]


@pytest.mark.parametrize("window", [False, True], ids=["radix", "window"])
@pytest.mark.parametrize("n,d,bounds", ROW_BLOCKS, ids=["%dx%d" % c[:2] for c in ROW_BLOCKS])
def test_poisoned_row_blocks(cuda, n, d, bounds, window):
    """n_local < n through stein_rank_begin / _pick / _radix / _finish, every block's workspace poisoned before its
    rank_begin.  Radix form: nothing persists, SELECT is poisoned too.  Window form: SELECT carries the predictor."""
    blocks = wsx.RankBlocks(n, d, bounds, cuda, window)
    twin = wsx.RankBlocks(n, d, bounds, cuda, window)
    Tu, Gu = (wsx.to_device(x, cuda) for x in wsx.unrelated_inputs(n, d, n + d))
    left = wsx.leftover_of(lambda: wsx.RankBlocks(n, d, bounds, cuda, window), lambda b: b.step(Tu, Gu, dK=True))
    for call, (T64, G64) in enumerate(wsx.input_sequence(n, d, seed=n + d, steps=5, drift=3 if window else 0)):
        T, G = wsx.to_device(T64, cuda), wsx.to_device(G64, cuda)
        pattern = wsx.PATTERNS[call % 4]
        tag = "row blocks %dx%d %s call %d (%s)" % (n, d, "window" if window else "radix", call, pattern)
        wsx.poison(blocks, pattern, keep_select=window, leftover=left)
        got = blocks.step(T, G, dK=call % 2 == 1)
        want = wsx.RankBlocks(n, d, bounds, cuda, window).step(T, G, dK=call % 2 == 1)
        wsx.assert_same(tag, got, want)
        if window:
            twin.step(T, G, dK=call % 2 == 1)
            assert blocks.window_stats() == twin.window_stats(), (tag, blocks.window_stats(), twin.window_stats())
    if window:
        print("row blocks %dx%d: window record %s" % (n, d, twin.window_stats()))


# ---------------------------------------------------------------------------------------------------------------
# (b) mixed calls on one workspace
# ---------------------------------------------------------------------------------------------------------------
REQUESTS = [(False, False), (True, False), (False, False), (False, True), (True, True), (False, False)]


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("n,d", [(1024, 256), (700, 300)])
def test_mixed_requests_on_one_engine(cuda, n, d, fold):
    """plain -> dK -> plain -> K -> dK + K -> plain on changing inputs, nothing poisoned: a plain call must not leave
    theta^T planes or PART_T where the next dK call trusts them, nor the reverse"""
    kw = dict(fold=fold, small=False)
    eng = _engine(n, d, cuda, kw)
    assert eng.fold == fold
    for call, (T64, G64) in enumerate(wsx.input_sequence(n, d, seed=3 * n + d, steps=2 * len(REQUESTS))):
        T, G = wsx.to_device(T64, cuda), wsx.to_device(G64, cuda)
        dK, K = REQUESTS[call % len(REQUESTS)]
        got = wsx.engine_call(eng, T, G, dK, K)
        wsx.assert_same("mixed %dx%d fold=%s call %d dK=%s K=%s" % (n, d, fold, call, dK, K), got,
                        wsx.fresh_result(n, d, T, G, dK, K, **kw))


X3T = _lib.FLAG_X3 | _lib.FLAG_TILED
ABI_FLAGS = [_lib.FLAG_FOLD, _lib.FLAG_NO_FOLD, _lib.FLAG_NO_WINDOW, _lib.FLAG_TILE_DISTANCE, 0,
             _lib.FLAG_FOLD | _lib.FLAG_NO_WINDOW, _lib.FLAG_NO_FOLD | _lib.FLAG_TILE_DISTANCE,
             _lib.FLAG_FOLD | _lib.FLAG_TILE_DISTANCE | _lib.FLAG_NO_WINDOW, _lib.FLAG_NO_FOLD | _lib.FLAG_NO_WINDOW,
             _lib.FLAG_FOLD | _lib.FLAG_TILE_DISTANCE]


def _engine_kw_of(flags):
    kw = dict(small=False, window=not flags & _lib.FLAG_NO_WINDOW, tile_distance=bool(flags & _lib.FLAG_TILE_DISTANCE))
    if flags & (_lib.FLAG_FOLD | _lib.FLAG_NO_FOLD):
        kw["fold"] = bool(flags & _lib.FLAG_FOLD)
    return kw


@pytest.mark.parametrize("n,d", [(1024, 256), (700, 300)])
def test_mixed_flags_on_one_workspace_at_the_abi(cuda, n, d):
    """stein_svgd_phi with explicit flags on one workspace sized for the largest request.  (STEIN_FLAG_KSD is left out:
    it moves the sections behind SQPART, and the header says so.)"""
    sets = [X3T | f for f in ABI_FLAGS]
    base = _lib.workspace_layout(n, n, d, _lib.F32, X3T)
    for f in sets:          # (test_workspace_layout.py shows it for a grid of shapes)
        assert _lib.workspace_layout(n, n, d, _lib.F32, f)[1] == base[1], "a flag of the cycle moves a section"
    abi = wsx.AbiCaller(n, d, cuda, sets)
    for call, (T64, G64) in enumerate(wsx.input_sequence(n, d, seed=5 * n + d, steps=len(sets))):
        T, G = wsx.to_device(T64, cuda), wsx.to_device(G64, cuda)
        flags = sets[call]
        dK, K = REQUESTS[call % len(REQUESTS)]
        got = abi.call(T, G, flags, dK, K)
        want = wsx.fresh_result(n, d, T, G, dK, K, **_engine_kw_of(flags))
        wsx.assert_same("abi %dx%d call %d flags 0x%x dK=%s K=%s" % (n, d, call, flags, dK, K), got, want)
        folded = abi.ws[abi._offs[_lib.WS_SELECT] + _lib.FUSE_FOLDED_OFFSET:][:4].view(torch.int32).item()
        assert folded == int(_lib.layout_folds(n, n, d, _lib.F32, flags)), (call, flags, folded)


# ---------------------------------------------------------------------------------------------------------------
# (c) the yardstick itself against fp64
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(n, d, bf16):
    T64, G64 = wsx.input_sequence(n, d, seed=n + d, steps=wsx.FAMILY_STEP + 1)[wsx.FAMILY_STEP]
    if bf16:
        T64, G64 = (tc._np(torch.tensor(x, dtype=torch.float32).to(BF16)) for x in (T64, G64))
    return T64, G64, orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)


ANCHORS = [(p[0], p[1], n, d) for p in PATHS if p[0] in ("unfolded", "folded", "folded-ksd", "bf16", "fp32-mfma", "one-kernel")
           for (n, d) in p[3] if n <= 2048]
ANCHORS += [("staged", dict(small=False), n, d) for (n, d) in STAGED]


@pytest.mark.parametrize("name,kw,n,d", ANCHORS, ids=["%s-%dx%d" % (a[0], a[2], a[3]) for a in ANCHORS])
def test_fresh_result_against_fp64(cuda, name, kw, n, d):
    """fresh_result on the sequence's conditioning_inputs step (graded or zero_const, theta times 2^-2, the score times
    2^7) under test_gpu_conditioning's per-column and bandwidth checks.  bf16 inputs: the bandwidth only -- their phi is
    held per column by test_bf16_inputs_per_column at this shape, against a yardstick this module may not restate."""
    dtype = kw.get("dtype", torch.float32)
    T64, G64, ref = _oracle(n, d, dtype == BF16)
    T, G = wsx.to_device(T64, cuda, dtype), wsx.to_device(G64, cuda, dtype)
    res = wsx.fresh_result(n, d, T, G, dK=True, staged=name == "staged", **kw)
    tag = "fresh %s %dx%d %s" % (name, n, d, wsx.family_of(n, d))
    tc._check_bandwidth(tag, res["h2"], res.get("D"), ref, n)
    assert torch.isfinite(res["phi"]).all() and torch.isfinite(res["dK"]).all() and torch.isfinite(res["sums"]).all(), tag
    if dtype == BF16:
        return
    terms = ref["K"].sum(1)[:, None] / ref["h2"]
    tc._check_columns(tag, tc._np(res["phi"]), ref["phi"], T64, "phi")
    tc._check_columns(tag, tc._np(res["dK"]), ref["dK"], T64, "dK", scale_terms=terms)
    if kw.get("ksd"):
        from test_gpu_ksd import TOL_F32, _errors
        eng = SvgdEngine(n, d, device=cuda, **kw)
        eng.ws.zero_()
        eng.compute_phi(T, G)
        errs, _ = _errors(eng, T, G)
        print("%s: ksd err/scale %s" % (tag, errs))
        assert torch.equal(eng._sums, res["sums"]) and max(errs) <= TOL_F32, errs


def test_appended_storage_against_fp64_rows(cuda):
    """the shape whose forced fold appends its partial sums: sampled rows in fp64 (test_gpu_fold._sampled_fp64) under
    test_gpu_fold.test_folded_against_unfolded's own bound -- twice the unfolded path's error on the same rows, and the
    project's tolerance"""
    n, d = APPENDED
    T64, G64 = wsx.input_sequence(n, d, seed=n + d, steps=1)[0]
    T, G = wsx.to_device(T64, cuda), wsx.to_device(G64, cuda)
    a = wsx.fresh_result(n, d, T, G, fold=True, small=False)
    b = wsx.fresh_result(n, d, T, G, fold=False, small=False)
    assert torch.equal(a["h2"], b["h2"]) and torch.equal(a["D"], b["D"])
    rows = torch.arange(0, n, n // 48, device=cuda)[:48]
    ref = tf._sampled_fp64(T, G, float(a["h2"].item()), rows)
    ea = ((a["phi"][rows].double() - ref).norm() / ref.norm()).item()
    eb = ((b["phi"][rows].double() - ref).norm() / ref.norm()).item()
    print("appended fold %dx%d: against fp64 on 48 rows folded %.3e, unfolded %.3e" % (n, d, ea, eb))
    assert ea <= min(2.0 * eb, tf.TOL), (ea, eb)
