"""GPU: the launches around the folded contraction -- the operand split (k_split, k_split_w: stein_x3.hip), the finish pass
(k_phi_finish: steinhip.hip) and the warm slice of the select launch (k_spec_select: stein_select.hip).  They are scheduling
and data movement only, so everything here is held bit for bit.

1. Planes.  theta and the score are integers / 64 in [-4, 4]: nine significant bits or fewer, so G - theta * (1 / h2) is exact
   in float64 and ONE rounding to float32 is the device's fmaf.  The planes and scales a call leaves in its workspace are
   decoded (tile-major, MFMA fragment order: the header of stein_x3.hip) and compared bit for bit with a NumPy restatement:
   bound from the column maxima -> power-of-two scale -> hi = fp16(x), lo = fp16(x - hi), round to nearest even; zeros in
   the padding.
2. Finish.  The j ranges of the folded contraction are asked for through stein_debug_fold_split.  A range starts on a
   multiple of 128 columns and empty tails are dropped (stein_make_layout), so 256 particles give at most two ranges and
   640 one, two, three or five, never four: the cases 256 x 256 and 640 x 130 at 1, 2, 4 and 3 ranges asked for are run as
   they are and come out as 1, 2, 2, 2 and 1, 2, 3, 3.  d = 130 is no multiple of four, so 640 x 130 runs the finish pass's
   one-entry-at-a-time branch; its four-columns-at-a-time branch, the one that is specialised by range count, gets
   512 x 256 at 4 ranges (the four-range form) and 640 x 256 at 3 and 5 (the loop behind the specialised forms) on top of
   256 x 256 at 1 and 2.  Both the range count that comes out and the branch a case takes are asserted, not assumed.
3. Warm slice.  phi, h2 and |phi|^2 with the slice and without it, on a window hit and on a forced miss.
Run with -s to see the figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import test_gpu_conditioning as tc  # noqa: E402
import test_gpu_x3 as tx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

PLANE_SHAPES = [(192, 130), (256, 256), (320, 257), (1088, 192)]
PEXP = 14


# ---------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------
def _lattice(n, d, seed):
    """theta, score: integers / 64 in [-4, 4] as float64 (exact in float32 and in bf16)"""
    rng = np.random.default_rng(seed + 7919 * n + d)
    return rng.integers(-256, 257, size=(n, d)) / 64.0, rng.integers(-256, 257, size=(n, d)) / 64.0


def _scale_exp(x32, lim):
    """scale_exp of stein_x3.hip on float32 values: s with x * 2^s in [2^13, 2^14); 0 for zero / subnormal / non-finite"""
    e = ((np.asarray(x32, dtype=np.float32).view(np.uint32) >> 23) & 0xff).astype(np.int64)
    return np.where((e == 0) | (e == 255), 0, np.clip(140 - e, -lim, lim))


def _terms(x32):
    """[2, ...] int16: the bits of hi = fp16(x) and lo = fp16(x - hi), round to nearest even"""
    x32 = np.asarray(x32, dtype=np.float32)
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    return np.stack([hi.view(np.int16), lo.view(np.int16)])


def _padded(x, rows, cols):
    out = np.zeros((rows, cols), dtype=x.dtype)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def _expect_transposed(X32, exps, dc, nk):
    """terms of the transposed image of X (rows = columns of X, scaled by 2^exps[c]; k = particles), [2, dc, nk]"""
    scaled = (X32 * np.exp2(exps[:X32.shape[1]]).astype(np.float32)[None, :]).astype(np.float32)
    return _terms(_padded(scaled.T.copy(), dc, nk))


def _decode(img, nrows, nks):
    """[tiles, 2, 4096] int16 in fragment order [row / 16][chunk][row % 16][8] (vfrag_offset) -> [2, nrows, nks]"""
    x = img.view(nrows // 128, nks // 32, 2, 8, 4, 16, 8)              # [rb, kt, term, q, chunk, r, e]
    return x.permute(2, 0, 3, 5, 1, 4, 6).reshape(2, nrows, nks).cpu().numpy()


def _dims(n, d):
    return (n + 127) // 128 * 128 + 128, (d + 31) // 32 * 32, (d + 127) // 128 * 128, (n + 31) // 32 * 32


def _same(tag, got, want):
    bad = got != want
    assert not bad.any(), (tag, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]])


def _check_w(tag, eng, T64, G64):
    """the planes and scales of W = G - theta / h2 that a folded call left behind"""
    n, d = T64.shape
    rows, dk, dc, nk = _dims(n, d)
    imgs, sc, dc_got = tc._plane_images(eng.planes, n, d)
    assert dc_got == dc
    h2 = np.float32(eng.h2.item())
    ih = np.float32(1.0) / h2
    assert np.isfinite(ih) and ih > 0
    W = (G64 - T64 * np.float64(ih)).astype(np.float32)               # exact in float64, one rounding: the device's fmaf
    bound = (np.abs(G64).max(0) + np.abs(T64).max(0) * np.float64(ih)).astype(np.float32)
    se = _padded(_scale_exp(bound, 100)[None, :], 1, dc)[0]
    sc = sc.cpu().numpy()
    _same(tag + " W in-scale", sc[:dc], np.exp2(se).astype(np.float32))
    _same(tag + " W out-scale", sc[2 * dc:3 * dc], np.exp2(-se - PEXP).astype(np.float32))
    _same(tag + " W planes", _decode(imgs[2], dc, nk), _expect_transposed(W, se, dc, nk))


def _check_theta_t(tag, eng, T64):
    n, d = T64.shape
    rows, dk, dc, nk = _dims(n, d)
    imgs, sc, _ = tc._plane_images(eng.planes, n, d)
    T32 = T64.astype(np.float32)
    st = _padded(_scale_exp(np.abs(T32).max(0), 100)[None, :], 1, dc)[0]
    _same(tag + " theta in-scale", sc.cpu().numpy()[dc:2 * dc], np.exp2(st).astype(np.float32))
    _same(tag + " theta^T planes", _decode(imgs[1], dc, nk), _expect_transposed(T32, st, dc, nk))


# ---------------------------------------------------------------------------------------------------------------
# 1. planes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", PLANE_SHAPES)
def test_w_planes_bit_for_bit(cuda, n, d):
    T64, G64 = _lattice(n, d, 0)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    eng = SvgdEngine(n, d, device=cuda, fold=True, small=False)
    assert eng.fold
    for call in range(2):           # radix select, then the window
        eng.compute_phi(T, G)
        torch.cuda.synchronize()
        _check_w("W %dx%d call %d" % (n, d, call), eng, T64, G64)


@pytest.mark.parametrize("n,d", [(192, 130), (320, 257)])
def test_w_and_theta_planes_of_the_dk_and_ksd_calls(cuda, n, d):
    """with dK_out or the statistic the folded call also contracts K with theta: its transposed image comes from k_split"""
    T64, G64 = _lattice(n, d, 1)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    dK = torch.empty(n, d, device=cuda)
    for kw, args in (({}, {"dK_out": dK}), ({"ksd": True}, {})):
        eng = SvgdEngine(n, d, device=cuda, fold=True, small=False, **kw)
        assert eng.fold
        eng.compute_phi(T, G, **args)
        torch.cuda.synchronize()
        tag = "%s %dx%d" % ("ksd" if kw else "dK", n, d)
        _check_w(tag, eng, T64, G64)
        _check_theta_t(tag, eng, T64)


@pytest.mark.parametrize("n,d", [(192, 130), (320, 257)])
def test_unfolded_planes_bit_for_bit(cuda, n, d):
    """k_split on the unfolded path: theta's row-major image (one scale), theta^T and score^T (column scales)"""
    T64, G64 = _lattice(n, d, 2)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    eng = SvgdEngine(n, d, device=cuda, fold=False, small=False)
    assert not eng.fold
    eng.compute_phi(T, G)
    torch.cuda.synchronize()
    rows, dk, dc, nk = _dims(n, d)
    imgs, sc, _ = tc._plane_images(eng.planes, n, d)
    sc = sc.cpu().numpy()
    tag = "unfolded %dx%d" % (n, d)
    T32, G32 = T64.astype(np.float32), G64.astype(np.float32)
    sa = int(_scale_exp(np.abs(T32).max(), 60))
    assert sc[4 * dc] == np.float32(2.0 ** sa) and sc[4 * dc + 1] == np.float32(2.0 ** (1 - 2 * sa))
    _same(tag + " theta planes", _decode(imgs[0], rows, dk), _terms(_padded(T32 * np.float32(2.0 ** sa), rows, dk)))
    _check_theta_t(tag, eng, T64)
    sg = _padded(_scale_exp(np.abs(G32).max(0), 100)[None, :], 1, dc)[0]
    _same(tag + " score in-scale", sc[:dc], np.exp2(sg).astype(np.float32))
    _same(tag + " score^T planes", _decode(imgs[2], dc, nk), _expect_transposed(G32, sg, dc, nk))


def test_bf16_planes_bit_for_bit(cuda):
    """KIND 1: one plane, the bf16 values themselves, no scales"""
    n, d = 192, 130
    T64, G64 = _lattice(n, d, 3)
    T = torch.tensor(T64, dtype=torch.bfloat16, device=cuda)
    G = torch.tensor(G64, dtype=torch.bfloat16, device=cuda)
    assert np.array_equal(T.float().cpu().numpy(), T64) and np.array_equal(G.float().cpu().numpy(), G64)
    eng = SvgdEngine(n, d, device=cuda, dtype=torch.bfloat16, small=False)
    assert not eng.fold
    eng.compute_phi(T, G)
    torch.cuda.synchronize()
    rows, dk, dc, nk = _dims(n, d)
    imgs, sc, _ = tc._plane_images(eng.planes, n, d)
    Tb, Gb = T.view(torch.int16).cpu().numpy(), G.view(torch.int16).cpu().numpy()
    _same("bf16 theta", _decode(imgs[0], rows, dk)[0], _padded(Tb, rows, dk))
    _same("bf16 theta^T", _decode(imgs[1], dc, nk)[0], _padded(Tb.T.copy(), dc, nk))
    _same("bf16 score^T", _decode(imgs[2], dc, nk)[0], _padded(Gb.T.copy(), dc, nk))


# ---------------------------------------------------------------------------------------------------------------
# 2. finish
# ---------------------------------------------------------------------------------------------------------------
def _ranges_from_plan(n, asked):
    """the rule of stein_make_layout for `asked` ranges: whole 128-column groups per range, empty tails dropped"""
    jt = (n + 31) // 32
    split = min(asked, jt)
    per = ((jt + split - 1) // split + 3) // 4 * 4
    return (jt + per - 1) // per


FINISH_CASES = [(n, d, k) for (n, d) in ((256, 256), (640, 130)) for k in (1, 2, 4, 3)] + [(512, 256, 4), (640, 130, 5), (640, 256, 3), (640, 256, 5)]
# what the plan makes of each case, and which branch of the finish pass the shape takes (True: four columns at a time)
FINISH_RANGES = {(256, 256, 1): 1, (256, 256, 2): 2, (256, 256, 4): 2, (256, 256, 3): 2, (640, 130, 1): 1, (640, 130, 2): 2,
                 (640, 130, 4): 3, (640, 130, 3): 3, (512, 256, 4): 4, (640, 130, 5): 5, (640, 256, 3): 3, (640, 256, 5): 5}
FINISH_VECTOR = {(256, 256): True, (640, 130): False, (512, 256): True, (640, 256): True}
_finish_refs = {}


def _finish_ref(n, d):
    if (n, d) not in _finish_refs:
        T64, G64 = tx._inputs(n, d)
        T64, G64 = ci.f32(T64), ci.f32(G64)
        _finish_refs[(n, d)] = (T64, G64, orc.svgd_step(T64, G64, orc.AdagradState(), np.float64))
    return _finish_refs[(n, d)]


@pytest.mark.parametrize("n,d,asked", FINISH_CASES, ids=["%dx%d-ask%d" % c for c in FINISH_CASES])
def test_finish_at_every_range_count(cuda, n, d, asked):
    T64, G64, ref = _finish_ref(n, d)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    tag = "finish %dx%d asked %d" % (n, d, asked)
    terms = ref["K"].sum(1)[:, None] / ref["h2"]
    try:
        _lib.debug_fold_split(asked)                # the workspace is sized under the hook, and the calls run under it
        plain = SvgdEngine(n, d, device=cuda, fold=True, small=False)
        withdk = SvgdEngine(n, d, device=cuda, fold=True, small=False)
        assert plain.fold and withdk.fold
        got = _lib.layout_fold_ranges(n, n, d, _lib.F32, plain.flags)
        print("%s: %d ranges" % (tag, got))
        assert got == _ranges_from_plan(n, asked) == FINISH_RANGES[(n, d, asked)], tag
        dK = torch.full((n, d), float("nan"), device=cuda)
        # the branch: four columns at a time needs d % 4 == 0 and 16-byte aligned buffers (finish_stage, steinhip.hip)
        vec = d % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (T, dK, plain.phi, plain.ws, withdk.phi, withdk.ws))
        assert vec == FINISH_VECTOR[(n, d)], tag
        for call in range(2):
            p0 = plain.compute_phi(T, G).clone()
            h0, s0 = plain.h2.clone(), plain.sqnorm.clone()
            p0b = plain.compute_phi(T, G).clone()
            p1 = withdk.compute_phi(T, G, dK_out=dK).clone()
            torch.cuda.synchronize()
            assert torch.equal(p0, p0b) and torch.equal(h0, plain.h2) and torch.equal(s0, plain.sqnorm), tag
            assert torch.equal(p0, p1) and torch.equal(h0, withdk.h2) and torch.equal(s0, withdk.sqnorm), tag
            tc._check_columns(tag, tc._np(p0), ref["phi"], T64, "phi")
            tc._check_columns(tag, tc._np(dK), ref["dK"], T64, "dK", scale_terms=terms)
            assert abs(s0.item() - ref["sqnorm"]) <= 2e-5 * ref["sqnorm"], tag
    finally:
        _lib.debug_fold_split(0)


def test_finish_range_counts_that_come_out():
    """what the header of this module says about the cases (host arithmetic; runs with the GPU tests because it explains them)"""
    flags = _lib.FLAG_X3 | _lib.FLAG_FOLD | _lib.FLAG_TILED
    try:
        out = {}
        for n, d, k in FINISH_CASES:
            _lib.debug_fold_split(k)
            out[(n, d, k)] = _lib.layout_fold_ranges(n, n, d, _lib.F32, flags)
    finally:
        _lib.debug_fold_split(0)
    assert out == FINISH_RANGES
    # every form of the four-columns-at-a-time branch is run by a case that takes it: 1, 2, 4 ranges and the loop (3, 5)
    assert {r for (n, d, k), r in out.items() if FINISH_VECTOR[(n, d)]} >= {1, 2, 3, 4, 5}
    assert _lib.layout_fold_ranges(16384, 16384, 256, _lib.F32, _lib.FLAG_X3) == 2     # the flagship shape: the two-range form


# ---------------------------------------------------------------------------------------------------------------
# 3. warm slice
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [True, False], ids=["hit", "miss"])
@pytest.mark.parametrize("n,d", [(256, 256), (4096, 256)])
def test_warm_slice_changes_nothing(cuda, n, d, window):
    """the extra workgroups of the select launch only read: with them and without them every output is the same to the bit.
    window=False: no window, the median comes from the radix passes on every call (the miss path)."""
    gen = torch.Generator(device="cpu").manual_seed(11)
    T = torch.randn(n, d, generator=gen).to(cuda)
    G = torch.randn(n, d, generator=gen).to(cuda)
    outs = []
    try:
        for off in (True, False):
            _lib.debug_no_warm(off)
            eng = SvgdEngine(n, d, device=cuda, fold=True, small=False, window=window)
            assert eng.fold
            res = []
            for call in range(3):
                phi = eng.compute_phi(T, G).clone()
                res.append((phi, eng.h2.clone(), eng.sqnorm.clone()))
            if window:
                assert eng.window_stats()[1] >= 1, "no call of the three hit the window"
            else:
                assert eng.window_stats()[1] == 0, "window=False, yet a median came from the window"
            outs.append(res)
    finally:
        _lib.debug_no_warm(False)
    torch.cuda.synchronize()
    for call, (a, b) in enumerate(zip(*outs)):
        assert torch.isfinite(a[0]).all()
        for x, y, what in zip(a, b, ("phi", "h2", "sqnorm")):
            assert torch.equal(x, y), (n, d, window, call, what)
