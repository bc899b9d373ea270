"""GPU: the folded step that is asked for phi alone has no k_colmax launch.  max|theta| comes from the prologue (one word per
workgroup, reduced by k_split to the scale of theta's row-major planes), the column maxima from the slice of the select
launch (k_spec_select: the body of k_colmax in its 16-byte and 4-byte forms), theta's column scales from k_split_w.  After
a call the scales area and the maxima must hold what the k_colmax launch used to leave there, entry for entry.

Inputs are integers / 64 (test_gpu_glue._lattice), so every expected value below is exact and every comparison is bit for
bit; the restatements are test_gpu_glue's (_scale_exp, _terms, _check_w, _check_theta_t).

Two things the shapes of this module cannot do as one might expect:
  * theta's row-major image T3 is dead behind the distance pass, and the folded contraction parks its row sums inside it
    (stein_make_layout: fold_rs).  The image is compared outside those bytes, which are located from the layout's own rule.
  * rows are dealt to the waves so that every wave takes a whole number of rounds of four where n allows it: with the slice
    (16 rows per round of a row group) and with the fallback kernel alike, 320 and 1088 rows leave nothing to the remainder
    loops.  REMAINDER_SHAPES add 330 and 1100 rows, where both have rows that only their remainder loops reach
    (_remainder_rows restates which); on the exact shapes the third planted maximum sits in a middle row.
Run with -s to see the figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_conditioning as tc  # noqa: E402
import test_gpu_glue as tg  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

PEXP = 14
SLICE_WGS = 255
# 4-byte forms with ragged n; the 16-byte form at n <= the solo limit; 1088 x 192; and a shape whose n d is more than 255 slice
# workgroups cover in one round of loads (four column blocks, 528 slots of 16 rows over 44 row groups: three rounds of four)
SHAPES = [(192, 130), (320, 257), (256, 256), (1088, 192), (8448, 1024)]
PLANT_SHAPES = [(320, 257), (1088, 192)]
REMAINDER_SHAPES = [(330, 257), (1100, 192)]


def _bits(x32):
    return np.asarray(x32, dtype=np.float32).view(np.uint32)


def _areas(eng):
    """(operand images, float32 scales area [4 dc + 4], uint32 column maxima [2 dc] = [score | theta], dc)"""
    n, d = eng.n, eng.d
    imgs, sc, dc = tc._plane_images(eng.planes, n, d)
    rows, dk, _, nk = tg._dims(n, d)
    a256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    off_sc = a256(3 * rows * dk * 2) + 2 * a256(3 * dc * nk * 2)
    at = off_sc + (4 * dc + 4) * 4
    cmax = eng.planes[at:at + 2 * dc * 4].view(torch.int32).cpu().numpy().view(np.uint32)
    return imgs, sc.cpu().numpy(), cmax, dc


def _t3_live(eng):
    """decoded mask [2, rows, dk] of theta's row-major image: False where the folded contraction's row sums were parked.
    Rule of stein_make_layout: K.theta's storage (n d floats, rounded up to 256 bytes) starts the image, the row sums
    (ranges x n floats) follow -- unless the fold's storage was appended behind the planes (the workspace then grew)."""
    n, d = eng.n, eng.d
    rows, dk, _, _ = tg._dims(n, d)
    raw = torch.zeros(3 * rows * dk, dtype=torch.int16)
    grown = _lib.workspace_layout(n, n, d, _lib.F32, eng.flags)[0] > _lib.workspace_layout(
        n, n, d, _lib.F32, (eng.flags & ~_lib.FLAG_FOLD) | _lib.FLAG_NO_FOLD)[0]
    if not grown:
        ot = (n * d * 4 + 255) // 256 * 256
        rs = _lib.layout_fold_ranges(n, n, d, _lib.F32, eng.flags) * n * 4
        assert ot + rs <= raw.numel() * 2
        raw[ot // 2:(ot + rs + 1) // 2] = 1
    parked = tg._decode(raw.view(-1, 3, 4096)[:, :2].clone(), rows, dk)
    assert int(parked.sum()) * 20 < parked.size, "the row sums cover more than a twentieth of the image: nothing would be checked"
    return parked == 0


def _check_all(tag, eng, T64, G64):
    """everything a plain folded call leaves behind: maxima, theta's scales, the three global entries, T3, W"""
    n, d = T64.shape
    rows, dk, dc, nk = tg._dims(n, d)
    imgs, sc, cmax, dc_got = _areas(eng)
    assert dc_got == dc
    T32, G32 = T64.astype(np.float32), G64.astype(np.float32)
    mg = tg._padded(np.abs(G32).max(0)[None, :], 1, dc)[0]
    mt = tg._padded(np.abs(T32).max(0)[None, :], 1, dc)[0]
    tg._same(tag + " max|G|", cmax[:dc], _bits(mg))
    tg._same(tag + " max|theta|", cmax[dc:], _bits(mt))
    st = tg._scale_exp(mt, 100)
    tg._same(tag + " theta in-scale", sc[dc:2 * dc], np.exp2(st).astype(np.float32))
    tg._same(tag + " theta out-scale", sc[3 * dc:4 * dc], np.exp2(-st - PEXP).astype(np.float32))
    sa = int(tg._scale_exp(np.abs(T32).max(), 60))
    want = np.array([2.0 ** sa, 2.0 ** (1 - 2 * sa), 2.0 ** -PEXP], dtype=np.float32)
    tg._same(tag + " sc[4dc + 0..2]", sc[4 * dc:4 * dc + 3], want)
    live = _t3_live(eng)
    got = tg._decode(imgs[0], rows, dk)
    exp = tg._terms(tg._padded(T32 * np.float32(2.0 ** sa), rows, dk))
    tg._same(tag + " theta planes", np.where(live, got, 0), np.where(live, exp, 0))
    tg._check_w(tag, eng, T64, G64)
    print("%s: sa %d, %d of %d T3 entries compared" % (tag, sa, int(live.sum()), live.size))


def _run_and_check(tag, cuda, T64, G64):
    n, d = T64.shape
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    eng = SvgdEngine(n, d, device=cuda, fold=True, small=False)
    assert eng.fold
    for call in range(2):           # radix select, then the window
        eng.compute_phi(T, G)
        torch.cuda.synchronize()
        _check_all("%s call %d" % (tag, call), eng, T64, G64)


# ---------------------------------------------------------------------------------------------------------------
# 1. the scales area and the maxima after a plain folded call
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES)
def test_scales_and_maxima_bit_for_bit(cuda, n, d):
    T64, G64 = tg._lattice(n, d, 4)
    _run_and_check("prepare %dx%d" % (n, d), cuda, T64, G64)


# ---------------------------------------------------------------------------------------------------------------
# 2. where a maximum hides
# ---------------------------------------------------------------------------------------------------------------
def _remainder_rows(n, d):
    """rows only the remainder loops read, (in the select launch's slice, in the k_colmax launch of the fallback): restated
    from stein_fused_select / launch_colmax.  A wave's rows are first, first + step, ...; those past the last whole four."""
    v4 = d % 4 == 0
    out = []
    for slice_form in (True, False):
        if slice_form:
            blocks, slots = -(-d // (256 if v4 else 64)), -(-n // 16)
            max_rg = max(SLICE_WGS // blocks, 1)
            rounds = -(-slots // (4 * max_rg))
            waves, groups = 16, -(-slots // (4 * rounds))
        else:
            waves, groups = (16, min(-(-n // 64), 64)) if v4 else (4, min(-(-n // 64), 256))
        step = waves * groups
        rem = set()
        for first in range(min(step, n)):
            mine = list(range(first, n, step))
            rem.update(mine[len(mine) // 4 * 4:])
        out.append(rem)
    return out


def _planted(n, d, seed):
    """lattice inputs with the unique largest |value| of a column, negative, in row 0, in the last row, in a row the remainder
    loops reach -- the slice's and the fallback kernel's, a column each; middle rows where there are none -- and in the last
    column; an all-zero column; a column of subnormals"""
    T64, G64 = tg._lattice(n, d, seed)
    in_slice, in_kernel = (sorted(rows) for rows in _remainder_rows(n, d))
    mid_slice = in_slice[len(in_slice) // 2] if in_slice else n // 2 + 1
    mid_kernel = in_kernel[len(in_kernel) // 2] if in_kernel else n // 2 + 18
    spots = [(0, 3), (n - 1, 70), (mid_slice, 129), (mid_kernel, 101), (n // 3, d - 1)]
    for k, (row, col) in enumerate(spots):
        T64[row, col] = -(5.0 + k)          # the lattice stops at 4
        G64[(row + 7) % n, col] = -(6.5 + k)
    T64[:, 11] = 0.0
    G64[:, 11] = 0.0
    sub = np.arange(1, n + 1, dtype=np.float64) % 8 + 1
    T64[:, 40] = sub * 2.0 ** -140          # subnormal in float32: scale_exp gives 0
    G64[:, 40] = sub[::-1] * 2.0 ** -141
    assert np.array_equal(T64.astype(np.float32).astype(np.float64), T64)
    assert np.array_equal(G64.astype(np.float32).astype(np.float64), G64)
    return T64, G64, bool(in_slice) and bool(in_kernel)


@pytest.mark.parametrize("n,d", PLANT_SHAPES + REMAINDER_SHAPES)
def test_a_maximum_hides_nowhere(cuda, n, d):
    T64, G64, has_remainder = _planted(n, d, 5)
    assert has_remainder == ((n, d) in REMAINDER_SHAPES), "the row split changed: see the header of this module"
    T32 = T64.astype(np.float32)
    assert tg._scale_exp(np.abs(T32).max(0), 100)[40] == 0 and np.abs(T32[:, 40]).max() > 0
    _run_and_check("planted %dx%d" % (n, d), cuda, T64, G64)


# ---------------------------------------------------------------------------------------------------------------
# 3. nothing carried over
# ---------------------------------------------------------------------------------------------------------------
def _state(eng, T, G):
    phi = eng.compute_phi(T, G).clone()
    torch.cuda.synchronize()
    imgs, sc, cmax, dc = _areas(eng)
    return dict(phi=phi, h2=eng.h2.clone(), sqnorm=eng.sqnorm.clone(), T3=imgs[0], W=imgs[2],
                scales=torch.from_numpy(sc[:4 * dc + 3].copy()), cmax=torch.from_numpy(cmax.astype(np.int64)))


def _equal_states(tag, got, want):
    for key in want:
        assert torch.equal(got[key].cpu(), want[key].cpu()), (tag, key)


@pytest.mark.parametrize("n,d", [(320, 257), (1088, 192)])
def test_nothing_carried_over(cuda, n, d):
    """a call after one on theta * 1024 (every maximum and scale of it larger), then after 0xFF and random bytes all over the
    workspace: the scales area, T3, W and the outputs are a fresh engine's"""
    T64, G64 = tg._lattice(n, d, 6)
    T, G, Tbig = tc._dev(T64, cuda), tc._dev(G64, cuda), tc._dev(T64 * 1024.0, cuda)
    fresh = _state(SvgdEngine(n, d, device=cuda, fold=True, small=False), T, G)
    eng = SvgdEngine(n, d, device=cuda, fold=True, small=False)
    assert eng.fold
    big = _state(eng, Tbig, G)
    assert not torch.equal(big["scales"], fresh["scales"]) and not torch.equal(big["cmax"], fresh["cmax"])
    _equal_states("after theta * 1024", _state(eng, T, G), fresh)
    gen = torch.Generator(device="cpu").manual_seed(n + d)
    for what in ("0xFF", "random"):
        if what == "0xFF":
            eng.ws.fill_(0xFF)
        else:
            eng.ws.copy_(torch.randint(0, 256, (eng.ws.numel(),), dtype=torch.uint8, generator=gen))
        _equal_states("after " + what, _state(eng, T, G), fresh)


# ---------------------------------------------------------------------------------------------------------------
# 4. forms and fallbacks agree
# ---------------------------------------------------------------------------------------------------------------
def _offset_by_4_bytes(x):
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("window", [True, False], ids=["hit", "miss"])
@pytest.mark.parametrize("n,d", [(256, 256), (1088, 192)])
def test_forms_and_fallback_agree(cuda, n, d, window):
    """16-byte forms (aligned tensors), 4-byte forms (the same values 4 bytes into a larger buffer) and the k_colmax launch of
    the fallback (stein_debug_no_warm): the same bits everywhere"""
    T64, G64 = tg._lattice(n, d, 7)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    assert T.data_ptr() % 16 == 0 and G.data_ptr() % 16 == 0
    T4, G4 = _offset_by_4_bytes(T), _offset_by_4_bytes(G)
    runs = {}
    try:
        for name, (a, b, off) in (("16-byte", (T, G, False)), ("4-byte", (T4, G4, False)), ("no slice", (T, G, True))):
            _lib.debug_no_warm(off)
            eng = SvgdEngine(n, d, device=cuda, fold=True, small=False, window=window)
            assert eng.fold
            runs[name] = [_state(eng, a, b) for call in range(3)]
            hits = eng.window_stats()[1]
            print("%dx%d %s window=%s: %d hits" % (n, d, name, window, hits))
            assert (hits >= 1) if window else (hits == 0), (name, hits)
    finally:
        _lib.debug_no_warm(False)
    for name in ("4-byte", "no slice"):
        for call, (got, want) in enumerate(zip(runs[name], runs["16-byte"])):
            assert torch.isfinite(got["phi"]).all()
            _equal_states("%s call %d" % (name, call), got, want)
    _check_all("forms %dx%d" % (n, d), eng, T64, G64)   # (the last engine: the fallback's leftovers against the restatement)


# ---------------------------------------------------------------------------------------------------------------
# 5. the other paths did not move
# ---------------------------------------------------------------------------------------------------------------
def test_dk_call_still_builds_theta_t_from_scales_in_place(cuda):
    """with dK_out the step keeps its k_colmax launch: theta's scales are there before k_split builds theta^T"""
    n, d = 192, 130
    T64, G64 = tg._lattice(n, d, 8)
    T, G = tc._dev(T64, cuda), tc._dev(G64, cuda)
    eng = SvgdEngine(n, d, device=cuda, fold=True, small=False)
    assert eng.fold
    dK = torch.empty(n, d, device=cuda)
    for call in range(2):
        eng.compute_phi(T, G, dK_out=dK)
        torch.cuda.synchronize()
        tg._check_theta_t("dK %dx%d call %d" % (n, d, call), eng, T64)
        tg._check_w("dK %dx%d call %d" % (n, d, call), eng, T64, G64)
