"""CPU: stein_workspace_layout over a seeded grid of (n_local, n, d, dtype, flags) -- host arithmetic, no GPU.

What tests/test_gpu_workspace_state.py relies on, and what include/steinhip.h says of the sections: 256-byte aligned, in
order, each as large as the header documents, the total behind the last; the fold, window, distance and timing flags move
nothing; the default gate never grows a workspace; where a forced fold does (it appends its partial sums to PLANES), the
default leaves the call unfolded."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import workspace_state as wsx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402

X3, TILED, KSD = _lib.FLAG_X3, _lib.FLAG_TILED, _lib.FLAG_KSD
FOLD, NO_FOLD = _lib.FLAG_FOLD, _lib.FLAG_NO_FOLD
NEUTRAL = [FOLD, NO_FOLD, _lib.FLAG_NO_WINDOW, _lib.FLAG_TILE_DISTANCE, _lib.FLAG_TIMING,
           _lib.FLAG_TIMING | _lib.FLAG_TIMING_CONTRACT, FOLD | _lib.FLAG_NO_WINDOW | _lib.FLAG_TILE_DISTANCE,
           NO_FOLD | _lib.FLAG_TILE_DISTANCE | _lib.FLAG_TIMING]
# shapes the issue of the fold names: the gate's own (C3, C4, the panel's first), its ragged test shapes, and the family
# whose fold does not fit the storage it reuses
NAMED = [(16384, 256), (8192, 2001), (4096, 256), (8192, 256), (2048, 256), (3072, 521), (3072, 638), (5120, 257),
         (5120, 384), (700, 300), (1281, 129), (1279, 257), (385, 1), (640, 2001), (1536, 130), (100, 10), (160, 55)]


def _grid():
    rng = np.random.default_rng(20240917)
    cases = [(n, n, d, _lib.F32, X3) for n, d in NAMED] + [(n, n, d, _lib.F32, X3 | TILED) for n, d in NAMED]
    while len(cases) < 480:
        n = int(2 ** rng.uniform(1, 14.3))
        d = int(2 ** rng.uniform(0, 11.1))
        kind = rng.integers(4)
        n_local = n if kind < 2 else (max(1, n // int(rng.integers(2, 9))) if kind == 2 else int(rng.integers(1, n + 1)))
        dtype = _lib.BF16 if rng.integers(4) == 0 else _lib.F32
        flags = (X3 if dtype == _lib.BF16 or rng.integers(4) else 0) | (TILED if rng.integers(2) else 0) | (KSD if rng.integers(3) == 0 else 0)
        cases.append((n_local, max(n, 2), d, dtype, flags))
    return [(min(nl, n), n, d, dt, f) for nl, n, d, dt, f in cases]


GRID = _grid()


def _up(x, a):
    return (x + a - 1) // a * a


def _documented_sizes(n_local, n, d, flags, extra):
    """bytes of every section but SPEC as include/steinhip.h documents them (PLANES: the operand images of stein_x3.hip's
    header, as test_gpu_conditioning._plane_images reads them)"""
    ld, split, sqb = extra[_lib.WSX_LD_DIST], extra[_lib.WSX_SPLIT], extra[_lib.WSX_SQ_BLOCKS]
    rows, dk, dc, nk = _up(n, 128) + 128, _up(d, 32), _up(d, 128), _up(n, 32)
    return {
        _lib.WS_ROWNORM: n * 4,
        _lib.WS_DIST: _up(n_local, 128) * ld * 4,
        _lib.WS_HIST: _lib.HIST_LEVELS * 2 * _lib.HIST_BINS * 8,
        _lib.WS_SELECT: _lib.SELECT_BYTES,
        _lib.WS_PART_G: split * n_local * d * 4,
        _lib.WS_PART_T: split * n_local * d * 4,
        _lib.WS_PART_RS: split * n_local * 4,
        _lib.WS_SQPART: max(sqb, (d + 31) // 32) * 8 * (3 if flags & KSD else 1),
        _lib.WS_PLANES: (_up(3 * rows * dk * 2, 256) + 2 * _up(3 * dc * nk * 2, 256) + (4 * dc + 4) * 4) if flags & X3 else 0,
    }


def test_grid_is_large_enough():
    assert len(GRID) >= 300 and len(set(GRID)) >= 300
    assert any(nl < n for nl, n, *_ in GRID) and any(dt == _lib.BF16 for *_, dt, _f in GRID) and any(f & KSD for *_, f in GRID)


def test_sections_are_aligned_ordered_and_large_enough():
    for nl, n, d, dt, f in GRID:
        total, offs, extra = _lib.workspace_layout(nl, n, d, dt, f)
        case = (nl, n, d, dt, f)
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and total % 256 == 0, case
        assert extra[_lib.WSX_LD_DIST] >= n and extra[_lib.WSX_LD_DIST] % 64 == 0 and extra[_lib.WSX_SPLIT] >= 1, case
        ends = offs[1:] + [total]
        sizes = _documented_sizes(nl, n, d, f, extra)
        for sec in range(_lib.WS_NSECTIONS):
            assert ends[sec] >= offs[sec], (case, sec, "sections out of order")
            if sec != _lib.WS_SPEC:
                assert ends[sec] - offs[sec] >= sizes[sec], (case, sec, "section overlaps the next", ends[sec] - offs[sec], sizes[sec])
        spec = ends[_lib.WS_SPEC] - offs[_lib.WS_SPEC]      # empty (the one-kernel path), or entries + slots + the table
        assert spec == 0 or spec >= 8 * (_lib.SPEC_TABLE_OFFSET_WORDS + _lib.SPEC_TABLE_WORDS), (case, spec)
        if spec == 0:
            assert nl == n <= 160 and not f & TILED, case
        assert total >= offs[_lib.WS_PLANES] + sizes[_lib.WS_PLANES], case


def test_fold_window_distance_and_timing_flags_move_nothing():
    for nl, n, d, dt, f in GRID:
        total, offs, extra = _lib.workspace_layout(nl, n, d, dt, f)
        for extra_flags in NEUTRAL:
            t2, o2, e2 = _lib.workspace_layout(nl, n, d, dt, f | extra_flags)
            assert o2 == offs and e2 == extra, ((nl, n, d, dt, f), extra_flags, "a section moved")
            if not extra_flags & FOLD:
                assert t2 == total, ((nl, n, d, dt, f), extra_flags, "the workspace changed size")
            else:
                assert t2 >= total


def test_default_gate_never_grows_a_workspace():
    grows = 0
    for nl, n, d, dt, f in GRID:
        case = (nl, n, d, dt, f)
        default = _lib.workspace_layout(nl, n, d, dt, f)[0]
        never = _lib.workspace_layout(nl, n, d, dt, f | NO_FOLD)[0]
        forced = _lib.workspace_layout(nl, n, d, dt, f | FOLD)[0]
        assert default == never, case
        assert not _lib.layout_folds(nl, n, d, dt, f | NO_FOLD), case
        if forced > never:
            grows += 1
            assert not _lib.layout_folds(nl, n, d, dt, f), (case, "the default gate folds where the fold needs appended storage")
            assert _lib.layout_folds(nl, n, d, dt, f | FOLD), case
        if _lib.layout_folds(nl, n, d, dt, f | FOLD):       # eligible: split path, fp32 inputs, every row, not one kernel
            assert f & X3 and dt == _lib.F32 and nl == n, case
    assert grows >= 4


def test_grid_holds_both_branches_at_the_sizes_the_gate_is_about():
    """at least one growing and one non-growing shape with n^2 d >= 4e9 and d > 128 (where the default gate would fold)"""
    big = [(nl, n, d, dt, f) for nl, n, d, dt, f in GRID if nl == n and dt == _lib.F32 and f & X3 and not f & KSD
           and n * n * d >= 4e9 and d > 128]
    growing = [c for c in big if _lib.workspace_layout(*c[:4], c[4] | FOLD)[0] > _lib.workspace_layout(*c[:4], c[4] | NO_FOLD)[0]]
    fitting = [c for c in big if c not in growing]
    assert growing and fitting, (len(growing), len(fitting))
    assert all(not _lib.layout_folds(*c) for c in growing)
    assert any(_lib.layout_folds(*c) for c in fitting)
    assert (3072, 3072, 521, _lib.F32, X3 | TILED) in growing       # the shape test_gpu_workspace_state.py runs


# ---- the helpers of the state tests (tests/workspace_state.py) ----------------------------------------------------
def test_no_poison_pattern_can_forge_the_predictor_magic():
    m1, m2 = wsx.spec_magic_words()
    assert m1 != m2 and 0 < m1 < 2 ** 32 and 0 < m2 < 2 ** 32
    for name, byte in wsx.PATTERN_BYTES.items():
        assert not wsx.pattern_can_forge_magic(byte), name


def test_input_sequence_moves_the_bandwidth():
    """neighbouring steps differ in values and in scale: h2 by more than a factor of four (fp64 oracle, two small shapes)"""
    for n, d in ((97, 1), (120, 7), (131, 12)):
        seq = wsx.input_sequence(n, d, seed=n + d, steps=6, drift=2)
        h2 = [float(orc.bandwidth_sq(orc.median_all(orc.pairwise_sq_dists(T, np.float64)), n, np.float64)) for T, _ in seq]
        assert all(max(a, b) > 4.0 * min(a, b) for a, b in zip(h2[:6], h2[1:6])), h2
        assert all(0.0 < b / a - 1.0 < 0.01 for a, b in zip(h2[5:], h2[6:])), h2       # the drift steps: a smooth median
        for (T, G), (T2, G2) in zip(seq, seq[1:]):
            assert not np.array_equal(G, G2) and np.array_equal(ci.f32(T2), T2) and np.array_equal(ci.f32(G2), G2)
    assert wsx.family_of(385, 1) == "graded" and {wsx.family_of(700, 300), wsx.family_of(640, 2001)} == {"graded", "zero_const"}
