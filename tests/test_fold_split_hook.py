"""CPU: stein_debug_fold_split, the test hook that asks the folded contraction's plan for a number of j ranges (host
arithmetic of stein_make_layout; tests/test_gpu_glue.py runs the finish pass at the range counts it yields)."""
import pytest

from stein_amd import _lib

FOLD = _lib.FLAG_X3 | _lib.FLAG_FOLD | _lib.FLAG_TILED


def test_hook_moves_ranges_and_workspace_together_and_resets():
    n, d = 1024, 256           # 32 j tiles of 32 columns: ranges of 4, 8, ... tiles
    natural = _lib.layout_fold_ranges(n, n, d, _lib.F32, FOLD)
    natural_bytes = _lib.workspace_layout(n, n, d, _lib.F32, FOLD)[0]
    try:
        for asked, want in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 4), (8, 8), (1000, 8)):
            _lib.debug_fold_split(asked)
            assert _lib.layout_fold_ranges(n, n, d, _lib.F32, FOLD) == want, asked
            assert _lib.layout_folds(n, n, d, _lib.F32, FOLD)
            # the partial sums of every range fit: K.W takes 4 n d bytes per range
            assert _lib.workspace_layout(n, n, d, _lib.F32, FOLD)[0] >= want * n * d * 4
        # the hook is about the folded plan only: the unfolded sections and the default gate do not move
        _lib.debug_fold_split(8)
        assert _lib.layout_fold_ranges(n, n, d, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_NO_FOLD) == 0
        a = _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_NO_FOLD)
    finally:
        _lib.debug_fold_split(0)
    assert a == _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_NO_FOLD)
    assert _lib.layout_fold_ranges(n, n, d, _lib.F32, FOLD) == natural
    assert _lib.workspace_layout(n, n, d, _lib.F32, FOLD)[0] == natural_bytes
    assert _lib.layout_fold_ranges(16384, 16384, 256, _lib.F32, _lib.FLAG_X3) == 2
    with pytest.raises(ValueError):
        _lib.debug_fold_split(-1)


def test_warm_hook_takes_zero_or_one():
    _lib.debug_no_warm(True)
    _lib.debug_no_warm(False)
    with pytest.raises(ValueError):
        _lib.call("stein_debug_no_warm", 2)
