"""GPU: the staged radix select (k_hist<LEVEL, SYM> + k_resolve, stein_select.hip) on distance images written by hand.

stein_median_hist_pass takes the distance image as an argument, so any multiset can be put in front of it: the images of
tests/select_inputs.py -- adjacent floats either side of a bin edge of every radix level, negatives with both zeros,
denormals to +inf, three-valued ties with the targets at the first / an interior / the last entry of a tie -- as ragged
rectangular row blocks, as symmetric matrices of which only col >= row is stored (weight 2, diagonal weight 1), and as two
row blocks accumulated into one histogram.  Everything the pass must not read (padding, the part below the diagonal)
holds a sentinel, and every case runs with two of them:

    "low"   the NaN with the sign bit set (0xffc00000): its key 0x003fffff lies BELOW every value's, -inf included, so every
            sentinel a pass counts pushes the targets down by its weight.  The adjacent* images hold exactly half the weight
            at or below lo: one stray count makes hi = lo (test_select_inputs.py asserts that on the CPU).  This is the
            sentinel that catches a pass reading a padded row or column or the lower triangle.
    "nan"   the positive NaN (0x7fc00000), key above every value's: counted, it lands behind both targets and cannot move
            them; what it would show is a NaN leaking into lo, hi or the histogram walk.

lo, hi, the median and the bandwidth must equal an exact NumPy sort's, to the bit."""
import numpy as np
import pytest
import torch

import select_inputs as si
from stein_amd import _lib
from stein_amd.engine import HipStages, tile_distances

pytestmark = pytest.mark.gpu


SENTINELS = {"low": 0xffc00000 - (1 << 32), "nan": 0x7fc00000}      # int32 bit patterns
BOTH = pytest.mark.parametrize("sentinel", list(SENTINELS))


def _tiled(M, device, sym, sentinel):
    """row-major fp32 [rows, cols] -> (tile-major device image, ld): the sentinel's bit pattern in the padding and, sym, below
    the diagonal (written and moved as int32, so that no copy can canonicalise the NaN)"""
    rows, cols = M.shape
    ld = (cols + 63) // 64 * 64
    rp = (rows + 127) // 128 * 128
    full = torch.full((rp, ld), SENTINELS[sentinel], dtype=torch.int32)
    full[:rows, :cols] = torch.from_numpy(np.ascontiguousarray(M).view(np.int32))
    if sym:
        r, c = torch.tril_indices(rows, cols, -1)
        full[r, c] = SENTINELS[sentinel]
    image = tile_distances(full.to(device), ld).view(torch.float32)
    assert image.shape == (rp, ld)
    return image, ld


class _Select:
    """hist, select state and outputs of one staged select"""

    def __init__(self, device):
        self.st = HipStages()
        self.hist = torch.full((_lib.HIST_LEVELS, 2, _lib.HIST_BINS), -1, dtype=torch.int64, device=device)   # (median_begin zeroes it)
        self.sel = torch.full((128,), 0xFF, dtype=torch.uint8, device=device)
        self.h2 = torch.full((1,), -7.0, device=device)
        self.med = torch.full((1,), -7.0, device=device)

    def run(self, blocks, n, total, sym=False):
        """blocks: [(image, ld, n_local)] -- every block's pass of a level adds to the one histogram, then one resolve"""
        st = self.st
        st.median_begin(self.hist, self.sel, total)
        for level in range(_lib.HIST_LEVELS):
            for image, ld, n_local in blocks:
                st.median_hist_pass(image, ld, n_local, n, level, self.sel, self.hist, symmetric=sym)
            st.median_resolve(self.hist, level, n, self.sel, self.h2, self.med)
        torch.cuda.synchronize()
        lo, hi = self.sel[40:48].view(torch.float32).cpu().numpy()      # SelState::lo, ::hi (stein_common.h)
        return np.float32(lo), np.float32(hi), np.float32(self.med.item()), np.float32(self.h2.item())


def _same_float(got, want):
    """equal as floats (-0.0 == +0.0), NaN == NaN; apart from zeros the bit patterns match"""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    return bool(got == want) and (want == 0 or got.view(np.uint32) == want.view(np.uint32))


def _check(got, M, n, tag):
    lo, hi, med = si.exact_median(M)
    want = (lo, hi, med, si.bandwidth(med, n))
    for name, g, w in zip(("lo", "hi", "median", "h2"), got, want):
        assert _same_float(g, w), (tag, name, float(g), float(w), si.diverge_level(lo, hi))


@BOTH
@pytest.mark.parametrize("rows,cols", si.RECT_SHAPES)
@pytest.mark.parametrize("family", si.IMAGE_FAMILIES)
def test_rectangular_block(cuda, family, rows, cols, sentinel):
    M = si.image_rect(family, rows, cols)
    image, ld = _tiled(M, cuda, False, sentinel)
    got = _Select(cuda).run([(image, ld, rows)], cols, rows * cols)
    _check(got, M, cols, (family, rows, cols))


@BOTH
@pytest.mark.parametrize("family,n", si.SYM_CASES, ids=lambda v: str(v))
def test_symmetric_upper_triangle(cuda, family, n, sentinel):
    M = si.image_sym(family, n)
    image, ld = _tiled(M, cuda, True, sentinel)
    got = _Select(cuda).run([(image, ld, n)], n, n * n, sym=True)
    _check(got, M, n, (family, n))


@BOTH
@pytest.mark.parametrize("n", si.SYM_SIZES)
def test_symmetric_with_a_diagonal_of_its_own(cuda, n, sentinel):
    """the diagonal holds 5.0 and nothing else does; the target sits at the end (even n) or the start (odd n) of its tie,
    so the weight-1 entries counted with weight 2, or not at all, give another lo / hi"""
    M = si.image_own_diagonal(n)
    image, ld = _tiled(M, cuda, True, sentinel)
    got = _Select(cuda).run([(image, ld, n)], n, n * n, sym=True)
    _check(got, M, n, ("own diagonal", n))
    assert got[0] == si.DIAG_VALUE


@BOTH
@pytest.mark.parametrize("rows,cols,top", [(300, 1001, 172), (640, 1536, 256), (129, 1000, 1)])
@pytest.mark.parametrize("family", ["adjacent1", "adjacent2", "ties_first", "ties_last", "negative"])
def test_two_row_blocks_of_one_matrix(cuda, family, rows, cols, top, sentinel):
    """the rank protocol without a collective: both blocks' passes of a level add to one histogram, one resolve per
    level.  Bit-identical to the single block and to the sort."""
    M = si.image_rect(family, rows, cols)
    whole = _Select(cuda).run([_tiled(M, cuda, False, sentinel) + (rows,)], cols, rows * cols)
    a, b = _tiled(M[:top], cuda, False, sentinel), _tiled(M[top:], cuda, False, sentinel)
    split = _Select(cuda).run([a + (top,), b + (rows - top,)], cols, rows * cols)
    _check(split, M, cols, (family, rows, cols, top))
    for g, w in zip(split, whole):
        assert np.float32(g).view(np.uint32) == np.float32(w).view(np.uint32) or (np.isnan(g) and np.isnan(w))
