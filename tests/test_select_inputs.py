"""CPU: the inputs of tests/select_inputs.py have the properties that make them hard for a radix select -- the level at
which the two targets part, the size of the ties they fall into, where inside the tie, what the diagonal weighs there --
and its references agree with each other and with the oracle.  Asserted for every (family, n) that
test_gpu_select_lattice.py runs and every image of test_gpu_select_images.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_inputs as si  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402


def test_keys_order_like_floats_and_levels_classify():
    x = np.array([-np.inf, -3.0, -1e-9, -1e-45, -0.0, 0.0, 1e-45, 1.17549435e-38, 1.0, 2.0, np.inf], dtype=np.float32)
    k = si.f32_key(x).astype(np.int64)
    assert np.all(np.diff(k) > 0)                              # strictly monotone, -0.0 just below +0.0
    assert k[4] == 0x7fffffff and k[5] == 0x80000000
    assert np.array_equal(si.key_f32(si.f32_key(x)).view(np.uint32), x.view(np.uint32))
    assert int(si.f32_key(np.float32("nan"))) > int(si.f32_key(np.float32("inf")))   # NaN padding sorts behind every value
    r = np.random.default_rng(0).normal(size=4096).astype(np.float32)
    assert np.array_equal(np.argsort(si.f32_key(r), kind="stable"), np.argsort(r, kind="stable"))
    two = np.float32(2.0)
    assert si.diverge_level(two, two) == "same"
    assert si.diverge_level(np.nextafter(two, np.float32(0)), two) == "L0"           # 2.0 opens a level-0 bin
    assert si.diverge_level(two, si.key_f32(np.uint32(0xC0000000 + 1024))) == "L1"
    assert si.diverge_level(two, si.key_f32(np.uint32(0xC0000000 + 1023))) == "L2"


def test_exact_median_weighted_equals_expanded_and_the_oracle():
    rng = np.random.default_rng(1)
    for count in (1, 2, 9, 10, 1001):
        v = rng.integers(-5, 6, size=count).astype(np.float32) / 4
        w = rng.integers(1, 4, size=count)
        assert si.exact_median(v, w) == si.exact_median(np.repeat(v, w))
        lo, hi, med = si.exact_median(v)
        assert med == orc.median_all(v)
    assert si.exact_median(np.array([1, 2, 3, 4], np.float32)) == (2.0, 3.0, 2.5)
    assert si.exact_median(np.array([1, 2, 3], np.float32)) == (2.0, 2.0, 2.0)
    assert si.exact_median(np.array([7, 5], np.float32), [1, 2]) == (5.0, 5.0, 5.0)


# ---- lattices ------------------------------------------------------------------------------------------------------
LINE_MULT = {160: 3816, 768: 87210, 2304: 786432}
GRID_MULT = {160: 338, 768: 2306}
SIMPLEX_FACTS = {"simplex4_128_1": (32768, 32769, "L2"), "simplex4_128_2": (32768, 32772, "L1"),
                 "simplex4_64_1": (8192, 8193, "L1"), "simplex4_8_1": (128, 129, "L1")}


@pytest.mark.parametrize("family,n", si.lattice_cases(), ids=lambda v: str(v))
def test_lattice_has_the_property_that_makes_it_hard(family, n):
    ref = si.lattice_ref(family, n)
    P, D = ref.P, ref.D
    assert P.min() >= 0 and P.max() <= 256                      # exact in bf16, fp16 split terms and fp32
    assert D.max() < 1 << 24 and np.array_equal(D, D.T) and not np.diag(D).any()
    # the int64 order statistics are those of the oracle's median on the same values as fp32
    assert ref.med == orc.median_all(D.astype(np.float32))
    assert ref.h2 == orc.bandwidth_sq(ref.med, n, np.float32) or (np.isnan(ref.h2) and ref.med < 0)
    level = si.diverge_level(ref.lo, ref.hi)
    over = ref.upper_mult_lo > si.SPEC_CAP
    if (family, n) in si.OVER_CAPACITY:
        assert over
    if n in si.WINDOW_N + si.SOLO_N + si.RANK_N:               # where a window may open, the buffer could hold lo's whole tie
        assert not over, (family, n, ref.upper_mult_lo)
    if family == "line":
        assert level == "same" and ref.distinct == min(9, n)
        if n >= 129:
            assert ref.lo == 9 and ref.mult_lo > n * n // 8    # both targets deep inside one tie
        if n in LINE_MULT:
            assert ref.mult_lo == LINE_MULT[n]
    elif family == "grid":
        assert level == "same"
        if n >= 129:
            assert ref.distinct >= 100 and ref.mult_lo >= 100
        if n in GRID_MULT:
            assert ref.mult_lo == GRID_MULT[n]
    elif family == "two":
        assert (ref.lo, ref.hi, level) == (0, 18, "L0") and ref.med == 9.0
        assert ref.mult_lo == n * n // 2 == ref.mult_hi          # the tie at 0 holds the whole diagonal (weight 1 entries)
    elif family == "identical":
        assert (ref.lo, ref.hi, ref.distinct) == (0, 0, 1) and ref.h2 == 0.0
    elif family == "scatter":
        # two targets on different values, ties far below the 1016 entries of one workgroup's window queue, and 256 .. 4096
        # keys apart: both inside the 8192-key window [lo - 4096, lo + 4096] in different high bytes of it (two_hb), hi
        # outside the later 96-key window (a miss by bb == 256)
        gap = int(si.f32_key(np.float32(ref.hi))) - int(si.f32_key(np.float32(ref.lo)))
        assert ref.lo != ref.hi and 256 <= gap <= 4096 and level in ("L1", "L0")
        assert ref.mult_lo <= 300 and ref.mult_hi <= 300 and ref.distinct >= 10000
        near = np.abs(D - ref.lo) <= 8                         # every entry the 8192-key window can hold (>= 512 keys per integer)
        assert int(np.triu(near).sum()) < 1016
        if n == 768:
            assert (ref.lo, ref.hi, gap) == (10600, 10601, 1024)
    else:
        lo, hi, lv = SIMPLEX_FACTS[family]
        assert (ref.lo, ref.hi, level) == (lo, hi, lv)
        assert (ref.mult_lo, ref.mult_hi, ref.distinct) == (n * n // 4, n * n // 2, 3)
        count = np.bincount(D.reshape(-1))                     # the sorted D: n^2/4 zeros, n^2/4 of lo, n^2/2 of hi
        assert (count[0], count[lo], count[hi]) == (n * n // 4, n * n // 4, n * n // 2)
        if family == "simplex4_128_1":
            assert float(ref.med) == 32768.5
            # 256 keys apart: inside one 8192-key window (half-width 4096), in different high bytes of it
            assert int(si.f32_key(np.float32(hi))) - int(si.f32_key(np.float32(lo))) == 256
    if n % 2 == 1:
        assert ref.lo == ref.hi                                  # odd count: one target


def test_simplex_rows_are_permuted():
    P = si.lattice("simplex4_128_1", 768)
    assert not np.array_equal(P[:, :4].argmax(1), np.arange(768) % 4)
    assert sorted(P[:, :4].argmax(1).tolist()) == sorted((np.arange(768) % 4).tolist())


# ---- images --------------------------------------------------------------------------------------------------------
def _check_image(family, M, total_even, n_cols):
    flat = M.reshape(-1)
    assert M.dtype == np.float32 and not np.isnan(flat).any()
    lo, hi, med = si.exact_median(flat)
    level = si.diverge_level(lo, hi)
    m_lo, m_hi = si.multiplicity(flat, lo), si.multiplicity(flat, hi)
    at_or_below = int((flat <= lo).sum())
    if family.startswith("adjacent"):
        kb = si.ADJ_HI_KEY[int(family[-1])]
        a, b = si.key_f32(np.uint32(kb - 1)), si.key_f32(np.uint32(kb))
        if total_even:
            assert (lo, hi) == (a, b) and level == "L" + family[-1]
            assert 2 * at_or_below == flat.size                  # exactly half the weight at or below lo
            assert si.with_stray_low(flat, 1) == (a, a)          # ... so ONE stray count below the values turns hi into lo
        else:
            assert lo == hi == a and level == "same"
        assert m_lo >= flat.size // 4 and (0.5 in flat or flat.size < 12) and si.multiplicity(flat, b) >= 1
    elif family == "negative":
        assert level == "same" and lo < 0 and -1e-6 <= lo <= -1e-9 and np.isnan(si.bandwidth(med, n_cols))
        assert 2 * int((flat < 0).sum()) > flat.size
        if flat.size >= 64:
            signs = np.signbit(flat[flat == 0])
            assert signs.any() and not signs.all()              # -0.0 and +0.0
            assert (flat > 0).any() and m_lo >= flat.size // 16
    elif family == "wide":
        assert level in ("same", "L0") and np.isfinite(med) and med > 0
        if flat.size >= 64:
            pos = flat[np.isfinite(flat)]
            assert np.isinf(flat).any() and (pos < np.finfo(np.float32).tiny).any() and np.finfo(np.float32).tiny in flat
            assert np.log2(float(pos.max()) / float(np.finfo(np.float32).tiny)) >= 60 and len(set(flat.tolist())) == len(si.WIDE_VALUES)
    else:
        position = family.split("_")[1]
        v = si.key_f32(np.array(si.TIE_KEYS, dtype=np.uint32))
        assert lo == hi == v[1] and level == "same" and len(set(flat.tolist())) <= 3
        srt = np.sort(flat)
        r0, r1 = si.target_ranks(flat.size)
        first, last = int(np.searchsorted(srt, v[1], "left")), int(np.searchsorted(srt, v[1], "right")) - 1
        assert m_lo == last - first + 1 and m_lo >= min(flat.size // 4, flat.size - 1)
        if position == "first":
            assert r0 == first
        elif position == "last":
            assert r1 == last
        elif flat.size >= 16:
            assert first < r0 and r1 < last
    return lo, hi, level, m_lo, m_hi


@pytest.mark.parametrize("rows,cols", si.RECT_SHAPES)
@pytest.mark.parametrize("family", si.IMAGE_FAMILIES)
def test_rectangular_images(family, rows, cols):
    M = si.image_rect(family, rows, cols)
    assert M.shape == (rows, cols) and np.array_equal(M, si.image_rect(family, rows, cols))
    _check_image(family, M, rows * cols % 2 == 0, cols)
    # two row blocks of one matrix hold the same multiset between them
    if rows >= 2:
        top = rows * 4 // 7
        assert si.exact_median(np.concatenate([M[:top].ravel(), M[top:].ravel()])) == si.exact_median(M)


@pytest.mark.parametrize("family,n", si.SYM_CASES, ids=lambda v: str(v))
def test_symmetric_images(family, n):
    M = si.image_sym(family, n)
    assert np.array_equal(M, M.T)                               # (-0.0 == +0.0)
    lo, hi, level, m_lo, m_hi = _check_image(family, M, n % 2 == 0, n)
    # the stored half with weights 2 / 1 is the same multiset
    iu = np.triu_indices(n)
    w = np.where(iu[0] == iu[1], 1, 2)
    assert si.exact_median(M[iu], w) == si.exact_median(M)
    # the targets' tie contains diagonal entries (weight 1) and off-diagonal ones (weight 2) wherever there is room for both
    dg = np.diag(M)
    on_diag = int(((dg == lo) | (dg == hi)).sum())
    assert on_diag >= 1
    if n >= 33:
        assert on_diag >= n // 2 and m_lo > on_diag


def test_every_family_has_a_symmetric_image_at_every_size_above_two():
    assert {(f, n) for n in si.SYM_SIZES[1:] for f in si.IMAGE_FAMILIES} <= set(si.SYM_CASES)
    assert {f for f, n in si.SYM_CASES if n == 2} == {f for f in si.IMAGE_FAMILIES if f.startswith(("adjacent", "ties"))}


@pytest.mark.parametrize("n", si.SYM_SIZES)
def test_own_diagonal_image_turns_on_the_diagonal_weight(n):
    M = si.image_own_diagonal(n)
    assert np.array_equal(M, M.T) and np.all(np.diag(M) == si.DIAG_VALUE) and si.multiplicity(M, si.DIAG_VALUE) == n
    lo, hi, med = si.exact_median(M)
    iu = np.triu_indices(n)
    stored, w = M[iu], np.where(iu[0] == iu[1], 1, 2)
    assert si.exact_median(stored, w) == (lo, hi, med)
    if n % 2 == 0:
        assert (lo, hi, med) == (5.0, 9.0, 7.0) and si.diverge_level(lo, hi) == "L0"
        # a diagonal entry counted twice, or not at all, gives another answer
        assert si.exact_median(stored, np.full_like(w, 2))[:2] == (5.0, 5.0) or n == 2
        assert si.exact_median(stored[w == 2], w[w == 2])[0] == 9.0
    else:
        assert lo == hi == med == 5.0
        assert si.exact_median(stored[w == 2], w[w == 2])[0] != 5.0    # the diagonal not counted
