"""CPU: the case tables of the one-kernel path (tests/small_cases.py) reach every code shape k_svgd_small can take, and the
dispatch model they are built from agrees with the library on which shapes take that kernel -- host arithmetic only, through
stein_workspace_layout (the SPEC section is empty exactly where the fused call will take the one-kernel path; that is how
stein_amd/engine.py reads it)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_cases as sc  # noqa: E402
from stein_amd import _lib  # noqa: E402

X3, TILED, KSD = _lib.FLAG_X3, _lib.FLAG_TILED, _lib.FLAG_KSD
ALL_ON_PATH = sc.MATRIX_CASES + sc.WIDE_CASES + sc.KSD_CASES + sc.BIT_CASES + [on for on, _ in sc.EDGE_OF_PATH]


def _library_takes_one_kernel(n_local, n, d, dtype=_lib.F32, flags=X3):
    _, offs, _ = _lib.workspace_layout(n_local, n, d, dtype, flags)
    return offs[_lib.WS_PLANES] == offs[_lib.WS_SPEC]


def _domain():
    """every (n, d) of the path with d <= 600, and the wide tail at a stride"""
    for n in range(2, sc.SM_MAXN + 1):
        top = min(sc.MAX_WORK // (n * n), sc.MAX_BLOCKS * sc.SM_COLS)
        for d in list(range(1, min(top, 600) + 1)) + list(range(601, top + 1, 97)) + [top]:
            yield n, d


def test_tables_have_their_stated_sizes():
    assert len(sc.EDGE_N) == 19 and len(sc.EDGE_D) == 13
    assert len(sc.RANDOM_CASES) == 24 and len(set(sc.RANDOM_CASES)) == 24
    assert all(2 <= n <= 160 and 1 <= d <= min(600, sc.MAX_WORK // (n * n)) for n, d in sc.RANDOM_CASES)
    assert len(sc.MATRIX_CASES) == len(set(sc.MATRIX_CASES)) <= 320
    for n in (2, 32, 33, 64, 65, 96, 97, 128, 129, 160):           # the full d set at the ends of every (R, RW) class
        assert all((n, d) in sc.EDGE_CASES for d in sc.EDGE_D), n
    assert all(sc.classify(lo, 1)["R"] == sc.classify(hi, 1)["R"] for lo, hi in sc._KSD_N)


def test_every_reachable_code_shape_is_in_the_tables():
    reachable = {(c["R"], c["RW"], c["clw_last"]) for c in (sc.classify(n, d) for n, d in _domain())}
    assert len(reachable) == 15                                     # five (R, RW) classes of n, three CLW
    cls = [sc.classify(n, d) for n, d in sc.MATRIX_CASES]
    assert all(c["on_path"] for c in cls)
    for multi in (False, True):                                     # each on a one-workgroup and on a multi-workgroup launch
        have = {(c["R"], c["RW"], c["clw_last"]) for c in cls if (c["blocks"] > 1) == multi}
        assert have == reachable, (multi, sorted(reachable - have))
    assert {c["clw_last"] for c in cls if c["R"] == 3} == {8, 16, 32}
    assert {c["RW"] for c in cls if c["blocks"] > 1 and c["clw_first"] != c["clw_last"]} == {2, 4, 8, 10}
    # CLW = 8 behind full workgroups at RW = 4; the first and the last workgroup differ at RW = 4 and at RW = 10
    assert any(c["RW"] == 4 and c["blocks"] > 1 and c["clw_last"] == 8 for c in cls)
    chunks = {c["chunks"] for c in cls}
    assert {1, 2, 3} <= chunks and max(chunks) >= 5, sorted(chunks)
    assert {c["ck"] for c in cls} >= {32, 64, 96, 128, 224, 256}
    assert {c["R"] for c in cls} == {1, 2, 3, 4, 5}


def test_chunk_cases_sit_on_the_chunk_edges():
    for n, d in sc.CHUNK_CASES:
        assert sc.chunk_role(n, d), (n, d, sc.full_chunk(n))
    roles = {(sc.classify(n, d)["chunks"], r) for n, d in sc.CHUNK_CASES for r in sc.chunk_role(n, d)}
    assert {(1, "k*ck"), (2, "k*ck+1"), (2, "k*ck-1"), (2, "k*ck"), (3, "k*ck+1")} <= roles, sorted(roles)
    assert any(c >= 5 and r == "k*ck" for c, r in roles) and any(c >= 5 and r == "k*ck+1" for c, r in roles)
    for a, b in ((20, 21), (40, 41), (80, 81)):                     # the steps of the chunk that n allows
        assert sc.full_chunk(a) > sc.full_chunk(b)
        assert any(n == a for n, _ in sc.CHUNK_CASES) and any(n == b for n, _ in sc.CHUNK_CASES)
    assert [sc.full_chunk(n) for n in (2, 20, 21, 40, 41, 53, 80, 81, 160)] == [256, 256, 224, 128, 96, 96, 64, 32, 32]


def test_ksd_and_bit_subsets_span_the_dispatch():
    cls = [sc.classify(n, d) for n, d in sc.KSD_CASES]
    for multi in (False, True):
        have = {(c["R"], c["RW"], c["clw_last"]) for c in cls if (c["blocks"] > 1) == multi}
        assert len(have) == 15, (multi, sorted(have))
    assert any(c["blocks"] == sc.MAX_BLOCKS for c in cls)
    assert sorted(sc.classify(n, d)["R"] for n, d in sc.BIT_CASES) == [1, 2, 3, 4, 5]
    assert all(sc.classify(n, d)["blocks"] > 1 for n, d in sc.BIT_CASES)
    assert {sc.classify(n, 1)["R"] for n in sc.SELECT_N} == {2, 3, 4} and sum(sc.classify(n, 1)["R"] == 3 for n in sc.SELECT_N) == 3
    assert {(n * n) % 2 for n in sc.SELECT_N} == {0, 1}


def test_wide_cases_reach_the_workgroup_and_work_bounds():
    cls = {c: sc.classify(*c) for c in sc.WIDE_CASES}
    assert all(c["on_path"] and c["chunks"] >= 17 for c in cls.values())
    assert cls[(2, 32768)]["blocks"] == sc.MAX_BLOCKS
    assert 13 * 13 * 13000 <= sc.MAX_WORK < 13 * 13 * 13100
    for (n, d), c in cls.items():                                   # sized by columns: more partials than the finish pass has
        extra = _lib.workspace_layout(n, n, d, _lib.F32, X3)[2]
        assert c["blocks"] > extra[_lib.WSX_SQ_BLOCKS], (n, d)


def test_model_agrees_with_the_library_on_who_takes_the_path():
    for n, d in ALL_ON_PATH:
        assert sc.classify(n, d)["on_path"] and _library_takes_one_kernel(n, n, d), (n, d)
        assert _library_takes_one_kernel(n, n, d, flags=X3 | KSD) and _library_takes_one_kernel(n, n, d, flags=0), (n, d)
        assert not _library_takes_one_kernel(n, n, d, flags=X3 | TILED), (n, d)
        assert not _library_takes_one_kernel(n, n, d, dtype=_lib.BF16), (n, d)
        assert not _library_takes_one_kernel(n - 1, n, d), (n, d)                   # a row block (n_local < n)
    for on, off in sc.EDGE_OF_PATH:
        assert sc.classify(*on)["on_path"] and not sc.classify(*off)["on_path"], (on, off)
        assert _library_takes_one_kernel(on[0], on[0], on[1]) and not _library_takes_one_kernel(off[0], off[0], off[1]), (on, off)
        assert abs(on[0] - off[0]) + abs(on[1] - off[1]) == 1
    assert 100 * 100 * 220 == sc.MAX_WORK                                          # the bound itself is on the path
    for n, d in _domain():                                                          # the whole domain, and one step past it
        assert _library_takes_one_kernel(n, n, d), (n, d)
    for n in range(2, sc.SM_MAXN + 1):
        top = min(sc.MAX_WORK // (n * n), sc.MAX_BLOCKS * sc.SM_COLS)
        assert sc.classify(n, top)["on_path"] and not sc.classify(n, top + 1)["on_path"]
        assert not _library_takes_one_kernel(n, n, top + 1), (n, top + 1)
    assert not _library_takes_one_kernel(161, 161, 1)


def test_one_particle_is_refused():
    assert not sc.classify(1, 5)["on_path"]
    for flags in (X3, X3 | KSD, X3 | TILED):
        with pytest.raises(ValueError, match=r"ln\(n\)"):
            _lib.workspace_layout(1, 1, 5, _lib.F32, flags)


def test_partials_section_holds_one_double_per_workgroup():
    for n, d in ALL_ON_PATH:
        blocks = sc.classify(n, d)["blocks"]
        for flags, sets in ((X3, 1), (X3 | KSD, 3), (0, 1), (KSD, 3)):
            _, offs, _ = _lib.workspace_layout(n, n, d, _lib.F32, flags)
            assert offs[_lib.WS_SPEC] - offs[_lib.WS_SQPART] >= 8 * blocks * sets, (n, d, flags)
