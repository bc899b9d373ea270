"""CPU: the host arithmetic of the streaming step (stein_svgd_phi_stream, include/steinhip.h): its workspace has no term in
n^2, its plan is one workgroup per (row tile of 128, column group of 256, j range), and bad arguments are refused with the
documented codes before anything is launched."""
import ctypes

import pytest

from stein_amd import _lib

NS = (1, 2, 127, 128, 129, 4096, 131072, 1048576)
DS = (1, 37, 256, 257, 2001)
GRID = [(n, d) for n in NS for d in DS]

# What bytes(2n, d) may exceed 2 bytes(n, d) by.  Every term of the documented formula is linear in roundup(n, 128) or in n
# (it at most doubles, plus padding: 128 more rows of both plane images, 6 bytes per entry, (2016 + 2048) columns at the
# widest d here: 3 MiB) except the partial sums, 4 jsplit n d bytes: jsplit > 1 only while jsplit * row_tiles * col_groups
# <= 256 workgroups, and a workgroup's tile is 128 x 256 floats, so with jsplit > 1 they hold at most 256 * 128 KiB = 32 MiB;
# with jsplit = 1 they are linear again.
GROWTH_CONSTANT = (32 << 20) + (4 << 20)


def _a256(x):
    return (x + 255) // 256 * 256


def _formula(n, d, jsplit):
    N, dk, dc = (n + 127) // 128 * 128, (d + 31) // 32 * 32, (d + 127) // 128 * 128
    return (_a256(4 * N) + _a256(4 * (6 * dc + 4)) + _a256(6 * N * dk) + _a256(6 * N * dc) + _a256(4 * jsplit * n * d) +
            _a256(4 * jsplit * n) + _a256(8 * min(1024, (n * d + 1023) // 1024)))


@pytest.mark.parametrize("n,d", GRID)
def test_workspace_is_linear_in_n(n, d):
    b1, b2 = _lib.stream_workspace_bytes(n, d), _lib.stream_workspace_bytes(2 * n, d)
    assert 0 < b1 and b2 <= 2 * b1 + GROWTH_CONSTANT, (n, d, b1, b2)
    assert b1 == _formula(n, d, _lib.stream_plan(n, d)[2]), "the header's formula"


def test_workspace_at_131072_x_256_is_below_one_gib():
    b = _lib.stream_workspace_bytes(131072, 256)
    stored = _lib.workspace_layout(131072, 131072, 256, _lib.F32, _lib.FLAG_X3)[0]
    print("131072 x 256: streaming %.1f MiB, stored-D %.1f GiB" % (b / 2.0 ** 20, stored / 2.0 ** 30))
    assert b < (1 << 30)
    assert stored > (64 << 30)
    # n = 262144 does not fit a stored-D workspace on the card at all; the streaming one is a GiB
    assert _lib.stream_workspace_bytes(262144, 256) < (5 << 28)


@pytest.mark.parametrize("n,d", GRID)
def test_plan_is_consistent(n, d):
    rt, cg, js = _lib.stream_plan(n, d)
    assert rt == (n + 127) // 128 and cg == (d + 255) // 256
    assert 1 <= js <= rt                       # a j range holds at least one 128-column j tile
    assert js == 1 or rt * cg * js <= 256      # ranges only fill a grid that is resident at once
    per = (rt + js - 1) // js
    assert (js - 1) * per < rt                 # no empty range


def test_debug_jsplit_moves_plan_and_workspace_together():
    try:
        natural = _lib.stream_plan(700, 300)
        for k in (1, 2, 3):
            _lib.debug_stream_jsplit(k)
            assert _lib.stream_plan(700, 300) == (6, 2, k)
            assert _lib.stream_workspace_bytes(700, 300) == _formula(700, 300, k)
        _lib.debug_stream_jsplit(4)            # 6 j tiles in ranges of 2: three ranges, none empty
        assert _lib.stream_plan(700, 300)[2] == 3
        _lib.debug_stream_jsplit(1000)
        assert _lib.stream_plan(700, 300)[2] == 6
    finally:
        _lib.debug_stream_jsplit(0)
    assert _lib.stream_plan(700, 300) == natural
    with pytest.raises(ValueError):
        _lib.debug_stream_jsplit(-1)


def test_bad_arguments_are_refused_with_the_documented_codes():
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    assert lib.stein_stream_workspace_bytes(100, 10, _lib.F32, 0, ref) == _lib.OK and out.value > 0
    assert lib.stein_stream_workspace_bytes(1, 1, _lib.F32, 0, ref) == _lib.OK       # n = 1 is allowed: no ln n
    assert lib.stein_stream_workspace_bytes(100, 10, _lib.BF16, 0, ref) == _lib.E_UNSUPPORTED
    assert b"bf16" in lib.stein_last_error()
    assert lib.stein_stream_workspace_bytes(100, 10, _lib.F64, 0, ref) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, _lib.FLAG_FOLD, 1 << 20):
        assert lib.stein_stream_workspace_bytes(100, 10, _lib.F32, flags, ref) == _lib.E_BADARG
    assert lib.stein_stream_workspace_bytes(0, 10, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert lib.stein_stream_workspace_bytes(100, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert lib.stein_stream_workspace_bytes(100, 10, _lib.F32, 0, None) == _lib.E_BADARG
    i = ctypes.c_int(0)
    assert lib.stein_stream_plan(100, 10, ctypes.byref(i), ctypes.byref(i), None) == _lib.E_BADARG
    assert lib.stein_stream_plan(0, 10, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == _lib.E_SHAPE


def test_the_call_checks_its_arguments_before_any_launch():
    """NULL pointers, dtype, flags and the workspace size are host checks: they answer without a GPU (the pointers below
    are never dereferenced)."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.stream_workspace_bytes(100, 10)

    def call(theta=p, score=p, dtype=_lib.F32, h2=p, phi=p, sq=p, ws=p, ws_bytes=need, flags=0):
        return lib.stein_svgd_phi_stream(theta, score, 100, 10, dtype, h2, phi, sq, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"score": null}, {"h2": null}, {"phi": null}, {"sq": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(dtype=_lib.BF16) == _lib.E_UNSUPPORTED
    assert call(flags=_lib.FLAG_X3) == _lib.E_BADARG
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ws_bytes=0) == _lib.E_WORKSPACE
