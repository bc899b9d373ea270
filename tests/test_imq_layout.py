"""CPU: the host arithmetic of the IMQ step (stein_svgd_phi_imq / stein_svgd_phi_imq_ksd, include/steinhip.h): its workspace
has no term in n^2, its plan is one workgroup per (row tile of 128, column block of 128, j range), the layout with the
statistic only appends, a buffer of its size also serves the streaming median, and bad arguments are refused with the
streaming step's codes before anything is launched."""
import ctypes

import pytest

from stein_amd import _lib

NS = (1, 2, 127, 128, 129, 4096, 131072, 1048576)
DS = (1, 37, 128, 129, 256, 257, 2001)
GRID = [(n, d) for n in NS for d in DS]


def _a256(x):
    return (x + 255) // 256 * 256


def _formula(n, d, jsplit):
    N, dk, dc = (n + 127) // 128 * 128, (d + 31) // 32 * 32, (d + 127) // 128 * 128
    return (_a256(4 * N) + _a256(4 * (6 * dc + 4)) + _a256(6 * N * dk) + 2 * _a256(6 * N * dc) +
            2 * _a256(4 * jsplit * n * d) + _a256(4 * jsplit * n) + _a256(8 * min(1024, (n * d + 1023) // 1024)))


def _ksd_extra(n, d, jsplit):
    return _a256(4 * jsplit * n) + _a256(16 * min(1024, (n * d + 1023) // 1024))


@pytest.mark.parametrize("n,d", GRID)
def test_sizes_follow_the_header(n, d):
    js = _lib.imq_plan(n, d)[2]
    plain, ksd = _lib.imq_workspace_bytes(n, d), _lib.imq_ksd_workspace_bytes(n, d)
    assert plain == _formula(n, d, js), "the header's formula"
    assert ksd == plain + _ksd_extra(n, d, js) and ksd > plain      # appended: no offset of the plain layout moves
    if n >= 2:
        assert _lib.stream_median_workspace_bytes(n, d) <= plain    # one buffer serves the median call and the step


@pytest.mark.parametrize("n,d", GRID)
def test_plan_is_consistent(n, d):
    rt, cb, js = _lib.imq_plan(n, d)
    assert rt == (n + 127) // 128 and cb == (d + 127) // 128
    assert 1 <= js <= rt                       # a j range holds at least one 128-column j tile
    assert js == 1 or rt * cb * js <= 256      # ranges only fill a grid that is resident at once
    per = (rt + js - 1) // js
    assert (js - 1) * per < rt                 # no empty range


def test_plan_fills_the_resident_grid_by_the_streaming_rule():
    assert _lib.imq_plan(4096, 256) == (32, 2, 4)       # floor(256 / 64)
    assert _lib.imq_plan(4096, 128) == (32, 1, 8)
    assert _lib.imq_plan(1536, 130) == (12, 2, 6)       # floor(256 / 24) = 10 asks for ranges of two tiles: six ranges
    assert _lib.imq_plan(16384, 256) == (128, 2, 1)
    assert _lib.imq_plan(2, 1) == (1, 1, 1)


def test_debug_jsplit_moves_plan_and_workspace_together():
    try:
        natural = _lib.imq_plan(700, 300)
        for k in (1, 2, 3):
            _lib.debug_stream_jsplit(k)
            assert _lib.imq_plan(700, 300) == (6, 3, k)
            assert _lib.imq_workspace_bytes(700, 300) == _formula(700, 300, k)
            assert _lib.imq_ksd_workspace_bytes(700, 300) == _formula(700, 300, k) + _ksd_extra(700, 300, k)
        _lib.debug_stream_jsplit(4)            # 6 j tiles in ranges of 2: three ranges, none empty
        assert _lib.imq_plan(700, 300)[2] == 3
        _lib.debug_stream_jsplit(1000)
        assert _lib.imq_plan(700, 300)[2] == 6
    finally:
        _lib.debug_stream_jsplit(0)
    assert _lib.imq_plan(700, 300) == natural


@pytest.mark.parametrize("fn", ["stein_imq_workspace_bytes", "stein_imq_ksd_workspace_bytes"])
def test_bad_arguments_are_refused_with_the_documented_codes(fn):
    lib = _lib.load()
    size = getattr(lib, fn)
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    assert size(100, 10, _lib.F32, 0, ref) == _lib.OK and out.value > 0
    assert size(1, 1, _lib.F32, 0, ref) == _lib.OK       # n = 1 is allowed: no ln n
    assert size(100, 10, _lib.BF16, 0, ref) == _lib.E_UNSUPPORTED
    assert b"bf16" in lib.stein_last_error()
    assert size(100, 10, _lib.F64, 0, ref) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, _lib.FLAG_FOLD, 1 << 20):
        assert size(100, 10, _lib.F32, flags, ref) == _lib.E_BADARG
    assert size(0, 10, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size(100, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size(100, 10, _lib.F32, 0, None) == _lib.E_BADARG
    i = ctypes.c_int(0)
    assert lib.stein_imq_plan(100, 10, ctypes.byref(i), ctypes.byref(i), None) == _lib.E_BADARG
    assert lib.stein_imq_plan(0, 10, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == _lib.E_SHAPE
    assert lib.stein_imq_plan(100, 0, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == _lib.E_SHAPE


@pytest.mark.parametrize("ksd", [False, True])
def test_the_calls_check_their_arguments_before_any_launch(ksd):
    """NULL pointers, dtype, flags, the workspace's size and alignment are host checks: they answer without a GPU (the
    pointers below are never dereferenced).  The same codes as stein_svgd_phi_stream{,_ksd} for every refusal."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.imq_ksd_workspace_bytes(100, 10) if ksd else _lib.imq_workspace_bytes(100, 10)
    fn = lib.stein_svgd_phi_imq_ksd if ksd else lib.stein_svgd_phi_imq

    def call(theta=p, score=p, n=100, d=10, dtype=_lib.F32, h2=p, phi=p, out=p, ws=p, ws_bytes=need, flags=0):
        return fn(theta, score, n, d, dtype, h2, phi, out, ws, ws_bytes, flags, null)

    nulls = [{"theta": null}, {"score": null}, {"h2": null}, {"out": null}, {"ws": null}]
    if not ksd:
        nulls.append({"phi": null})            # (the statistic's call takes phi = NULL: the sums alone)
    for kw in nulls:
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(dtype=_lib.BF16) == _lib.E_UNSUPPORTED
    assert call(flags=_lib.FLAG_X3) == _lib.E_BADARG
    assert call(n=0) == _lib.E_SHAPE and call(d=0) == _lib.E_SHAPE
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ws_bytes=0) == _lib.E_WORKSPACE
    if ksd:                                    # the plain layout's size is too short for the statistic
        assert call(ws_bytes=_lib.imq_workspace_bytes(100, 10)) == _lib.E_WORKSPACE
