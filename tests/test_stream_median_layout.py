"""CPU: the host side of the streaming median (stein_stream_median, include/steinhip.h): its workspace is a prefix-compatible
subset of the streaming step's and never larger, bad arguments are refused with the documented codes before anything is
launched, the engine and the sampler check their switches, and the lattice inputs the GPU tests use reach every divergence
class of the radix select."""
import ctypes

import pytest

import select_inputs as si
from stein_amd import _lib

NS = (2, 127, 128, 129, 700, 16384, 262144)
DS = (1, 37, 128, 130, 256, 300, 2001)
GRID = [(n, d) for n in NS for d in DS]
HIST_BYTES = _lib.HIST_LEVELS * 2 * _lib.HIST_BINS * 8


def _a256(x):
    return (x + 255) // 256 * 256


def _prefix(n, d):
    """row norms | scales | theta's planes: the streaming step's own first three sections (include/steinhip.h)"""
    N, dk, dc = (n + 127) // 128 * 128, (d + 31) // 32 * 32, (d + 127) // 128 * 128
    return _a256(4 * N) + _a256(4 * (6 * dc + 4)) + _a256(6 * N * dk)


@pytest.mark.parametrize("n,d", GRID)
def test_workspace_fits_inside_the_streaming_steps(n, d):
    med, step = _lib.stream_median_workspace_bytes(n, d), _lib.stream_workspace_bytes(n, d)
    assert 0 < med <= step, (n, d, med, step)
    assert med == _prefix(n, d) + HIST_BYTES + 256, "the header's formula"
    hist_at, state_at, tiles, blocks = _lib.stream_median_plan(n, d)
    assert hist_at == _prefix(n, d)                       # where the step keeps W's planes
    assert state_at == hist_at + HIST_BYTES and state_at + 64 <= med
    assert hist_at % 256 == 0 and state_at % 256 == 0
    nt = (n + 127) // 128
    assert tiles == nt * (nt + 1) // 2 and blocks == min(tiles, 512)


def test_workspace_has_no_term_in_n_squared():
    assert _lib.stream_median_workspace_bytes(262144, 256) < (1 << 30)
    assert _lib.stream_median_workspace_bytes(32768, 64) < (50 << 20)
    assert _lib.stream_workspace_bytes(32768, 64) < (50 << 20)       # the buffer the engine really allocates


def test_debug_grid_moves_the_plan_only():
    try:
        before = _lib.stream_median_workspace_bytes(1536, 130)
        for k in (1, 3, 4096):
            _lib.debug_stream_median_grid(k)
            assert _lib.stream_median_plan(1536, 130)[2:] == (78, k)
            assert _lib.stream_median_workspace_bytes(1536, 130) == before
    finally:
        _lib.debug_stream_median_grid(0)
    assert _lib.stream_median_plan(1536, 130)[2:] == (78, 78)
    with pytest.raises(ValueError):
        _lib.debug_stream_median_grid(-1)


def test_bad_arguments_are_refused_with_the_documented_codes():
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    assert lib.stein_stream_median_workspace_bytes(100, 10, _lib.F32, 0, ref) == _lib.OK and out.value > 0
    assert lib.stein_stream_median_workspace_bytes(2, 1, _lib.F32, 0, ref) == _lib.OK
    assert lib.stein_stream_median_workspace_bytes(1, 10, _lib.F32, 0, ref) == _lib.E_SHAPE      # ln 1 = 0
    assert b"ln n" in lib.stein_last_error()
    assert lib.stein_stream_median_workspace_bytes(0, 10, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert lib.stein_stream_median_workspace_bytes(100, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert lib.stein_stream_median_workspace_bytes(100, 10, _lib.BF16, 0, ref) == _lib.E_UNSUPPORTED
    assert b"bf16" in lib.stein_last_error()
    assert lib.stein_stream_median_workspace_bytes(100, 10, _lib.F64, 0, ref) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, _lib.FLAG_FOLD, 1 << 20):
        assert lib.stein_stream_median_workspace_bytes(100, 10, _lib.F32, flags, ref) == _lib.E_BADARG
    assert lib.stein_stream_median_workspace_bytes(100, 10, _lib.F32, 0, None) == _lib.E_BADARG
    sz, i64, i = ctypes.c_size_t(0), ctypes.c_int64(0), ctypes.c_int(0)
    assert lib.stein_stream_median_plan(100, 10, ctypes.byref(sz), ctypes.byref(sz), ctypes.byref(i64), None) == _lib.E_BADARG
    assert lib.stein_stream_median_plan(1, 10, ctypes.byref(sz), ctypes.byref(sz), ctypes.byref(i64),
                                        ctypes.byref(i)) == _lib.E_SHAPE
    assert lib.stein_debug_stream_median_grid(-1) == _lib.E_BADARG


def test_the_call_checks_its_arguments_before_any_launch():
    """NULL pointers, alignment, dtype, flags, n = 1 and the workspace size are host checks: they answer without a GPU (the
    pointers below are never dereferenced)."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.stream_median_workspace_bytes(100, 10)

    def call(theta=p, n=100, dtype=_lib.F32, h2=p, med=p, ws=p, ws_bytes=need, flags=0):
        return lib.stein_stream_median(theta, n, 10, dtype, h2, med, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"h2": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(dtype=_lib.BF16) == _lib.E_UNSUPPORTED
    assert call(flags=_lib.FLAG_X3) == _lib.E_BADARG
    assert call(n=1) == _lib.E_SHAPE
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ws_bytes=0) == _lib.E_WORKSPACE
    assert call(med=null, ws_bytes=need - 1) == _lib.E_WORKSPACE      # median_out may be NULL: the next check answers


def test_engine_and_sampler_check_their_switches():
    """Everything here is refused before a device buffer is allocated."""
    from stein_amd.engine import SvgdEngine
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    import numpy as np
    import torch
    for bad in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="median_every"):
            SvgdEngine(100, 10, device="cpu", h2="median", median_every=bad)
    with pytest.raises(ValueError, match="median_every"):
        SvgdEngine(100, 10, device="cpu", median_every=2)                 # the stored-D default engine
    with pytest.raises(ValueError, match="median_every"):
        SvgdEngine(100, 10, device="cpu", h2=1.5, median_every=2)         # a supplied bandwidth
    with pytest.raises(ValueError, match="n >= 2"):
        SvgdEngine(1, 10, device="cpu", h2="median")
    # what the streaming engine refuses stays refused, by the same messages
    with pytest.raises(ValueError, match="group"):
        SvgdEngine(100, 10, device="cpu", h2="median", group=object())
    with pytest.raises(ValueError, match="bf16"):
        SvgdEngine(100, 10, device="cpu", h2="median", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="x3=False"):
        SvgdEngine(100, 10, device="cpu", h2="median", x3=False)
    with pytest.raises(ValueError, match="ksd"):
        SvgdEngine(100, 10, device="cpu", h2="median", ksd=True)
    with pytest.raises(ValueError, match="positive finite float"):
        SvgdEngine(100, 10, device="cpu", h2="mean")                      # any other word is not a bandwidth
    T0 = np.zeros((100, 10))
    gd = AdagradGradientDescent(learning_rate=1e-2)
    with pytest.raises(ValueError, match="median_every"):
        SteinSampler(100, None, gd, theta=T0, device="cpu", median_every=2)
    with pytest.raises(ValueError, match="median_every"):
        SteinSampler(100, None, gd, theta=T0, device="cpu", bandwidth=1.3, median_every=2)
    with pytest.raises(ValueError, match="median_every"):
        SteinSampler(100, None, gd, theta=T0, device="cpu", bandwidth="median", median_every=0)
    with pytest.raises(ValueError, match="not both"):
        SteinSampler(100, None, gd, theta=T0, device="cpu", bandwidth="median", h2=torch.ones(1))
    with pytest.raises(ValueError):
        SteinSampler(100, None, gd, theta=T0, device="cpu", bandwidth="wide")


EXPECTED_CLASS = {"two": "L0", "simplex4_128_1": "L2", "simplex4_128_2": "L1", "simplex4_64_1": "L1", "simplex4_8_1": "L1",
                  "scatter": "L1", "line": "same", "grid": "same", "identical": "same"}


@pytest.mark.parametrize("n", [384, 768, 1536])
def test_lattice_cases_reach_every_divergence_class(n):
    """The families of si.families_at(n) that tests/test_gpu_stream_median.py runs put the two median targets in one key
    (`same`) or part them at radix level 0, 1 or 2: every branch of k_stream_hist's prefix tests and of k_resolve."""
    seen = {}
    for f in si.families_at(n):
        ref = si.lattice_ref(f, n)
        seen[f] = si.diverge_level(ref.lo, ref.hi)
        assert seen[f] == EXPECTED_CLASS[f], (f, n, ref.lo, ref.hi, seen[f])
    assert set(seen.values()) == {"same", "L0", "L1", "L2"}, seen
