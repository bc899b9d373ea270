"""CPU: the host arithmetic of the streaming step with the Stein discrepancy sums (stein_svgd_phi_stream_ksd,
include/steinhip.h): its workspace is the plain streaming step's with the partial rd and two more sets of block partials
appended, bad arguments are refused with the documented codes before anything is launched, and the Python switches that
need no device refuse by name."""
import ctypes

import numpy as np
import pytest
import torch

from stein_amd import _lib

NS = (1, 2, 127, 128, 129, 700, 4096, 131072, 262144)
DS = (1, 37, 256, 257, 2001)
GRID = [(n, d) for n in NS for d in DS]


def _a256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("n,d", GRID)
def test_workspace_appends_rd_and_two_partial_sets(n, d):
    plain, ksd = _lib.stream_workspace_bytes(n, d), _lib.stream_ksd_workspace_bytes(n, d)
    jsplit = _lib.stream_plan(n, d)[2]
    sq_blocks = min(1024, (n * d + 1023) // 1024)
    assert ksd >= plain
    assert ksd == plain + _a256(4 * jsplit * n) + _a256(2 * 8 * sq_blocks), "the header's formula"
    if n >= 2:
        assert _lib.stream_median_workspace_bytes(n, d) <= ksd        # one buffer serves all three calls


def test_workspace_follows_the_debug_jsplit():
    try:
        for k in (1, 2, 3, 6):
            _lib.debug_stream_jsplit(k)
            plain, ksd = _lib.stream_workspace_bytes(700, 300), _lib.stream_ksd_workspace_bytes(700, 300)
            assert ksd == plain + _a256(4 * k * 700) + _a256(16 * 206)
    finally:
        _lib.debug_stream_jsplit(0)


def test_262144_x_256_stays_linear():
    assert _lib.stream_ksd_workspace_bytes(262144, 256) < (5 << 28)


def test_bad_arguments_are_refused_with_the_documented_codes():
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    assert lib.stein_stream_ksd_workspace_bytes(100, 10, _lib.F32, 0, ref) == _lib.OK and out.value > 0
    assert lib.stein_stream_ksd_workspace_bytes(1, 1, _lib.F32, 0, ref) == _lib.OK
    assert lib.stein_stream_ksd_workspace_bytes(100, 10, _lib.BF16, 0, ref) == _lib.E_UNSUPPORTED
    assert b"bf16" in lib.stein_last_error()
    assert lib.stein_stream_ksd_workspace_bytes(100, 10, _lib.F64, 0, ref) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, _lib.FLAG_FOLD, 1 << 20):
        assert lib.stein_stream_ksd_workspace_bytes(100, 10, _lib.F32, flags, ref) == _lib.E_BADARG
    assert lib.stein_stream_ksd_workspace_bytes(0, 10, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert lib.stein_stream_ksd_workspace_bytes(100, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert lib.stein_stream_ksd_workspace_bytes(100, 10, _lib.F32, 0, None) == _lib.E_BADARG


def test_the_call_checks_its_arguments_before_any_launch():
    """Host checks only: the pointers below are never dereferenced."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.stream_ksd_workspace_bytes(100, 10)
    assert need > _lib.stream_workspace_bytes(100, 10)

    def call(theta=p, score=p, dtype=_lib.F32, h2=p, phi=p, sums=p, ws=p, ws_bytes=need, flags=0):
        return lib.stein_svgd_phi_stream_ksd(theta, score, 100, 10, dtype, h2, phi, sums, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"score": null}, {"h2": null}, {"sums": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(dtype=_lib.BF16) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD):
        assert call(flags=flags) == _lib.E_BADARG
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ws_bytes=_lib.stream_workspace_bytes(100, 10)) == _lib.E_WORKSPACE    # the plain step's size is too small
    assert call(ws_bytes=0) == _lib.E_WORKSPACE
    assert call(phi=null, ws_bytes=need - 1) == _lib.E_WORKSPACE      # phi may be NULL: the next check answers


def test_python_switches_refuse_without_a_device():
    from stein_amd.engine import SvgdEngine
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    T0 = np.zeros((100, 10))
    gd = AdagradGradientDescent(learning_rate=1e-2)
    with pytest.raises(ValueError, match="ksd_every"):
        SteinSampler(100, None, gd, theta=T0, device="cpu", ksd_every=2)                  # a stored-D sampler
    with pytest.raises(ValueError, match="ksd_every"):
        SteinSampler(100, None, gd, theta=T0, device="cpu", ksd=True, ksd_every=2)
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="ksd_every"):
            SteinSampler(100, None, gd, theta=T0, device="cpu", bandwidth=1.3, ksd_every=bad)
    # the constructor's refusal of ksd=True names the per-call keyword
    with pytest.raises(ValueError, match="ksd.*discrepancy=True"):
        SvgdEngine(100, 10, device="cpu", h2=1.5, ksd=True)
    T = torch.zeros(8, 3)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "wide", True, [1.0, 2.0]):
        with pytest.raises(ValueError, match="bandwidth"):
            ksd(T, T, bandwidth=bad)
    with pytest.raises(ValueError, match="bandwidth=.*float32"):
        ksd(T.bfloat16(), T.bfloat16(), bandwidth=1.0)
    with pytest.raises(ValueError, match="device"):
        ksd(T, T, bandwidth=1.0)                                                           # a good bandwidth: today's checks
