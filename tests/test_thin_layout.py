"""CPU: the host side of Stein thinning (stein_thin, include/steinhip.h): its workspace is O(n) and follows the header's
formula, bad arguments are refused with the library's codes before anything is launched, and the Python function checks its
arguments on tensors that never reach the device."""
import ctypes

import pytest
import torch

from stein_amd import _lib
from stein_amd.utilities import stein_thinning

NS = (1, 2, 31, 32, 33, 4096, 131073, 1048576)
DS = (1, 4, 37, 256, 2001)


def _a256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("n", NS)
def test_size_follows_the_header(n):
    want = _a256(8 * n) + _a256(2 * 1024 * 16) + _a256(8)
    for d in DS:
        assert _lib.thin_workspace_bytes(n, d) == want          # no term in d, none in the pick count
    assert want <= 8 * n + 33280 + 255


def test_sizing_refuses_bad_arguments_with_the_documented_codes():
    lib = _lib.load()
    size = lib.stein_thin_workspace_bytes
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    assert size(100, 10, _lib.F32, 0, ref) == _lib.OK and out.value > 0
    assert size(1, 1, _lib.F32, 0, ref) == _lib.OK
    for dtype in (_lib.BF16, _lib.F64):
        assert size(100, 10, dtype, 0, ref) == _lib.E_UNSUPPORTED
        assert b"bf16" in lib.stein_last_error()
    assert size(100, 10, 7, 0, ref) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, 1 << 20):
        assert size(100, 10, _lib.F32, flags, ref) == _lib.E_BADARG
    assert size(0, 10, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size(100, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size((1 << 30) + 1, 1, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size(100, 10, _lib.F32, 0, None) == _lib.E_BADARG


def test_the_call_checks_its_arguments_before_any_launch():
    """every refusal is a host check: it answers without a GPU (the pointers below are never dereferenced)"""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.thin_workspace_bytes(100, 10)

    def call(theta=p, score=p, n=100, d=10, dtype=_lib.F32, h2=p, kernel=_lib.KERNEL_IMQ, m=8, idx=p, ksd2=p, ws=p,
             ws_bytes=need, flags=0):
        return lib.stein_thin(theta, score, n, d, dtype, h2, kernel, m, idx, ksd2, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"score": null}, {"h2": null}, {"idx": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(n=0) == _lib.E_SHAPE and call(d=0) == _lib.E_SHAPE
    assert call(m=0) == _lib.E_SHAPE and call(m=-3) == _lib.E_SHAPE
    assert b"m=" in lib.stein_last_error()
    for dtype in (_lib.BF16, _lib.F64):
        assert call(dtype=dtype) == _lib.E_UNSUPPORTED
        assert b"bf16" in lib.stein_last_error()
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, 1 << 20):
        assert call(flags=flags) == _lib.E_BADARG
        assert b"flags" in lib.stein_last_error()
    for kernel in (-1, 2, 7):
        assert call(kernel=kernel) == _lib.E_BADARG
        assert b"kernel" in lib.stein_last_error()
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ws_bytes=0) == _lib.E_WORKSPACE
    assert b"workspace" in lib.stein_last_error()
    # a refused ksd2_out = NULL call is refused for the same reasons (NULL itself is allowed)
    assert call(ksd2=null, ws_bytes=0) == _lib.E_WORKSPACE


def test_the_grid_hook_takes_counts_and_refuses_nonsense():
    lib = _lib.load()
    try:
        for k in (1, 3, 1024, 5000):
            assert lib.stein_debug_thin_grid(k) == _lib.OK
        assert lib.stein_debug_thin_grid(-1) == _lib.E_BADARG
        assert lib.stein_debug_thin_grid(1 << 20) == _lib.E_BADARG
    finally:
        assert lib.stein_debug_thin_grid(0) == _lib.OK
    assert _lib.thin_workspace_bytes(100, 10) == _a256(800) + 32768 + 256     # the hook does not move the layout


def test_python_argument_checks():
    t = torch.zeros(8, 4)
    with pytest.raises(ValueError, match="kernel must be"):
        stein_thinning(t, t, 3, kernel="laplace")
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "mean", None):
        with pytest.raises(ValueError, match="bandwidth"):
            stein_thinning(t, t, 3, bandwidth=bad)
    with pytest.raises(ValueError, match="theta must be a torch tensor"):
        stein_thinning(t.numpy(), t, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        stein_thinning(t, t, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        stein_thinning(t, t, 3, bandwidth=1.0, kernel="rbf")


class _Dev(torch.Tensor):
    """a CPU tensor that says it lives on the device: the checks behind the device check, without one"""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_Dev)


def test_python_shape_and_dtype_checks():
    t = _dev(torch.zeros(8, 4))
    with pytest.raises(ValueError, match=r"theta must be \[n, d\]"):
        stein_thinning(_dev(torch.zeros(8)), t, 3)
    with pytest.raises(ValueError, match="score must be float32, got torch.bfloat16"):
        stein_thinning(t, _dev(torch.zeros(8, 4, dtype=torch.bfloat16)), 3)
    with pytest.raises(ValueError, match="theta must be float32, got torch.float64"):
        stein_thinning(_dev(torch.zeros(8, 4, dtype=torch.float64)), t, 3)
    with pytest.raises(ValueError, match="same shape"):
        stein_thinning(t, _dev(torch.zeros(8, 5)), 3)
    for bad in (0, -2, 2.5, True, None):
        with pytest.raises(ValueError, match="m must be an integer >= 1"):
            stein_thinning(t, t, bad)
    with pytest.raises(ValueError, match="1-element float32 tensor"):
        stein_thinning(t, t, 3, bandwidth=torch.ones(2))
    with pytest.raises(ValueError, match="1-element float32 tensor"):
        stein_thinning(t, t, 3, bandwidth=torch.ones(1, dtype=torch.float64))


def test_sharded_sampler_is_refused():
    from stein_amd.samplers import SteinSampler
    s = object.__new__(SteinSampler)
    s._group = object()
    with pytest.raises(ValueError, match="one rank only"):
        s.thin(4)
