"""CPU: the host side of the Stein-kernel products and the Stein importance weights (stein_ksd_matmul, stein_weights,
include/steinhip.h): their workspaces follow the header's formulas, bad arguments are refused with the library's codes before
anything is launched, and the Python functions check their arguments on tensors that never reach the device."""
import ctypes

import pytest
import torch

from stein_amd import _lib
from stein_amd.utilities import stein_importance_weights, stein_kernel_products
from test_boot_layout import _a256, _plan, _up

SHAPES = [(2, 1, 1), (127, 31, 31), (128, 32, 32), (129, 33, 33), (300, 260, 257), (4096, 256, 256), (16384, 256, 1),
          (65536, 256, 256), (8192, 2001, 1), (262144, 16, 1)]


def _matmul_bytes(n, d, reps, forced=0):
    R, dk, dc, C, P = _up(n, 128), _up(d, 32), _up(d, 128), _up(reps, 128), _up(reps, 32)
    _, _, js = _plan(n, reps, forced)
    terms = [4 * R, 4 * (6 * dc + 4), 6 * R * dk, 4 * n * d, 4 * (6 * dc + 4), 6 * R * dk, 4 * (6 * R + 4), 6 * C * R, 4 * R, 4 * R,
             8 * R, 256, 4 * js * P * R]
    return sum(_a256(t) for t in terms)


def _weights_bytes(n, d, forced=0):
    return sum(_a256(t) for t in [_matmul_bytes(n, d, 1, forced), 8 * n, 8 * n, 4 * n, 4 * n, 2 * 1024 * 24])


@pytest.mark.parametrize("n,d,reps", SHAPES)
def test_sizes_follow_the_header(n, d, reps):
    assert _lib.ksd_matmul_workspace_bytes(n, d, reps) == _matmul_bytes(n, d, reps)
    assert _lib.weights_workspace_bytes(n, d) == _weights_bytes(n, d)
    assert _lib.weights_workspace_bytes(n, d) % 256 == 0
    lib = _lib.load()
    try:
        for k in (1, 2, 3, 1000):                               # the plan is the bootstrap's, and so is its hook
            assert lib.stein_debug_boot_jsplit(k) == _lib.OK
            assert _lib.ksd_matmul_workspace_bytes(n, d, reps) == _matmul_bytes(n, d, reps, k)
            assert _lib.weights_workspace_bytes(n, d) == _weights_bytes(n, d, k)
    finally:
        assert lib.stein_debug_boot_jsplit(0) == _lib.OK
    # the partial block is the only difference to the bootstrap's layout besides the canonical weights it does not keep
    R, P = _up(n, 128), _up(reps, 32)
    rt, _, js = _plan(n, reps)
    assert _lib.ksd_matmul_workspace_bytes(n, d, reps) - _lib.ksd_boot_workspace_bytes(n, d, reps) == \
        _a256(4 * js * P * R) - _a256(4 * js * rt * P) - _a256(4 * reps * n)


def test_the_workspaces_are_linear_in_n():
    """no n x n term: 65536 x 256 stays far below one fp32 image of U (16 GiB), whatever the iteration count"""
    assert _lib.weights_workspace_bytes(65536, 256) < 1 << 29
    assert _lib.ksd_matmul_workspace_bytes(65536, 256, 256) < 1 << 30


def test_sizing_refuses_bad_arguments_with_the_documented_codes():
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    mm = lambda n, d, dtype, flags, o, reps=8: lib.stein_ksd_matmul_workspace_bytes(n, d, reps, dtype, flags, o)   # noqa: E731
    for size, who in ((mm, b"stein_ksd_matmul"), (lib.stein_weights_workspace_bytes, b"stein_weights")):
        assert size(100, 10, _lib.F32, 0, ref) == _lib.OK and out.value > 0
        for dtype in (_lib.BF16, _lib.F64):
            assert size(100, 10, dtype, 0, ref) == _lib.E_UNSUPPORTED
            assert b"bf16" in lib.stein_last_error() and who in lib.stein_last_error()
        assert size(100, 10, 7, 0, ref) == _lib.E_UNSUPPORTED
        for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, 1 << 20):
            assert size(100, 10, _lib.F32, flags, ref) == _lib.E_BADARG
            assert b"flags" in lib.stein_last_error() and who in lib.stein_last_error()
        assert size(1, 10, _lib.F32, 0, ref) == _lib.E_SHAPE
        assert b"n >= 2" in lib.stein_last_error()
        assert size(100, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
        assert size((1 << 24) + 1, 1, _lib.F32, 0, ref) == _lib.E_SHAPE
        assert size(100, 10, _lib.F32, 0, None) == _lib.E_BADARG
    assert mm(100, 10, _lib.F32, 0, ref, reps=0) == _lib.E_SHAPE
    assert b"reps" in lib.stein_last_error()


def test_the_product_call_checks_its_arguments_before_any_launch():
    """every refusal is a host check: it answers without a GPU (the pointers below are never dereferenced)"""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.ksd_matmul_workspace_bytes(100, 10, 8)

    def call(theta=p, score=p, n=100, d=10, dtype=_lib.F32, h2=p, kernel=_lib.KERNEL_IMQ, V=p, reps=8, out=p, ws=p, ws_bytes=need,
             flags=0):
        return lib.stein_ksd_matmul(theta, score, n, d, dtype, h2, kernel, V, reps, out, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"score": null}, {"h2": null}, {"V": null}, {"out": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(n=1) == _lib.E_SHAPE and call(n=0) == _lib.E_SHAPE and call(d=0) == _lib.E_SHAPE
    assert call(n=(1 << 24) + 1) == _lib.E_SHAPE
    assert call(reps=0) == _lib.E_SHAPE and call(reps=-3) == _lib.E_SHAPE
    assert b"reps >= 1" in lib.stein_last_error()
    for dtype in (_lib.BF16, _lib.F64):
        assert call(dtype=dtype) == _lib.E_UNSUPPORTED
        assert b"bf16" in lib.stein_last_error()
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, 1 << 20):
        assert call(flags=flags) == _lib.E_BADARG
        assert b"flags" in lib.stein_last_error()
    for kernel in (-1, 2, 7):
        assert call(kernel=kernel) == _lib.E_BADARG
        assert b"kernel" in lib.stein_last_error()
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE and call(ws_bytes=0) == _lib.E_WORKSPACE
    assert b"workspace" in lib.stein_last_error()


def test_the_weights_call_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.weights_workspace_bytes(100, 10)

    def call(theta=p, score=p, n=100, d=10, dtype=_lib.F32, h2=p, kernel=_lib.KERNEL_IMQ, iters=8, w=p, stats=p, idx=p, gamma=p,
             ws=p, ws_bytes=need, flags=0):
        return lib.stein_weights(theta, score, n, d, dtype, h2, kernel, iters, w, stats, idx, gamma, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"score": null}, {"h2": null}, {"w": null}, {"stats": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(n=1) == _lib.E_SHAPE and call(n=0) == _lib.E_SHAPE and call(d=0) == _lib.E_SHAPE
    assert b"n >= 2" in lib.stein_last_error()
    assert call(n=(1 << 24) + 1) == _lib.E_SHAPE
    assert call(iters=-1) == _lib.E_SHAPE and call(iters=(1 << 30) + 1) == _lib.E_SHAPE
    assert b"iters=" in lib.stein_last_error()
    for dtype in (_lib.BF16, _lib.F64):
        assert call(dtype=dtype) == _lib.E_UNSUPPORTED
        assert b"bf16" in lib.stein_last_error()
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, 1 << 20):
        assert call(flags=flags) == _lib.E_BADARG
        assert b"flags" in lib.stein_last_error()
    for kernel in (-1, 2, 7):
        assert call(kernel=kernel) == _lib.E_BADARG
        assert b"kernel" in lib.stein_last_error()
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE and call(ws_bytes=0) == _lib.E_WORKSPACE
    assert b"workspace" in lib.stein_last_error()
    # idx_out = gamma_out = NULL and iters = 0 are allowed: such calls are refused only for the other reasons
    assert call(idx=null, gamma=null, ws_bytes=0) == _lib.E_WORKSPACE
    assert call(iters=0, ws_bytes=0) == _lib.E_WORKSPACE


def test_the_grid_hook_takes_counts_and_refuses_nonsense():
    lib = _lib.load()
    before = _lib.weights_workspace_bytes(100, 10)
    try:
        for k in (1, 3, 1024, 5000):
            assert lib.stein_debug_weights_grid(k) == _lib.OK
            assert _lib.weights_workspace_bytes(100, 10) == before     # the hook does not move the layout
        assert lib.stein_debug_weights_grid(-1) == _lib.E_BADARG
        assert lib.stein_debug_weights_grid(1 << 20) == _lib.E_BADARG
    finally:
        assert lib.stein_debug_weights_grid(0) == _lib.OK


def test_python_argument_checks():
    t = torch.zeros(8, 4)
    v = torch.ones(3, 8)
    with pytest.raises(ValueError, match="kernel must be"):
        stein_kernel_products(t, t, v, kernel="laplace")
    with pytest.raises(ValueError, match="kernel must be"):
        stein_importance_weights(t, t, kernel="laplace")
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "mean", None):
        with pytest.raises(ValueError, match="bandwidth"):
            stein_kernel_products(t, t, v, bandwidth=bad)
        with pytest.raises(ValueError, match="bandwidth"):
            stein_importance_weights(t, t, bandwidth=bad)
    with pytest.raises(ValueError, match="theta must be a torch tensor"):
        stein_importance_weights(t.numpy(), t)
    with pytest.raises(ValueError, match="no CPU path"):
        stein_kernel_products(t, t, v)
    with pytest.raises(ValueError, match="no CPU path"):
        stein_importance_weights(t, t, bandwidth=1.0, kernel="rbf")


class _Dev(torch.Tensor):
    """a CPU tensor that says it lives on the device: the checks behind the device check, without one"""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_Dev)


def test_python_shape_and_dtype_checks():
    t = _dev(torch.zeros(8, 4))
    v = _dev(torch.ones(3, 8))
    with pytest.raises(ValueError, match=r"theta must be \[n, d\]"):
        stein_kernel_products(_dev(torch.zeros(8)), t, v)
    with pytest.raises(ValueError, match="score must be float32, got torch.bfloat16"):
        stein_importance_weights(t, _dev(torch.zeros(8, 4, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="same shape"):
        stein_importance_weights(t, _dev(torch.zeros(8, 5)))
    with pytest.raises(ValueError, match="need n >= 2"):
        stein_importance_weights(_dev(torch.zeros(1, 4)), _dev(torch.zeros(1, 4)))
    for bad in (_dev(torch.ones(3, 7)), _dev(torch.ones(8)), _dev(torch.ones(3, 8, dtype=torch.float64)), torch.ones(3, 8), None):
        with pytest.raises(ValueError, match="weights must be a float32 tensor"):
            stein_kernel_products(t, t, bad)
    for bad in (-1, 2.5, True, "many"):
        with pytest.raises(ValueError, match="iters must be None or an integer >= 0"):
            stein_importance_weights(t, t, iters=bad)
    with pytest.raises(ValueError, match="1-element float32 tensor"):
        stein_kernel_products(t, t, v, bandwidth=torch.ones(2))
    with pytest.raises(ValueError, match="1-element float32 tensor"):
        stein_importance_weights(t, t, bandwidth=torch.ones(1, dtype=torch.float64))


def test_sharded_sampler_is_refused():
    from stein_amd.samplers import SteinSampler
    s = object.__new__(SteinSampler)
    s._group = object()
    with pytest.raises(ValueError, match="one rank only"):
        s.importance_weights()
