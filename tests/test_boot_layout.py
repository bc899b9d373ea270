"""CPU: the host side of the KSD test's quadratic forms (stein_ksd_boot, include/steinhip.h): its workspace follows the
header's formula, its plan the header's rule, bad arguments are refused with the library's codes before anything is launched,
and the Python functions check their arguments on tensors that never reach the device."""
import ctypes

import pytest
import torch

from stein_amd import _lib
from stein_amd.utilities import ksd_quadratic_forms, stein_goodness_of_fit

SHAPES = [(2, 1, 1), (127, 31, 31), (128, 32, 32), (129, 33, 33), (300, 260, 257), (4096, 256, 256), (16384, 256, 1024),
          (65536, 256, 256), (8192, 2001, 256)]


def _a256(x):
    return (x + 255) // 256 * 256


def _up(x, m):
    return (x + m - 1) // m * m


def _plan(n, reps, forced=0):
    rt, cg = (n + 127) // 128, (reps + 255) // 256
    want = forced if forced > 0 else max(1, 256 // (rt * cg))
    want = min(want, rt)
    per = (rt + want - 1) // want
    return rt, cg, (rt + per - 1) // per


def _bytes(n, d, reps, forced=0):
    R, dk, dc, C, P = _up(n, 128), _up(d, 32), _up(d, 128), _up(reps, 128), _up(reps, 32)
    rt, _, js = _plan(n, reps, forced)
    terms = [4 * R, 4 * (6 * dc + 4), 6 * R * dk, 4 * n * d, 4 * (6 * dc + 4), 6 * R * dk, 4 * (6 * R + 4), 6 * C * R, 4 * R, 4 * R,
             8 * R, 256, 4 * js * rt * P, 4 * reps * n]
    return sum(_a256(t) for t in terms)


@pytest.mark.parametrize("n,d,reps", SHAPES)
def test_size_and_plan_follow_the_header(n, d, reps):
    assert _lib.ksd_boot_plan(n, d, reps) == _plan(n, reps)
    assert _lib.ksd_boot_workspace_bytes(n, d, reps) == _bytes(n, d, reps)
    lib = _lib.load()
    try:
        for k in (1, 2, 3, 1000):
            assert lib.stein_debug_boot_jsplit(k) == _lib.OK
            assert _lib.ksd_boot_plan(n, d, reps) == _plan(n, reps, k)
            assert _lib.ksd_boot_workspace_bytes(n, d, reps) == _bytes(n, d, reps, k)
        assert lib.stein_debug_boot_jsplit(-1) == _lib.E_BADARG
    finally:
        assert lib.stein_debug_boot_jsplit(0) == _lib.OK


def test_the_workspace_is_linear_in_n():
    """no n x n term: 65536 x 256 with 256 rows of weights stays far below one fp32 image of U (16 GiB)"""
    assert _lib.ksd_boot_workspace_bytes(65536, 256, 256) < 1 << 29


def test_sizing_and_plan_refuse_bad_arguments_with_the_documented_codes():
    lib = _lib.load()
    size, plan = lib.stein_ksd_boot_workspace_bytes, lib.stein_ksd_boot_plan
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    assert size(100, 10, 8, _lib.F32, 0, ref) == _lib.OK and out.value > 0
    for dtype in (_lib.BF16, _lib.F64):
        assert size(100, 10, 8, dtype, 0, ref) == _lib.E_UNSUPPORTED
        assert b"bf16" in lib.stein_last_error()
    assert size(100, 10, 8, 7, 0, ref) == _lib.E_UNSUPPORTED
    for flags in (_lib.FLAG_X3, _lib.FLAG_KSD, 1 << 20):
        assert size(100, 10, 8, _lib.F32, flags, ref) == _lib.E_BADARG
    assert size(1, 10, 8, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert b"n >= 2" in lib.stein_last_error()
    assert size(100, 0, 8, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size(100, 10, 0, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert b"reps" in lib.stein_last_error()
    assert size((1 << 24) + 1, 1, 1, _lib.F32, 0, ref) == _lib.E_SHAPE
    assert size(100, 10, 8, _lib.F32, 0, None) == _lib.E_BADARG
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert plan(100, 10, 8, ctypes.byref(a), ctypes.byref(b), None) == _lib.E_BADARG
    assert plan(1, 10, 8, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == _lib.E_SHAPE
    assert plan(100, 10, 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == _lib.E_SHAPE


def test_the_call_checks_its_arguments_before_any_launch():
    """every refusal is a host check: it answers without a GPU (the pointers below are never dereferenced)"""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    need = _lib.ksd_boot_workspace_bytes(100, 10, 8)

    def call(theta=p, score=p, n=100, d=10, dtype=_lib.F32, h2=p, kernel=_lib.KERNEL_IMQ, weights=p, reps=8, q=p, diag=p, ws=p,
             ws_bytes=need, flags=0):
        return lib.stein_ksd_boot(theta, score, n, d, dtype, h2, kernel, weights, reps, q, diag, ws, ws_bytes, flags, null)

    for kw in ({"theta": null}, {"score": null}, {"h2": null}, {"weights": null}, {"q": null}, {"ws": null}):
        assert call(**kw) == _lib.E_BADARG, kw
        assert b"NULL" in lib.stein_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 8)) == _lib.E_BADARG
    assert b"aligned" in lib.stein_last_error()
    assert call(n=1) == _lib.E_SHAPE and call(n=0) == _lib.E_SHAPE and call(d=0) == _lib.E_SHAPE
    assert b"n >= 2" in lib.stein_last_error()
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
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ws_bytes=0) == _lib.E_WORKSPACE
    assert b"workspace" in lib.stein_last_error()
    # diag_out = NULL is allowed: such a call is refused only for the other reasons
    assert call(diag=null, ws_bytes=0) == _lib.E_WORKSPACE


def test_python_argument_checks():
    t = torch.zeros(8, 4)
    w = torch.ones(3, 8)
    with pytest.raises(ValueError, match="kernel must be"):
        ksd_quadratic_forms(t, t, w, kernel="laplace")
    with pytest.raises(ValueError, match="kernel must be"):
        stein_goodness_of_fit(t, t, kernel="laplace")
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "mean", None):
        with pytest.raises(ValueError, match="bandwidth"):
            ksd_quadratic_forms(t, t, w, bandwidth=bad)
    with pytest.raises(ValueError, match="theta must be a torch tensor"):
        ksd_quadratic_forms(t.numpy(), t, w)
    with pytest.raises(ValueError, match="no CPU path"):
        ksd_quadratic_forms(t, t, w)
    with pytest.raises(ValueError, match="no CPU path"):
        stein_goodness_of_fit(t, t, bandwidth=1.0, kernel="rbf")
    for bad in (0, -2, 2.5, True, None):
        with pytest.raises(ValueError, match="n_boot must be an integer >= 1"):
            stein_goodness_of_fit(t, t, n_boot=bad)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), True, "half", None):
        with pytest.raises(ValueError, match="flip_prob must be a float in"):
            stein_goodness_of_fit(t, t, flip_prob=bad)
    with pytest.raises(ValueError, match="statistic must be"):
        stein_goodness_of_fit(t, t, statistic="w")


class _Dev(torch.Tensor):
    """a CPU tensor that says it lives on the device: the checks behind the device check, without one"""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_Dev)


def test_python_shape_and_dtype_checks():
    t = _dev(torch.zeros(8, 4))
    w = _dev(torch.ones(3, 8))
    with pytest.raises(ValueError, match=r"theta must be \[n, d\]"):
        ksd_quadratic_forms(_dev(torch.zeros(8)), t, w)
    with pytest.raises(ValueError, match="score must be float32, got torch.bfloat16"):
        ksd_quadratic_forms(t, _dev(torch.zeros(8, 4, dtype=torch.bfloat16)), w)
    with pytest.raises(ValueError, match="theta must be float32, got torch.bfloat16"):
        stein_goodness_of_fit(_dev(torch.zeros(8, 4, dtype=torch.bfloat16)), t)
    with pytest.raises(ValueError, match="same shape"):
        ksd_quadratic_forms(t, _dev(torch.zeros(8, 5)), w)
    with pytest.raises(ValueError, match="need n >= 2"):
        stein_goodness_of_fit(_dev(torch.zeros(1, 4)), _dev(torch.zeros(1, 4)))
    for bad in (_dev(torch.ones(3, 7)), _dev(torch.ones(8)), _dev(torch.ones(3, 8, dtype=torch.float64)), torch.ones(3, 8), None):
        with pytest.raises(ValueError, match="weights must be a float32 tensor"):
            ksd_quadratic_forms(t, t, bad)
    with pytest.raises(ValueError, match=r"weights must be a float32 tensor \[5, 8\]"):
        stein_goodness_of_fit(t, t, n_boot=5, weights=w)              # 3 rows where n_boot says 5
    with pytest.raises(ValueError, match="statistic='u'"):
        stein_goodness_of_fit(t, t, n_boot=3, weights=w, statistic="u")
    with pytest.raises(ValueError, match="1-element float32 tensor"):
        ksd_quadratic_forms(t, t, w, bandwidth=torch.ones(2))


def test_sharded_sampler_is_refused():
    from stein_amd.samplers import SteinSampler
    s = object.__new__(SteinSampler)
    s._group = object()
    with pytest.raises(ValueError, match="one rank only"):
        s.goodness_of_fit()
