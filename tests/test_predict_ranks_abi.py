"""CPU: the C ABI of the predictive order statistics (include/steinhip.h, csrc/stein_predict_ranks.hip) -- the three declarations
are exported and bound, every refusal comes back with its code and message and in the documented order, and the workspace
size is 76 bytes per (row, rank): independent of n and d, monotone in batch and n_ranks.  No call here passes the checks, so
none reaches a launch, with or without a GPU."""
import ctypes
import os
import re
import sys

import pytest

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quantile_cases as qc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stein_predict_ranks_workspace_bytes", "stein_predict_glm_ranks", "stein_predict_bnn_ranks")


def test_declarations_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for name in NAMES + ("stein_debug_predict_ranks_slices",):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"enum \{ STEIN_PRED_RANKS_MAX = 8 \};", text) and _lib.PRED_RANKS_MAX == 8
    # the model arguments of the summary calls without y and noise_precision, then ranks, n_ranks, out, workspace, size, stream
    tail = [ctypes.POINTER(_lib._i64), _lib._i64, _lib._vp, _lib._vp, _lib._sz, _lib._vp]
    glm, bnn = _lib._SIGNATURES["stein_predict_glm"], _lib._SIGNATURES["stein_predict_bnn"]
    assert _lib._SIGNATURES["stein_predict_glm_ranks"] == glm[:8] + [glm[9]] + tail
    assert _lib._SIGNATURES["stein_predict_bnn_ranks"] == bnn[:8] + [bnn[9]] + tail
    from stein_amd.predict import BnnPredict, GlmPredict
    for cls in (GlmPredict, BnnPredict):
        assert callable(cls.order_statistics) and callable(cls.quantiles)


_BUF = (ctypes.c_double * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer: never dereferenced, every call below is refused
BIG = 1 << 30
KEEP = object()


def _ranks(r):
    return None if r is None else (ctypes.c_int64 * len(r))(*r)


def _glm(lib, n=4, d=8, kind=_lib.GLM_LOGISTIC, output=_lib.PRED_LINK, w_col=0, F=3, batch=5, theta=P, X=P, ranks=(0, 3),
         n_ranks=KEEP, out=P, ws=P, ws_bytes=BIG):
    k = (0 if ranks is None else len(ranks)) if n_ranks is KEEP else n_ranks
    return lib.stein_predict_glm_ranks(theta, n, d, kind, output, w_col, F, X, batch, _ranks(ranks), k, out, ws, ws_bytes, None)


def _bnn(lib, n=4, d=40, n_in=2, H=3, cols=(0, 6, 9, 12, 13, 14), output=_lib.PRED_LINK, batch=5, theta=P, X=P, ranks=(0, 3),
         n_ranks=KEEP, out=P, ws=P, ws_bytes=BIG):
    cols = None if cols is None else (ctypes.c_int64 * 6)(*cols)
    k = (0 if ranks is None else len(ranks)) if n_ranks is KEEP else n_ranks
    return lib.stein_predict_bnn_ranks(theta, n, d, n_in, H, cols, output, X, batch, _ranks(ranks), k, out, ws, ws_bytes, None)


def test_every_refusal_comes_back_before_any_launch():
    lib = _lib.load()
    err = lib.stein_last_error
    nine = tuple(range(9))
    for call in (_glm, _bnn):
        for null in ("theta", "X", "ranks", "out"):
            assert call(lib, n_ranks=2, **{null: None}) == _lib.E_BADARG and b"NULL" in err(), null
        for k in (0, -1):
            assert call(lib, n_ranks=k) == _lib.E_BADARG and b"n_ranks" in err()
        assert call(lib, output=2) == _lib.E_BADARG and b"output" in err()
        for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(n=1 << 31), dict(batch=1 << 31),
                    dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
            assert call(lib, **bad) == _lib.E_SHAPE, bad
        assert call(lib, n=9, ranks=nine) == _lib.E_UNSUPPORTED and b"8 ranks" in err()
        for r in ((0, 4), (-1, 0), (3, 1 << 40)):
            assert call(lib, ranks=r) == _lib.E_BADARG and b"outside [0, 4)" in err(), r
        assert call(lib, ranks=(3, 0, 3, 3, 0), ws=None, ws_bytes=0) == _lib.E_WORKSPACE   # any order, repeats: no refusal of theirs
        need = qc.workspace_bytes(5, 2)
        assert call(lib, ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"workspace" in err()
        assert call(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE and b"too small" in err()
        assert call(lib, ws=ctypes.c_void_p(P.value + 2)) == _lib.E_WORKSPACE and b"aligned" in err()
        # the order: NULL pointers and n_ranks < 1, the output, the shapes, the rank count, the ranks, the workspace
        assert call(lib, theta=None, n_ranks=0) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, n_ranks=0, output=2) == _lib.E_BADARG and b"n_ranks" in err()
        assert call(lib, output=2, n=0) == _lib.E_BADARG and b"output" in err()
        assert call(lib, n=0, ranks=nine) == _lib.E_SHAPE
        assert call(lib, n=4, ranks=nine) == _lib.E_UNSUPPORTED                           # nine ranks, one of them >= n
        assert call(lib, ranks=(0, 4), ws=None, ws_bytes=0) == _lib.E_BADARG and b"outside" in err()
    # the shape and column checks of stein_predict_*: unchanged codes and messages, ahead of the rank checks
    assert _bnn(lib, cols=None) == _lib.E_BADARG and b"NULL" in err()
    assert _glm(lib, kind=2) == _lib.E_BADARG and b"kind" in err()
    assert _glm(lib, F=0) == _lib.E_SHAPE
    assert _glm(lib, w_col=6, F=3) == _lib.E_SHAPE and b"do not fit" in err()
    assert _glm(lib, w_col=-1) == _lib.E_SHAPE
    assert _glm(lib, d=1030, F=1025) == _lib.E_UNSUPPORTED and b"1024 features" in err()
    assert _glm(lib, w_col=6, ranks=nine) == _lib.E_SHAPE and b"do not fit" in err()
    assert _bnn(lib, n_in=0) == _lib.E_SHAPE and _bnn(lib, H=0) == _lib.E_SHAPE
    assert _bnn(lib, n_in=5, cols=(0, 15, 18, 21, 22, 23)) == _lib.E_UNSUPPORTED and b"input features" in err()
    assert _bnn(lib, d=5000, n_in=1, H=1025, cols=(0, 1025, 2050, 3075, 3076, 3077)) == _lib.E_UNSUPPORTED and b"1024 hidden" in err()
    assert _bnn(lib, cols=(0, 5, 9, 12, 13, 14)) == _lib.E_SHAPE and b"overlap" in err()
    assert _bnn(lib, cols=(0, 6, 9, 12, 13, 13)) == _lib.E_SHAPE and b"overlap" in err()
    assert _bnn(lib, d=14) == _lib.E_SHAPE and b"does not fit" in err()
    assert _bnn(lib, cols=(-1, 6, 9, 12, 13, 14)) == _lib.E_SHAPE
    assert _bnn(lib, d=14, ranks=nine) == _lib.E_SHAPE and b"does not fit" in err()


def test_workspace_bytes_has_no_n_and_no_d_and_is_monotone():
    sig = _lib._SIGNATURES["stein_predict_ranks_workspace_bytes"]
    assert sig[:3] == [_lib._i64, _lib._i64, _lib._i64] and len(sig) == 4          # (n, batch, n_ranks, out): no d
    ns = (1, 16, 17, 1000, 16400, 1 << 20, 1 << 30)
    bs = (1, 20, 255, 256, 257, 4000, 100000, 1 << 30)
    for j, b in enumerate(bs):
        for r in range(1, _lib.PRED_RANKS_MAX + 1):
            got = {_lib.predict_ranks_workspace_bytes(n, b, r) for n in ns}
            assert got == {qc.workspace_bytes(b, r)}, (b, r)                       # 76 bytes per (row, rank), whatever n is
            if r > 1:
                assert _lib.predict_ranks_workspace_bytes(5, b, r) > _lib.predict_ranks_workspace_bytes(5, b, r - 1)
            if j:
                assert _lib.predict_ranks_workspace_bytes(5, b, r) > _lib.predict_ranks_workspace_bytes(5, bs[j - 1], r)
    for bad in ((0, 5, 1), (5, 0, 1), (1 << 31, 5, 1), ((1 << 30) + 1, 5, 1), (5, (1 << 30) + 1, 1), (5, 5, 0), (5, 5, 9)):
        with pytest.raises(ValueError):
            _lib.predict_ranks_workspace_bytes(*bad)
    lib = _lib.load()
    assert lib.stein_predict_ranks_workspace_bytes(4, 5, 1, None) == _lib.E_BADARG
    assert lib.stein_predict_ranks_workspace_bytes(4, 5, 0, ctypes.byref(ctypes.c_size_t())) == _lib.E_BADARG
    assert lib.stein_predict_ranks_workspace_bytes(4, 5, 9, ctypes.byref(ctypes.c_size_t())) == _lib.E_UNSUPPORTED


def test_the_slices_hook_takes_its_range_only():
    lib = _lib.load()
    try:
        for k in (1, 7, 1024):
            assert lib.stein_debug_predict_ranks_slices(k) == _lib.OK
        assert lib.stein_debug_predict_ranks_slices(-1) == _lib.E_BADARG
        assert lib.stein_debug_predict_ranks_slices(1025) == _lib.E_BADARG
    finally:
        assert lib.stein_debug_predict_ranks_slices(0) == _lib.OK
