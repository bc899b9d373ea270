"""CPU: the C ABI of the predictive producers (include/steinhip.h, csrc/stein_predict.hip) -- the declarations are
exported, every refusal comes back with its code and a message before anything is launched, and the workspace size is
monotone in both of its arguments and has no others.  No call here passes the checks, so none reaches a launch, with or
without a GPU (that a call for pred alone needs no workspace is a launching call: the subsets of
tests/test_gpu_predict_matrix.py make it)."""
import ctypes
import os
import re
import sys

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stein_predict_workspace_bytes", "stein_predict_glm", "stein_predict_bnn")


def test_declarations_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    assert "STEIN_PRED_LINK = 0, STEIN_PRED_MEAN = 1" in text and (_lib.PRED_LINK, _lib.PRED_MEAN) == (0, 1)
    from stein_amd import scores
    from stein_amd.predict import BnnPredict, GlmPredict
    assert scores.GlmPredict is GlmPredict and scores.BnnPredict is BnnPredict
    assert GlmPredict.wants_matrix is True and BnnPredict.wants_matrix is True


_BUF = (ctypes.c_float * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer: never dereferenced, every call below is refused before a launch
BIG = 1 << 30


def _glm(lib, n=4, d=8, kind=_lib.GLM_LOGISTIC, output=_lib.PRED_LINK, w_col=0, F=3, batch=5, tau=1.0, theta=P, X=P, y=P,
         pred=P, mean=P, var=P, lpd=P, ws=P, ws_bytes=BIG):
    return lib.stein_predict_glm(theta, n, d, kind, output, w_col, F, X, y, batch, tau, pred, mean, var, lpd, ws, ws_bytes, None)


def _bnn(lib, n=4, d=40, n_in=2, H=3, cols=(0, 6, 9, 12, 13, 14), output=_lib.PRED_LINK, batch=5, theta=P, X=P, y=P,
         pred=P, mean=P, var=P, lpd=P, ws=P, ws_bytes=BIG):
    cols = None if cols is None else (ctypes.c_int64 * 6)(*cols)
    return lib.stein_predict_bnn(theta, n, d, n_in, H, cols, output, X, y, batch, pred, mean, var, lpd, ws, ws_bytes, None)


def test_every_refusal_comes_back_before_any_launch():
    lib = _lib.load()
    err = lib.stein_last_error
    for call in (_glm, _bnn):
        assert call(lib, theta=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, X=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, pred=None, mean=None, var=None, lpd=None) == _lib.E_BADARG and b"no output" in err()
        assert call(lib, y=None) == _lib.E_BADARG and b"lpd needs y" in err()
        assert call(lib, output=2) == _lib.E_BADARG and b"output" in err()
        for summary in ("mean", "var", "lpd"):             # any one summary needs the workspace
            only = dict(pred=None, mean=None, var=None, lpd=None)
            only[summary] = P
            assert call(lib, ws=None, ws_bytes=0, **only) == _lib.E_WORKSPACE and b"workspace" in err()
            need = pc.workspace_bytes(4, 5)
            assert call(lib, ws_bytes=need - 1, **only) == _lib.E_WORKSPACE and b"too small" in err()
        for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(n=1 << 31), dict(batch=1 << 31),
                    dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):     # n and batch stop at 2^30: int indices in the kernels
            assert call(lib, **bad) == _lib.E_SHAPE, bad
    assert _bnn(lib, cols=None) == _lib.E_BADARG and b"NULL" in err()
    assert _glm(lib, kind=2) == _lib.E_BADARG and b"kind" in err()
    assert _glm(lib, F=0) == _lib.E_SHAPE
    assert _glm(lib, w_col=6, F=3) == _lib.E_SHAPE and b"do not fit" in err()           # the weights run past d
    assert _glm(lib, w_col=-1) == _lib.E_SHAPE
    assert _glm(lib, d=1030, F=1025) == _lib.E_UNSUPPORTED and b"1024 features" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert _glm(lib, kind=_lib.GLM_LINEAR, tau=tau) == _lib.E_BADARG and b"noise_precision" in err()
    assert _bnn(lib, n_in=0) == _lib.E_SHAPE and _bnn(lib, H=0) == _lib.E_SHAPE
    assert _bnn(lib, n_in=5, cols=(0, 15, 18, 21, 22, 23)) == _lib.E_UNSUPPORTED and b"input features" in err()
    assert _bnn(lib, d=5000, n_in=1, H=1025, cols=(0, 1025, 2050, 3075, 3076, 3077)) == _lib.E_UNSUPPORTED and b"1024 hidden" in err()
    assert _bnn(lib, cols=(0, 5, 9, 12, 13, 14)) == _lib.E_SHAPE and b"overlap" in err()        # b1 inside w1
    assert _bnn(lib, cols=(0, 6, 9, 12, 13, 13)) == _lib.E_SHAPE and b"overlap" in err()        # two scalars share a column
    assert _bnn(lib, d=14) == _lib.E_SHAPE and b"does not fit" in err()                         # log_gamma at column d
    assert _bnn(lib, cols=(-1, 6, 9, 12, 13, 14)) == _lib.E_SHAPE


def test_workspace_bytes_is_monotone_and_has_no_d():
    assert _lib._SIGNATURES["stein_predict_workspace_bytes"][:2] == [_lib._i64, _lib._i64]   # (n, batch, out): no d
    assert len(_lib._SIGNATURES["stein_predict_workspace_bytes"]) == 3
    ns = (1, 15, 16, 17, 100, 1023, 1024, 1025, 5000, 16384, 1 << 20)
    bs = (1, 20, 200, 255, 256, 257, 2304, 2305, 4000, 100000)
    table = [[_lib.predict_workspace_bytes(n, b) for b in bs] for n in ns]
    for i, n in enumerate(ns):
        for j, b in enumerate(bs):
            assert table[i][j] == pc.workspace_bytes(n, b) > 0
            rt, slices, per = pc.plan(n, b)
            assert slices * pc.PR_STATE * 4 * b <= table[i][j]          # what a call writes fits
            assert table[i][j] <= 20 * min(pc.PR_SLICE_CAP * b, pc.PR_TARGET_WGS * pc.PR_ROWS + b)   # small: O(slices * batch)
            if i:
                assert table[i][j] >= table[i - 1][j]
            if j:
                assert table[i][j] >= table[i][j - 1]
    import pytest
    for bad in ((0, 5), (5, 0), (1 << 31, 5), ((1 << 30) + 1, 5), (5, (1 << 30) + 1)):
        with pytest.raises(ValueError):
            _lib.predict_workspace_bytes(*bad)
