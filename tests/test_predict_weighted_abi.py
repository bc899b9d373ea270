"""CPU: the C ABI of the weighted predictive producers (include/steinhip.h, csrc/stein_predict.hip) -- the declarations are
exported, every refusal of the unweighted calls comes back from the weighted ones with its code and message and in the same
order, NULL weights are refused, ess alone counts as a requested output and as a summary that needs the workspace, and the
workspace size is monotone in both of its arguments and has no others.  No call here passes the checks, so none reaches a
launch, with or without a GPU."""
import ctypes
import os
import re
import sys

import pytest

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stein_predict_weighted_workspace_bytes", "stein_predict_glm_weighted", "stein_predict_bnn_weighted")


def test_declarations_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    # the weighted signatures are the unweighted ones with `weights` ahead of pred and `ess` behind lpd
    for base in ("stein_predict_glm", "stein_predict_bnn"):
        plain, weighted = _lib._SIGNATURES[base], _lib._SIGNATURES[base + "_weighted"]
        at = len(plain) - 7                                # pred, mean, var, lpd, workspace, ws_bytes, stream
        assert weighted == plain[:at] + [_lib._vp] + plain[at:at + 4] + [_lib._vp] + plain[at + 4:]
    from stein_amd.predict import BnnPredict, GlmPredict
    assert callable(GlmPredict.weighted_summary) and callable(BnnPredict.weighted_summary)


_BUF = (ctypes.c_double * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer, 8-byte aligned: never dereferenced, every call below is refused
BIG = 1 << 30


def _glm(lib, n=4, d=8, kind=_lib.GLM_LOGISTIC, output=_lib.PRED_LINK, w_col=0, F=3, batch=5, tau=1.0, theta=P, X=P, y=P,
         weights=P, pred=P, mean=P, var=P, lpd=P, ess=P, ws=P, ws_bytes=BIG):
    return lib.stein_predict_glm_weighted(theta, n, d, kind, output, w_col, F, X, y, batch, tau, weights, pred, mean, var, lpd,
                                          ess, ws, ws_bytes, None)


def _bnn(lib, n=4, d=40, n_in=2, H=3, cols=(0, 6, 9, 12, 13, 14), output=_lib.PRED_LINK, batch=5, theta=P, X=P, y=P,
         weights=P, pred=P, mean=P, var=P, lpd=P, ess=P, ws=P, ws_bytes=BIG):
    cols = None if cols is None else (ctypes.c_int64 * 6)(*cols)
    return lib.stein_predict_bnn_weighted(theta, n, d, n_in, H, cols, output, X, y, batch, weights, pred, mean, var, lpd, ess,
                                          ws, ws_bytes, None)


NONE = dict(pred=None, mean=None, var=None, lpd=None, ess=None)


def test_every_refusal_comes_back_before_any_launch():
    lib = _lib.load()
    err = lib.stein_last_error
    for call in (_glm, _bnn):
        assert call(lib, theta=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, X=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, weights=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, **NONE) == _lib.E_BADARG and b"no output" in err() and b"ess" in err()
        assert call(lib, y=None) == _lib.E_BADARG and b"lpd needs y" in err()
        assert call(lib, output=2) == _lib.E_BADARG and b"output" in err()
        need = pwc.workspace_bytes(4, 5)
        for summary in ("mean", "var", "lpd", "ess"):      # any one summary, ess among them, needs the workspace
            only = dict(NONE)
            only[summary] = P
            assert call(lib, ws=None, ws_bytes=0, **only) == _lib.E_WORKSPACE and b"workspace" in err()
            assert call(lib, ws_bytes=need - 1, **only) == _lib.E_WORKSPACE and b"too small" in err()
            assert call(lib, ws_bytes=pc.workspace_bytes(4, 5), **only) == _lib.E_WORKSPACE    # the unweighted size is not enough
            odd = ctypes.c_void_p(P.value + 4)
            assert call(lib, ws=odd, **only) == _lib.E_WORKSPACE and b"aligned" in err()
        for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(n=1 << 31), dict(batch=1 << 31),
                    dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
            assert call(lib, **bad) == _lib.E_SHAPE, bad
        # the order of the unweighted calls: NULL pointers, then no output, then lpd without y, then output, then shapes
        assert call(lib, weights=None, **NONE) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, y=None, output=2, **dict(NONE, lpd=P)) == _lib.E_BADARG and b"lpd needs y" in err()
        assert call(lib, output=2, n=0) == _lib.E_BADARG and b"output" in err()
        assert call(lib, n=0, ws=None, ws_bytes=0) == _lib.E_SHAPE
    assert _bnn(lib, cols=None) == _lib.E_BADARG and b"NULL" in err()
    assert _glm(lib, kind=2) == _lib.E_BADARG and b"kind" in err()
    assert _glm(lib, F=0) == _lib.E_SHAPE
    assert _glm(lib, w_col=6, F=3) == _lib.E_SHAPE and b"do not fit" in err()
    assert _glm(lib, w_col=-1) == _lib.E_SHAPE
    assert _glm(lib, d=1030, F=1025) == _lib.E_UNSUPPORTED and b"1024 features" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert _glm(lib, kind=_lib.GLM_LINEAR, tau=tau) == _lib.E_BADARG and b"noise_precision" in err()
    assert _bnn(lib, n_in=0) == _lib.E_SHAPE and _bnn(lib, H=0) == _lib.E_SHAPE
    assert _bnn(lib, n_in=5, cols=(0, 15, 18, 21, 22, 23)) == _lib.E_UNSUPPORTED and b"input features" in err()
    assert _bnn(lib, d=5000, n_in=1, H=1025, cols=(0, 1025, 2050, 3075, 3076, 3077)) == _lib.E_UNSUPPORTED and b"1024 hidden" in err()
    assert _bnn(lib, cols=(0, 5, 9, 12, 13, 14)) == _lib.E_SHAPE and b"overlap" in err()
    assert _bnn(lib, cols=(0, 6, 9, 12, 13, 13)) == _lib.E_SHAPE and b"overlap" in err()
    assert _bnn(lib, d=14) == _lib.E_SHAPE and b"does not fit" in err()
    assert _bnn(lib, cols=(-1, 6, 9, 12, 13, 14)) == _lib.E_SHAPE


def test_workspace_bytes_is_monotone_and_has_no_d():
    sig = _lib._SIGNATURES["stein_predict_weighted_workspace_bytes"]
    assert sig[:2] == [_lib._i64, _lib._i64] and len(sig) == 3                     # (n, batch, out): no d
    ns = (1, 15, 16, 17, 100, 1023, 1024, 1025, 5000, 16384, 17403, 1 << 20)
    bs = (1, 20, 200, 255, 256, 257, 2304, 2305, 4000, 100000)
    table = [[_lib.predict_weighted_workspace_bytes(n, b) for b in bs] for n in ns]
    for i, n in enumerate(ns):
        for j, b in enumerate(bs):
            assert table[i][j] == pwc.workspace_bytes(n, b)
            plain = _lib.predict_workspace_bytes(n, b)
            slices_bound = min(-(-n // pc.PR_PASS), pc.PR_SLICE_CAP)
            assert table[i][j] == plain + 8 * (pwc.PW_HEAD + 3 * slices_bound)    # the unweighted size plus the slice sums
            head, states = pwc.used_bytes(n, b)
            assert head % 8 == 0 and head + states <= table[i][j]                 # what a call writes fits
            if i:
                assert table[i][j] >= table[i - 1][j]
            if j:
                assert table[i][j] >= table[i][j - 1]
    for bad in ((0, 5), (5, 0), (1 << 31, 5), ((1 << 30) + 1, 5), (5, (1 << 30) + 1)):
        with pytest.raises(ValueError):
            _lib.predict_weighted_workspace_bytes(*bad)
    lib = _lib.load()
    assert lib.stein_predict_weighted_workspace_bytes(4, 5, None) == _lib.E_BADARG
