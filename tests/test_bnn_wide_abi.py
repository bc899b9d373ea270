"""CPU: the C ABI of the wide network entry points (include/steinhip.h: stein_score_bnn_wide, stein_predict_bnn_wide,
stein_predict_bnn_wide_weighted) -- the declarations are exported with the argument lists of their narrow twins, every
refusal of the domain comes back with its code and a message that names the limit, the twins' own refusals come back from
the wide names too, in the twins' order, and the narrow names still refuse five input features.  No call here passes the
checks, so none reaches a launch, with or without a GPU."""
import ctypes
import os
import re

from stein_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"stein_score_bnn_wide": "stein_score_bnn", "stein_predict_bnn_wide": "stein_predict_bnn",
         "stein_predict_bnn_wide_weighted": "stein_predict_bnn_weighted"}


def _declaration(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_declarations_are_exported_with_the_twins_argument_lists():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for wide, narrow in TWINS.items():
        assert _declaration(text, wide) == _declaration(text, narrow), wide
        assert hasattr(lib, wide) and wide in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[wide] == _lib._SIGNATURES[narrow], wide
    assert "1 <= n_in <= 128" in text and "n_in * n_hidden <= 16384" in text


_BUF = (ctypes.c_float * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer: never dereferenced, every call below is refused before a launch
BIG = 1 << 30


def _cols(n_in, H, at=0):
    """the six blocks back to back from column `at` -> (cols, the first column past them)"""
    sizes = (n_in * H, H, H, 1, 1, 1)
    cols, c = [], at
    for s in sizes:
        cols.append(c)
        c += s
    return tuple(cols), c


def _score(lib, name="stein_score_bnn_wide", n=4, d=None, n_in=5, H=3, cols="fit", batch=5, n_train=10.0, theta=P, X=P, y=P, score=P):
    fit, end = _cols(n_in, H)
    cols = fit if cols == "fit" else cols
    d = end if d is None else d
    cols = None if cols is None else (ctypes.c_int64 * 6)(*cols)
    return getattr(lib, name)(theta, n, d, n_in, H, cols, X, y, batch, n_train, 1.0, 0.01, score, None)


def _predict(lib, name="stein_predict_bnn_wide", n=4, d=None, n_in=5, H=3, cols="fit", output=_lib.PRED_LINK, batch=5, theta=P,
             X=P, y=P, pred=P, mean=P, var=P, lpd=P, ws=P, ws_bytes=BIG, weights=P, ess=P):
    fit, end = _cols(n_in, H)
    cols = fit if cols == "fit" else cols
    d = end if d is None else d
    cols = None if cols is None else (ctypes.c_int64 * 6)(*cols)
    w, e = ((weights,), (ess,)) if name.endswith("_weighted") else ((), ())
    return getattr(lib, name)(theta, n, d, n_in, H, cols, output, X, y, batch, *w, pred, mean, var, lpd, *e, ws, ws_bytes, None)


def _weighted(lib, **kw):
    return _predict(lib, name="stein_predict_bnn_wide_weighted", **kw)


def test_every_refusal_of_the_domain_names_its_limit():
    lib = _lib.load()
    err = lib.stein_last_error
    for call in (_score, _predict, _weighted):
        assert call(lib, n_in=129, H=1) == _lib.E_UNSUPPORTED and b"128 input features" in err()
        assert call(lib, n_in=5, H=1025) == _lib.E_UNSUPPORTED and b"1024 hidden units" in err()
        # n_in * n_hidden = 16385 = 5 * 29 * 113: the two factor pairs inside both of the other limits, and the next products up
        for n_in, H in ((29, 565), (113, 145), (17, 964), (128, 129), (16, 1024 + 1)):
            assert n_in * H > 16384
            code = call(lib, n_in=n_in, H=H)
            assert code == _lib.E_UNSUPPORTED, (n_in, H)
            assert (b"1024 hidden units" in err()) if H > 1024 else (b"16384" in err() and b"n_in * n_hidden" in err()), (n_in, H)
        assert 29 * 565 == 113 * 145 == 16385


def test_the_twins_refusals_come_back_from_the_wide_names():
    lib = _lib.load()
    err = lib.stein_last_error
    # score: NULL pointers, shapes, cols fit and overlap, n_train
    for k in ("theta", "X", "y", "score", "cols"):
        assert _score(lib, **{k: None}) == _lib.E_BADARG and b"NULL" in err(), k
    for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(n_in=0), dict(H=0), dict(n=1 << 31), dict(batch=1 << 31)):
        assert _score(lib, **bad) == _lib.E_SHAPE, bad
    fit, end = _cols(5, 3)
    assert _score(lib, d=end - 1) == _lib.E_SHAPE and b"does not fit" in err()
    assert _score(lib, cols=(0, 14) + fit[2:]) == _lib.E_SHAPE and b"overlap" in err()           # b1 inside w1
    assert _score(lib, cols=fit[:5] + (fit[4],)) == _lib.E_SHAPE and b"overlap" in err()         # two scalars share a column
    assert _score(lib, cols=(-1,) + fit[1:]) == _lib.E_SHAPE
    for bad in (0.0, -1.0, float("nan")):
        assert _score(lib, n_train=bad) == _lib.E_BADARG and b"n_train" in err()
    assert _score(lib, n_in=129, H=1, n_train=0.0) == _lib.E_UNSUPPORTED                          # the domain ahead of n_train, as in the twin
    # predictive: the twins' list, in their order
    for call in (_predict, _weighted):
        assert call(lib, theta=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, X=None) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, cols=None) == _lib.E_BADARG and b"NULL" in err()
        none = dict(pred=None, mean=None, var=None, lpd=None)
        if call is _weighted:
            none["ess"] = None
        assert call(lib, **none) == _lib.E_BADARG and b"no output" in err()
        assert call(lib, y=None) == _lib.E_BADARG and b"lpd needs y" in err()
        assert call(lib, output=2) == _lib.E_BADARG and b"output" in err()
        for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(H=0), dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
            assert call(lib, **bad) == _lib.E_SHAPE, bad
        assert call(lib, n_in=0) == _lib.E_SHAPE
        assert call(lib, d=end - 1) == _lib.E_SHAPE and b"does not fit" in err()
        assert call(lib, cols=(0, 14) + fit[2:]) == _lib.E_SHAPE and b"overlap" in err()
        assert call(lib, ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"workspace" in err()
        assert call(lib, ws_bytes=8) == _lib.E_WORKSPACE and b"too small" in err()
        assert call(lib, y=None, n_in=129, H=1) == _lib.E_BADARG and b"lpd needs y" in err()     # the shared checks ahead of the domain
        assert call(lib, n_in=129, H=1, ws=None, ws_bytes=0) == _lib.E_UNSUPPORTED                # the domain ahead of the workspace
    assert _weighted(lib, weights=None) == _lib.E_BADARG and b"NULL" in err()
    odd = ctypes.c_void_p(P.value + 4)
    assert _weighted(lib, ws=odd) == _lib.E_WORKSPACE and b"8-byte aligned" in err()


def test_the_narrow_names_still_refuse_five_inputs():
    lib = _lib.load()
    err = lib.stein_last_error
    assert _score(lib, name="stein_score_bnn") == _lib.E_UNSUPPORTED and b"4 input features" in err()
    assert _predict(lib, name="stein_predict_bnn") == _lib.E_UNSUPPORTED and b"4 input features" in err()
    assert _predict(lib, name="stein_predict_bnn_weighted") == _lib.E_UNSUPPORTED and b"4 input features" in err()
    # and through the wide names four inputs meet the narrow names' own checks (the narrow code runs)
    assert _score(lib, n_in=4, H=1025) == _lib.E_UNSUPPORTED and b"1024 hidden units" in err()
    assert _predict(lib, n_in=4, H=1025) == _lib.E_UNSUPPORTED and b"1024 hidden units" in err()
    assert _score(lib, n_in=4, H=3, theta=None) == _lib.E_BADARG and _predict(lib, n_in=4, H=3, theta=None) == _lib.E_BADARG
