"""CPU: the C ABI of the network-classifier entry points (include/steinhip.h: stein_score_bnn_class, stein_predict_bnn_class,
stein_predict_bnn_class_workspace_bytes) -- the declarations and the ctypes signatures agree, every refusal of the domain
comes back with its code and a message that names the limit, and the other refusals come back in the order the header
states.  No call here passes the checks, so none reaches a launch, with or without a GPU."""
import ctypes
import os
import re
import sys

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_cases as ncc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = (ctypes.c_float * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer: never dereferenced, every call below is refused before a launch
BIG = 1 << 40
_CTYPE = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
NAMES = ("stein_score_bnn_class", "stein_predict_bnn_class", "stein_predict_bnn_class_workspace_bytes")


def _declaration(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declarations_and_signatures_agree():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        args = _declaration(text, name)
        sig = _lib._SIGNATURES[name]
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and len(args) == len(sig), name
        for arg, ct in zip(args, sig):
            if arg.startswith("size_t*"):
                assert ct == ctypes.POINTER(ctypes.c_size_t), (name, arg)
            elif arg.startswith("const int64_t*"):
                assert ct == ctypes.POINTER(ctypes.c_int64), (name, arg)
            elif "*" in arg:
                assert ct == ctypes.c_void_p, (name, arg)
            else:
                assert ct == _CTYPE[arg.rsplit(" ", 1)[0]], (name, arg)
    # stein_score_bnn_wide's list with n_classes behind n_hidden, labels for y and the softmax model's three scalars
    wide = _declaration(text, "stein_score_bnn_wide")
    wide.insert(wide.index("int64_t n_hidden") + 1, "int64_t n_classes")
    wide[wide.index("const float* y")] = "const int32_t* labels"
    i = wide.index("double n_train")
    wide[i:i + 3] = ["double scale", "double prior_precision", "double gamma_rate"]
    assert _declaration(text, "stein_score_bnn_class") == wide
    # stein_predict_softmax's outputs and workspace arguments
    soft, mine = _declaration(text, "stein_predict_softmax"), _declaration(text, "stein_predict_bnn_class")
    assert mine[mine.index("const float* X"):] == soft[soft.index("const float* X"):]
    assert _lib._SIGNATURES[NAMES[2]] == _lib._SIGNATURES["stein_predict_softmax_workspace_bytes"]
    for phrase in ("1 <= n_in <= 128", "2 <= n_classes <= 32", "1 <= n_hidden <= 512", "(n_in + CS) * n_hidden <= 16384",
                   "4 (n_classes + 2)", "is not taken over"):
        assert phrase in text, phrase
    from stein_amd import scores
    from stein_amd.predict import BnnClassPredict
    assert scores.BnnClassScore.wants_matrix and BnnClassPredict.classes and BnnClassPredict.wants_matrix
    assert scores.BnnClassScore.NAMES == ("model/w_1:0", "model/b_1:0", "model/w_2:0", "model/b_2:0", "model/log_lambda:0")
    access = {k: (10 * i, 10 * i + 5) for i, k in enumerate(scores.BnnClassScore.NAMES[:4])}
    assert scores.BnnClassScore.columns(access) == (0, 10, 20, 30, None)


def _cols(F, H, C, lam=True):
    at = [0, F * H, F * H + H, F * H + H + H * C, F * H + H + H * C + C]
    return (ctypes.c_int64 * 5)(*(at[:4] + [at[4] if lam else -1])), at[4] + (1 if lam else 0)


def _score(lib, n=4, d=None, F=5, H=6, C=3, cols=None, batch=7, theta=P, X=P, labels=P, score=P, lam=True, no_cols=False):
    c, need = _cols(F, H, C, lam)
    return lib.stein_score_bnn_class(theta, n, need if d is None else d, F, H, C, None if no_cols else (cols or c), X, labels, batch,
                                     1.0, 1.0, 0.01, score, None)


def _predict(lib, n=4, d=None, output=_lib.PRED_MEAN, F=5, H=6, C=3, cols=None, batch=7, theta=P, X=P, labels=P, pred=P, prob=P,
             lpd=P, ent=P, label=P, ws=P, ws_bytes=BIG, no_cols=False):
    c, need = _cols(F, H, C, False)
    return lib.stein_predict_bnn_class(theta, n, need if d is None else d, output, F, H, C, None if no_cols else (cols or c), X,
                                       labels, batch, pred, prob, lpd, ent, label, ws, ws_bytes, None)


def _just_past():
    """(n_in, H, C) with (n_in + CS) * H just past 16384: for every CS the smallest product above it over the factor pairs"""
    out = []
    for C in (2, 7, 12, 16, 20, 32):
        cs = ncc.cs_of(C)
        best = min(((F + cs) * H, F, H) for F in range(1, 129) for H in range(1, 513) if (F + cs) * H > 16384)
        out.append((best[1], best[2], C))
    return out + [(128, 103, 32), (29, 512, 4), (128, 125, 2), (54, 283, 7)]


def test_every_refusal_of_the_domain_names_its_limit():
    lib = _lib.load()
    err = lib.stein_last_error
    for call in (_score, _predict):
        assert call(lib, F=129, H=1) == _lib.E_UNSUPPORTED and b"more than 128 input features" in err()
        assert call(lib, C=1) == _lib.E_UNSUPPORTED and b"fewer than 2 classes" in err()
        assert call(lib, C=33) == _lib.E_UNSUPPORTED and b"more than 32 classes" in err()
        assert call(lib, H=513, F=1) == _lib.E_UNSUPPORTED and b"more than 512 hidden units" in err()
        for F, H, C in _just_past():
            assert not ncc.in_domain(F, H, C) and F <= 128 and H <= 512 and (F + ncc.cs_of(C)) * H > 16384
            assert call(lib, F=F, H=H, C=C) == _lib.E_UNSUPPORTED, (F, H, C)
            assert b"16384" in err() and b"(n_in + CS) * n_hidden" in err(), (F, H, C)
        assert any((F + ncc.cs_of(C)) * H == 16385 for F, H, C in _just_past())          # the first product past the limit
        # members of the domain at its edge are no refusal of the domain: they fall to the next check
        for F, H, C in ((128, 102, 32), (28, 512, 4), (8, 512, 8), (54, 100, 7), (13, 50, 3), (128, 64, 32), (4, 16, 3)):
            assert ncc.in_domain(F, H, C) and call(lib, F=F, H=H, C=C, d=8) == _lib.E_SHAPE, (F, H, C)
    size = ctypes.c_size_t(0)
    assert lib.stein_predict_bnn_class_workspace_bytes(4, 6, 33, ctypes.byref(size)) == _lib.E_UNSUPPORTED and b"32 classes" in err()
    assert lib.stein_predict_bnn_class_workspace_bytes(4, 6, 1, ctypes.byref(size)) == _lib.E_UNSUPPORTED
    assert lib.stein_predict_bnn_class_workspace_bytes(4, 6, 3, None) == _lib.E_BADARG
    assert lib.stein_predict_bnn_class_workspace_bytes(0, 6, 3, ctypes.byref(size)) == _lib.E_SHAPE


def test_the_scores_other_refusals_in_the_headers_order():
    lib = _lib.load()
    err = lib.stein_last_error
    for k in ("theta", "X", "labels", "score"):
        assert _score(lib, **{k: None}) == _lib.E_BADARG and b"NULL" in err(), k
    assert _score(lib, no_cols=True) == _lib.E_BADARG and b"NULL" in err()
    for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(F=0), dict(H=0), dict(C=0), dict(n=1 << 31), dict(batch=1 << 31)):
        assert _score(lib, **bad) == _lib.E_SHAPE, bad
    _, need = _cols(5, 6, 3)
    assert _score(lib, d=need - 1) == _lib.E_SHAPE and b"does not fit" in err()            # the log_lambda column past d
    assert _score(lib, d=need - 2, lam=False) == _lib.E_SHAPE and b"does not fit" in err()  # the last entry of b2 past d
    c, _ = _cols(5, 6, 3)
    for i, v in ((0, -1), (1, 29), (2, 35), (3, 36 + 17), (4, 3), (4, need)):                # negative, overlaps, log_lambda inside w1 / past d
        cc = (ctypes.c_int64 * 5)(*c)
        cc[i] = v
        assert _score(lib, cols=cc) == _lib.E_SHAPE and (b"overlap" in err() or b"does not fit" in err()), (i, v)
    cc = (ctypes.c_int64 * 5)(*c)
    cc[4] = -7                                                                              # any negative value: no log_lambda
    assert _score(lib, cols=cc, theta=None) == _lib.E_BADARG
    # the order: NULL ahead of the shape, the shape ahead of the domain, the domain ahead of the fit
    assert _score(lib, theta=None, n=0) == _lib.E_BADARG
    assert _score(lib, n=0, C=33) == _lib.E_SHAPE
    assert _score(lib, C=33, d=1) == _lib.E_UNSUPPORTED
    assert _score(lib, F=129, H=1, d=1) == _lib.E_UNSUPPORTED


def test_the_predictive_calls_other_refusals_in_the_headers_order():
    lib = _lib.load()
    err = lib.stein_last_error
    assert _predict(lib, theta=None) == _lib.E_BADARG and b"NULL" in err()
    assert _predict(lib, X=None) == _lib.E_BADARG and b"NULL" in err()
    assert _predict(lib, no_cols=True) == _lib.E_BADARG and b"NULL" in err()
    none = dict(pred=None, prob=None, lpd=None, ent=None, label=None)
    assert _predict(lib, **none) == _lib.E_BADARG and b"no output" in err()
    assert _predict(lib, labels=None) == _lib.E_BADARG and b"lpd needs labels" in err()
    assert _predict(lib, output=2) == _lib.E_BADARG and b"output" in err()
    for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(F=0), dict(H=0), dict(C=0), dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
        assert _predict(lib, **bad) == _lib.E_SHAPE, bad
    _, need = _cols(5, 6, 3, False)
    assert _predict(lib, d=need - 1) == _lib.E_SHAPE and b"does not fit" in err()
    c, _ = _cols(5, 6, 3, False)
    cc = (ctypes.c_int64 * 5)(*c)
    cc[2] = 31
    assert _predict(lib, cols=cc) == _lib.E_SHAPE and b"overlap" in err()
    cc = (ctypes.c_int64 * 5)(*c)
    cc[4] = 3                                                                               # the log_lambda column is not read
    assert _predict(lib, cols=cc, ws=None, ws_bytes=0) == _lib.E_WORKSPACE
    assert _predict(lib, ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"workspace" in err()
    assert _predict(lib, ws_bytes=8) == _lib.E_WORKSPACE and b"too small" in err()
    need_ws = _lib.predict_bnn_class_workspace_bytes(4, 7, 3)
    assert need_ws == 1 * 7 * 5 * 4 and _predict(lib, ws_bytes=need_ws - 1) == _lib.E_WORKSPACE
    # the order: the shared checks ahead of the domain, the domain ahead of the fit, the fit ahead of the workspace
    assert _predict(lib, labels=None, C=33) == _lib.E_BADARG
    assert _predict(lib, n=0, C=33) == _lib.E_SHAPE
    assert _predict(lib, C=33, ws=None, ws_bytes=0) == _lib.E_UNSUPPORTED
    assert _predict(lib, F=128, H=103, C=32, d=8, ws_bytes=0) == _lib.E_UNSUPPORTED
    assert _predict(lib, d=need - 1, ws_bytes=0) == _lib.E_SHAPE
    # lpd = NULL lifts the need for labels; a call that asks for pred alone would pass every check, so it is not made here
    assert _predict(lib, labels=None, lpd=None, ws_bytes=0) == _lib.E_WORKSPACE


def test_the_workspace_formula():
    last = 0
    for n, B, C in ((1, 1, 2), (16, 1, 2), (17, 1, 2), (17, 300, 7), (40, 300, 7), (16384, 4000, 7), (16384, 4000, 32), (1 << 20, 1 << 20, 32)):
        got = _lib.predict_bnn_class_workspace_bytes(n, B, C)
        assert got == ncc.predict_workspace_bytes(n, B, C) == _lib.predict_softmax_workspace_bytes(n, B, C), (n, B, C)
        assert got >= ncc.predict_plan(5, 20, C, n, B)["slices"] * B * (C + 2) * 4
        if C == 2:
            assert got >= last
            last = got
