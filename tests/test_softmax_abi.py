"""CPU: the C ABI of the softmax-regression entry points (include/steinhip.h: stein_score_softmax, stein_predict_softmax,
stein_predict_softmax_workspace_bytes) -- the declarations and the ctypes signatures agree, every refusal of the domain
comes back with its code and a message that names the limit, and the other refusals come back in the order the header
states.  No call here passes the checks, so none reaches a launch, with or without a GPU."""
import ctypes
import os
import re

from stein_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = (ctypes.c_float * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer: never dereferenced, every call below is refused before a launch
BIG = 1 << 40
_CTYPE = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


def _declaration(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declarations_and_signatures_agree():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for name in ("stein_score_softmax", "stein_predict_softmax", "stein_predict_softmax_workspace_bytes"):
        args = _declaration(text, name)
        sig = _lib._SIGNATURES[name]
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and len(args) == len(sig), name
        for arg, ct in zip(args, sig):
            if arg.startswith("size_t*"):
                assert ct == ctypes.POINTER(ctypes.c_size_t), (name, arg)
            elif "*" in arg:
                assert ct == ctypes.c_void_p, (name, arg)
            else:
                assert ct == _CTYPE[arg.rsplit(" ", 1)[0]], (name, arg)
    # stein_score_glm's list with n_classes behind n_feats, labels for y and no kind
    glm = [a for a in _declaration(text, "stein_score_glm") if a != "int kind"]
    glm.insert(glm.index("int64_t n_feats") + 1, "int64_t n_classes")
    glm[glm.index("const float* y")] = "const int32_t* labels"
    assert _declaration(text, "stein_score_softmax") == glm
    assert "2 <= n_classes <= 32" in text and "1 <= n_feats <= 1024" in text and "n_feats * n_classes <= 16384" in text
    assert "4 (n_classes + 2)" in text


def _score(lib, n=4, d=None, w_col=0, F=5, C=3, alpha_col=-1, batch=6, theta=P, X=P, labels=P, score=P):
    d = w_col + F * C + (1 if alpha_col >= 0 else 0) if d is None else d
    return lib.stein_score_softmax(theta, n, d, w_col, F, C, alpha_col, X, labels, batch, 1.0, 1.0, 0.01, score, None)


def _predict(lib, n=4, d=None, output=_lib.PRED_MEAN, w_col=0, F=5, C=3, batch=6, theta=P, X=P, labels=P, pred=P, prob=P, lpd=P,
             ent=P, label=P, ws=P, ws_bytes=BIG):
    d = w_col + F * C if d is None else d
    return lib.stein_predict_softmax(theta, n, d, output, w_col, F, C, X, labels, batch, pred, prob, lpd, ent, label, ws, ws_bytes, None)


def test_every_refusal_of_the_domain_names_its_limit():
    lib = _lib.load()
    err = lib.stein_last_error
    for call in (_score, _predict):
        assert call(lib, C=1) == _lib.E_UNSUPPORTED and b"fewer than 2 classes" in err()
        assert call(lib, C=33) == _lib.E_UNSUPPORTED and b"more than 32 classes" in err()
        assert call(lib, F=1025, C=2) == _lib.E_UNSUPPORTED and b"more than 1024 features" in err()
        for F, C in ((565, 29), (964, 17), (1024, 17), (513, 32)):      # 565 * 29 = 16385, and the next products up
            assert F * C > 16384 and F <= 1024
            assert call(lib, F=F, C=C) == _lib.E_UNSUPPORTED, (F, C)
            assert b"16384" in err() and b"n_feats * n_classes" in err(), (F, C)
        assert call(lib, F=565, C=29) == _lib.E_UNSUPPORTED and 565 * 29 == 16385      # F C = 16385 itself
        assert call(lib, F=512, C=32, d=8) == _lib.E_SHAPE                              # the largest member is no refusal of the domain
    size = ctypes.c_size_t(0)
    assert lib.stein_predict_softmax_workspace_bytes(4, 6, 33, ctypes.byref(size)) == _lib.E_UNSUPPORTED and b"32 classes" in err()
    assert lib.stein_predict_softmax_workspace_bytes(4, 6, 1, ctypes.byref(size)) == _lib.E_UNSUPPORTED
    assert lib.stein_predict_softmax_workspace_bytes(4, 6, 3, None) == _lib.E_BADARG
    assert lib.stein_predict_softmax_workspace_bytes(0, 6, 3, ctypes.byref(size)) == _lib.E_SHAPE


def test_the_scores_other_refusals():
    lib = _lib.load()
    err = lib.stein_last_error
    for k in ("theta", "X", "labels", "score"):
        assert _score(lib, **{k: None}) == _lib.E_BADARG and b"NULL" in err(), k
    for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(F=0), dict(C=0), dict(n=1 << 31), dict(batch=1 << 31)):
        assert _score(lib, **bad) == _lib.E_SHAPE, bad
    assert _score(lib, d=14) == _lib.E_SHAPE and b"do not fit" in err()                  # 15 weights
    assert _score(lib, w_col=1, d=15) == _lib.E_SHAPE
    assert _score(lib, w_col=-1) == _lib.E_SHAPE
    assert _score(lib, alpha_col=15, d=15) == _lib.E_SHAPE                               # the alpha column past d
    assert _score(lib, alpha_col=7, d=16) == _lib.E_SHAPE and b"log-alpha" in err()      # ... inside the weights
    assert _score(lib, alpha_col=0, w_col=0, d=16) == _lib.E_SHAPE
    assert _score(lib, C=33, d=1) == _lib.E_UNSUPPORTED                                  # the domain ahead of the fit


def test_the_predictive_calls_other_refusals_in_the_headers_order():
    lib = _lib.load()
    err = lib.stein_last_error
    assert _predict(lib, theta=None) == _lib.E_BADARG and b"NULL" in err()
    assert _predict(lib, X=None) == _lib.E_BADARG and b"NULL" in err()
    none = dict(pred=None, prob=None, lpd=None, ent=None, label=None)
    assert _predict(lib, **none) == _lib.E_BADARG and b"no output" in err()
    assert _predict(lib, labels=None) == _lib.E_BADARG and b"lpd needs labels" in err()
    assert _predict(lib, output=2) == _lib.E_BADARG and b"output" in err()
    for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(F=0), dict(C=0), dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
        assert _predict(lib, **bad) == _lib.E_SHAPE, bad
    assert _predict(lib, d=14) == _lib.E_SHAPE and b"do not fit" in err()
    assert _predict(lib, w_col=-1) == _lib.E_SHAPE
    assert _predict(lib, ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"workspace" in err()
    assert _predict(lib, ws_bytes=8) == _lib.E_WORKSPACE and b"too small" in err()
    need = _lib.predict_softmax_workspace_bytes(4, 6, 3)
    assert need == 1 * 6 * 5 * 4 and _predict(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    # the order: the shared checks ahead of the domain, the domain ahead of the fit and of the workspace
    assert _predict(lib, labels=None, C=33) == _lib.E_BADARG
    assert _predict(lib, C=33, ws=None, ws_bytes=0) == _lib.E_UNSUPPORTED
    assert _predict(lib, C=1, ws_bytes=0) == _lib.E_UNSUPPORTED
    assert _predict(lib, F=1025, C=2, d=8, ws_bytes=0) == _lib.E_UNSUPPORTED
    assert _predict(lib, F=565, C=29, ws_bytes=0) == _lib.E_UNSUPPORTED
    assert _predict(lib, d=14, ws_bytes=0) == _lib.E_SHAPE
    # a call that asks for pred alone needs no workspace and no labels: it passes every check that comes before the launch,
    # so it is not made here; lpd = NULL lifts the need for labels
    assert _predict(lib, labels=None, lpd=None, ws_bytes=0) == _lib.E_WORKSPACE


def test_the_workspace_formula():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import softmax_cases as smc
    last = 0
    for n, B, C in ((1, 1, 2), (16, 1, 2), (17, 1, 2), (17, 300, 7), (40, 300, 7), (16384, 4000, 7), (16384, 4000, 32), (1 << 20, 1 << 20, 32)):
        got = _lib.predict_softmax_workspace_bytes(n, B, C)
        assert got == smc.predict_workspace_bytes(n, B, C), (n, B, C)
        assert got >= smc.predict_plan(5, C, n, B)["slices"] * B * (C + 2) * 4
        if C == 2:
            assert got >= last
            last = got
