"""CPU: the C ABI of the weighted class summaries (include/steinhip.h: stein_predict_softmax_weighted,
stein_predict_bnn_class_weighted and their workspace sizes) -- the declarations and the ctypes signatures agree, the refusals
come back in the order of the unweighted calls with weights among the NULL pointers and ess counting as an output and as a
summary, and the workspace is the unweighted size behind the weight pass's header, 8-byte aligned and monotone.  No call here
passes the checks, so none reaches a launch, with or without a GPU."""
import ctypes
import os
import re
import sys

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_weighted_cases as cwc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = (ctypes.c_double * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer, 8-byte aligned: never dereferenced, every call below is refused
ODD = ctypes.c_void_p(P.value + 4)          # ... and one that is not
BIG = 1 << 40
_CTYPE = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
NAMES = {"softmax": ("stein_predict_softmax", "stein_predict_softmax_weighted", "stein_predict_softmax_weighted_workspace_bytes"),
         "netclass": ("stein_predict_bnn_class", "stein_predict_bnn_class_weighted", "stein_predict_bnn_class_weighted_workspace_bytes")}


def _declaration(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declarations_and_signatures_agree():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for plain, weighted, size in NAMES.values():
        for name in (weighted, size):
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
        # the unweighted call's list with weights ahead of the outputs and ess behind them
        want = _declaration(text, plain)
        want.insert(want.index("float* pred"), "const double* weights")
        want.insert(want.index("int32_t* label") + 1, "double* ess")
        assert _declaration(text, weighted) == want
    for phrase in ("Lane weights", "Power-of-two scaling", "Zero weight", "Bad weights", "Bad labels", "Deterministic", "Summation",
                   "8-byte aligned", "ess counting as a requested output and as a summary"):
        assert phrase in text, phrase


def _softmax(lib, n=4, d=None, output=_lib.PRED_MEAN, w_col=0, F=5, C=3, batch=6, theta=P, X=P, labels=P, weights=P, pred=P, prob=P,
             lpd=P, ent=P, label=P, ess=P, ws=P, ws_bytes=BIG):
    d = w_col + F * C if d is None else d
    return lib.stein_predict_softmax_weighted(theta, n, d, output, w_col, F, C, X, labels, batch, weights, pred, prob, lpd, ent, label,
                                              ess, ws, ws_bytes, None)


def _netclass(lib, n=4, d=None, output=_lib.PRED_MEAN, F=5, H=6, C=3, batch=6, theta=P, cols="fit", X=P, labels=P, weights=P, pred=P,
              prob=P, lpd=P, ent=P, label=P, ess=P, ws=P, ws_bytes=BIG, w_col=0):
    at = [w_col, w_col + F * H, w_col + F * H + H, w_col + F * H + H + H * C, -1]
    d = at[3] + C if d is None else d
    cols = (ctypes.c_int64 * 5)(*at) if cols == "fit" else cols
    return lib.stein_predict_bnn_class_weighted(theta, n, d, output, F, H, C, cols, X, labels, batch, weights, pred, prob, lpd, ent,
                                                label, ess, ws, ws_bytes, None)


CALLS = {"softmax": _softmax, "netclass": _netclass}


def test_the_refusals_in_the_unweighted_calls_order():
    lib = _lib.load()
    err = lib.stein_last_error
    for model, call in CALLS.items():
        size = getattr(_lib, "predict_%s_weighted_workspace_bytes" % ("softmax" if model == "softmax" else "bnn_class"))
        # NULL pointers, weights among them
        for k in ("theta", "X", "weights") + (("cols",) if model == "netclass" else ()):
            assert call(lib, **{k: None}) == _lib.E_BADARG and b"NULL" in err(), (model, k)
        # no output: ess counts, so it alone is an output
        none = dict(pred=None, prob=None, lpd=None, ent=None, label=None)
        assert call(lib, ess=None, **none) == _lib.E_BADARG and b"no output" in err() and b"ess" in err(), model
        assert call(lib, ws=None, ws_bytes=0, **none) == _lib.E_WORKSPACE, model       # ess alone: legal, and it needs the workspace
        assert call(lib, weights=None, ess=None, **none) == _lib.E_BADARG and b"NULL" in err()
        # lpd without labels, a bad output
        assert call(lib, labels=None) == _lib.E_BADARG and b"lpd needs labels" in err(), model
        assert call(lib, ess=None, **none, labels=None) == _lib.E_BADARG and b"no output" in err()
        assert call(lib, output=2) == _lib.E_BADARG and b"output" in err(), model
        assert call(lib, labels=None, output=2) == _lib.E_BADARG and b"lpd needs labels" in err()
        # shape, domain, fit
        for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(F=0), dict(C=0), dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
            assert call(lib, **bad) == _lib.E_SHAPE, (model, bad)
        assert call(lib, output=2, n=0) == _lib.E_BADARG
        assert call(lib, C=33) == _lib.E_UNSUPPORTED and b"more than 32 classes" in err(), model
        assert call(lib, C=1) == _lib.E_UNSUPPORTED and b"fewer than 2 classes" in err(), model
        assert call(lib, C=33, n=0) == _lib.E_SHAPE
        fit = call(lib, d=14)
        assert fit == _lib.E_SHAPE and (b"do not fit" in err() or b"does not fit" in err()), model
        assert call(lib, w_col=-1) == _lib.E_SHAPE
        assert call(lib, C=33, d=14) == _lib.E_UNSUPPORTED
        # the workspace: missing, too small, misaligned; behind everything else
        need = size(4, 6, 3)
        assert call(lib, ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"weighted_workspace_bytes" in err(), model
        assert call(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE and b"too small" in err(), model
        assert call(lib, ws=ODD, ws_bytes=need) == _lib.E_WORKSPACE and b"8-byte aligned" in err(), model
        assert call(lib, ws=ODD, ws_bytes=need - 1) == _lib.E_WORKSPACE and b"too small" in err(), model
        assert call(lib, d=14, ws=None, ws_bytes=0) == _lib.E_SHAPE
        assert call(lib, C=33, ws=None, ws_bytes=0) == _lib.E_UNSUPPORTED
        # the unweighted size does not do
        plain = getattr(_lib, "predict_%s_workspace_bytes" % ("softmax" if model == "softmax" else "bnn_class"))(4, 6, 3)
        assert plain < need and call(lib, ws_bytes=plain) == _lib.E_WORKSPACE


def test_the_workspace_size_calls_refusals():
    lib = _lib.load()
    err = lib.stein_last_error
    size = ctypes.c_size_t(0)
    for _, _, name in NAMES.values():
        fn = getattr(lib, name)
        assert fn(4, 6, 33, ctypes.byref(size)) == _lib.E_UNSUPPORTED and b"32 classes" in err()
        assert fn(4, 6, 1, ctypes.byref(size)) == _lib.E_UNSUPPORTED
        assert fn(4, 6, 3, None) == _lib.E_BADARG
        assert fn(0, 6, 3, ctypes.byref(size)) == _lib.E_SHAPE
        assert fn(4, (1 << 30) + 1, 3, ctypes.byref(size)) == _lib.E_SHAPE


def test_the_workspace_formula_and_its_monotonicity():
    for model in cwc.MODELS:
        stem = "softmax" if model == "softmax" else "bnn_class"
        weighted = getattr(_lib, "predict_%s_weighted_workspace_bytes" % stem)
        plain = getattr(_lib, "predict_%s_workspace_bytes" % stem)
        last = 0
        for n, B, C in ((1, 1, 2), (16, 1, 2), (17, 1, 2), (17, 300, 2), (40, 300, 2), (16384, 4000, 2), (1 << 20, 1 << 20, 2),
                        (17, 300, 7), (16384, 4000, 7), (16384, 4000, 32), (1 << 20, 1 << 20, 32)):
            got = weighted(n, B, C)
            slices = min(-(-n // 16), 1024)
            assert got == 8 * (2 + 3 * slices) + plain(n, B, C) == cwc.workspace_bytes(model, n, B, C), (model, n, B, C)
            assert got % 8 == 0                            # the states behind the header stay 4-byte aligned, the header 8
            if C == 2:
                assert got >= last
                last = got
        # monotone in n and in batch over a sweep, not only along the list above; independent of d by its arguments
        for C in (2, 7, 32):
            for B in (1, 255, 256, 257, 4000, 1 << 19, (1 << 19) + 1):
                sizes = [weighted(n, B, C) for n in (1, 15, 16, 17, 31, 32, 33, 16383, 16384, 16385, 1 << 20)]
                assert sizes == sorted(sizes), (model, C, B)
            for n in (1, 16, 17, 16384, 1 << 20):
                sizes = [weighted(n, B, C) for B in (1, 2, 255, 256, 257, 511, 512, 513, 4000, 1 << 19, (1 << 19) + 1, 1 << 20)]
                assert sizes == sorted(sizes), (model, C, n)
