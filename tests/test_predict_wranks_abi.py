"""CPU: the C ABI of the weighted predictive order statistics (include/steinhip.h, csrc/stein_predict_ranks.hip) -- the
declarations are exported and bound, every refusal comes back with its code and message and in the order of the unweighted
ranks calls, the workspace sizes are 512 bytes + 76 per (row, level) and 24 per workgroup of the masses pass: independent of
d, monotone.  No call here passes the checks, so none reaches a launch, with or without a GPU."""
import ctypes
import os
import re
import sys

import pytest

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wquantile_cases as wq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stein_predict_ranks_weighted_workspace_bytes", "stein_predict_glm_ranks_weighted", "stein_predict_bnn_ranks_weighted",
         "stein_debug_predict_ranks_weighted_bits", "stein_predict_rank_masses_workspace_bytes", "stein_predict_rank_masses")


def test_declarations_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS
    assert (_lib.MASS_NORMALISED, _lib.MASS_COUNTS) == (0, 1)
    # the arguments of the ranks calls with masses (device) and levels (host doubles) in place of ranks
    for kind in ("glm", "bnn"):
        plain, weighted = _lib._SIGNATURES["stein_predict_%s_ranks" % kind], _lib._SIGNATURES["stein_predict_%s_ranks_weighted" % kind]
        at = plain.index(ctypes.POINTER(_lib._i64), 6)                                     # ranks (behind the network's cols)
        assert weighted == plain[:at] + [_lib._vp, ctypes.POINTER(_lib._dbl)] + plain[at + 1:]
    from stein_amd.predict import BnnPredict, GlmPredict
    from stein_amd.samplers import SteinSampler
    for cls in (GlmPredict, BnnPredict):
        assert callable(cls.weighted_quantiles)
    assert callable(SteinSampler.predictive_quantiles)


_BUF = (ctypes.c_double * 16)()
P = ctypes.cast(_BUF, ctypes.c_void_p)      # a host pointer: never dereferenced, every call below is refused
BIG = 1 << 30
KEEP = object()


def _levels(q):
    return None if q is None else (ctypes.c_double * len(q))(*q)


def _glm(lib, n=4, d=8, kind=_lib.GLM_LOGISTIC, output=_lib.PRED_LINK, w_col=0, F=3, batch=5, theta=P, X=P, masses=P,
         levels=(0.1, 0.9), n_levels=KEEP, out=P, ws=P, ws_bytes=BIG):
    k = (0 if levels is None else len(levels)) if n_levels is KEEP else n_levels
    return lib.stein_predict_glm_ranks_weighted(theta, n, d, kind, output, w_col, F, X, batch, masses, _levels(levels), k, out, ws,
                                                ws_bytes, None)


def _bnn(lib, n=4, d=40, n_in=2, H=3, cols=(0, 6, 9, 12, 13, 14), output=_lib.PRED_LINK, batch=5, theta=P, X=P, masses=P,
         levels=(0.1, 0.9), n_levels=KEEP, out=P, ws=P, ws_bytes=BIG):
    cols = None if cols is None else (ctypes.c_int64 * 6)(*cols)
    k = (0 if levels is None else len(levels)) if n_levels is KEEP else n_levels
    return lib.stein_predict_bnn_ranks_weighted(theta, n, d, n_in, H, cols, output, X, batch, masses, _levels(levels), k, out, ws,
                                                ws_bytes, None)


def test_every_refusal_comes_back_before_any_launch():
    lib = _lib.load()
    err = lib.stein_last_error
    nine = tuple(i / 8.0 for i in range(9))
    for call in (_glm, _bnn):
        for null in ("theta", "X", "masses", "levels", "out"):
            assert call(lib, n_levels=2, **{null: None}) == _lib.E_BADARG and b"NULL" in err(), null
        for k in (0, -1):
            assert call(lib, n_levels=k) == _lib.E_BADARG and b"n_levels" in err()
        assert call(lib, output=2) == _lib.E_BADARG and b"output" in err()
        for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(n=1 << 31), dict(batch=1 << 31),
                    dict(n=(1 << 30) + 1), dict(batch=(1 << 30) + 1)):
            assert call(lib, **bad) == _lib.E_SHAPE, bad
        assert call(lib, levels=nine) == _lib.E_UNSUPPORTED and b"8 levels" in err()
        for q in ((0.5, 1.0000001), (-1e-9, 0.5), (0.5, float("nan")), (float("inf"), 0.1)):
            assert call(lib, levels=q) == _lib.E_BADARG and b"outside [0, 1]" in err(), q
        assert call(lib, levels=(1.0, 0.0, 0.5, 0.5, 0.0), ws=None, ws_bytes=0) == _lib.E_WORKSPACE   # ends, any order, repeats
        need = wq.workspace_bytes(5, 2)
        assert call(lib, ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"workspace" in err()
        assert call(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE and b"too small" in err()
        assert call(lib, ws=ctypes.c_void_p(P.value + 4)) == _lib.E_WORKSPACE and b"aligned" in err()
        # the order: NULL pointers and n_levels < 1, the output, the shapes, the level count, the levels, the workspace
        assert call(lib, theta=None, n_levels=0) == _lib.E_BADARG and b"NULL" in err()
        assert call(lib, n_levels=0, output=2) == _lib.E_BADARG and b"n_levels" in err()
        assert call(lib, output=2, n=0) == _lib.E_BADARG and b"output" in err()
        assert call(lib, n=0, levels=nine) == _lib.E_SHAPE
        assert call(lib, levels=nine[:8] + (2.0,)) == _lib.E_UNSUPPORTED                  # nine levels, one of them bad
        assert call(lib, levels=(0.5, 2.0), ws=None, ws_bytes=0) == _lib.E_BADARG and b"outside" in err()
    # the shape and column checks of stein_predict_*: unchanged codes and messages, ahead of the level checks
    assert _bnn(lib, cols=None) == _lib.E_BADARG and b"NULL" in err()
    assert _glm(lib, kind=2) == _lib.E_BADARG and b"kind" in err()
    assert _glm(lib, F=0) == _lib.E_SHAPE
    assert _glm(lib, w_col=6, F=3) == _lib.E_SHAPE and b"do not fit" in err()
    assert _glm(lib, d=1030, F=1025) == _lib.E_UNSUPPORTED and b"1024 features" in err()
    assert _glm(lib, w_col=6, levels=nine) == _lib.E_SHAPE and b"do not fit" in err()
    assert _bnn(lib, n_in=0) == _lib.E_SHAPE and _bnn(lib, H=0) == _lib.E_SHAPE
    assert _bnn(lib, n_in=5, cols=(0, 15, 18, 21, 22, 23)) == _lib.E_UNSUPPORTED and b"input features" in err()
    assert _bnn(lib, d=5000, n_in=1, H=1025, cols=(0, 1025, 2050, 3075, 3076, 3077)) == _lib.E_UNSUPPORTED and b"1024 hidden" in err()
    assert _bnn(lib, cols=(0, 5, 9, 12, 13, 14)) == _lib.E_SHAPE and b"overlap" in err()
    assert _bnn(lib, d=14) == _lib.E_SHAPE and b"does not fit" in err()
    assert _bnn(lib, d=14, levels=nine) == _lib.E_SHAPE and b"does not fit" in err()


def test_a_forced_width_that_does_not_fit_the_cu_is_refused_before_any_launch():
    lib = _lib.load()
    err = lib.stein_last_error
    eight = tuple(i / 7.0 for i in range(8))
    try:
        for k in (1, 2, 3, 4):
            assert lib.stein_debug_predict_ranks_weighted_bits(k) == _lib.OK
        assert lib.stein_debug_predict_ranks_weighted_bits(-1) == _lib.E_BADARG
        assert lib.stein_debug_predict_ranks_weighted_bits(5) == _lib.E_BADARG
        # 4 bits, eight levels: 129 words a lane = 132 KB beside a 64 KB tile; 3 bits fit
        assert wq.glm_lds_bytes(59, 8, 4) > 160 * 1024 >= wq.glm_lds_bytes(59, 8, 3)
        assert lib.stein_debug_predict_ranks_weighted_bits(4) == _lib.OK
        assert _glm(lib, d=60, F=59, levels=eight) == _lib.E_UNSUPPORTED and b"LDS" in err()
        # behind the workspace checks, as the last refusal
        assert _glm(lib, d=60, F=59, levels=eight, ws=None, ws_bytes=0) == _lib.E_WORKSPACE
        # the network call beside 24.8 KB of its own: 132 KB + 24.8 KB fit, so its next refusal is the workspace's
        assert _bnn(lib, levels=eight, ws=None, ws_bytes=0) == _lib.E_WORKSPACE
    finally:
        assert lib.stein_debug_predict_ranks_weighted_bits(0) == _lib.OK


def test_workspace_bytes_have_no_d_and_are_monotone():
    sig = _lib._SIGNATURES["stein_predict_ranks_weighted_workspace_bytes"]
    assert sig[:3] == [_lib._i64, _lib._i64, _lib._i64] and len(sig) == 4              # (n, batch, n_levels, out): no d
    ns = (1, 16, 17, 1000, 16400, 1 << 20, 1 << 30)
    bs = (1, 20, 255, 256, 257, 4000, 100000, 1 << 30)
    for j, b in enumerate(bs):
        for r in range(1, _lib.PRED_RANKS_MAX + 1):
            got = {_lib.predict_ranks_weighted_workspace_bytes(n, b, r) for n in ns}
            assert got == {wq.workspace_bytes(b, r)}, (b, r)
            assert wq.workspace_bytes(b, r) == _lib.predict_ranks_workspace_bytes(5, b, r) + 512
            if r > 1:
                assert _lib.predict_ranks_weighted_workspace_bytes(5, b, r) > _lib.predict_ranks_weighted_workspace_bytes(5, b, r - 1)
            if j:
                assert _lib.predict_ranks_weighted_workspace_bytes(5, b, r) > _lib.predict_ranks_weighted_workspace_bytes(5, bs[j - 1], r)
    for bad in ((0, 5, 1), (5, 0, 1), (1 << 31, 5, 1), ((1 << 30) + 1, 5, 1), (5, (1 << 30) + 1, 1), (5, 5, 0), (5, 5, 9)):
        with pytest.raises(ValueError):
            _lib.predict_ranks_weighted_workspace_bytes(*bad)
    lib = _lib.load()
    assert lib.stein_predict_ranks_weighted_workspace_bytes(4, 5, 1, None) == _lib.E_BADARG
    assert lib.stein_predict_ranks_weighted_workspace_bytes(4, 5, 9, ctypes.byref(ctypes.c_size_t())) == _lib.E_UNSUPPORTED
    # the masses pass: a function of n alone
    assert _lib._SIGNATURES["stein_predict_rank_masses_workspace_bytes"] == [_lib._i64, ctypes.POINTER(_lib._sz)]
    last = 0
    for n in (1, 255, 256, 257, 1000, 65536, 65537, 1 << 20, 1 << 30):
        got = _lib.predict_rank_masses_workspace_bytes(n)
        assert got == wq.masses_workspace_bytes(n) and got >= last
        last = got
    for bad in (0, -1, (1 << 30) + 1):
        with pytest.raises(ValueError):
            _lib.predict_rank_masses_workspace_bytes(bad)
    assert lib.stein_predict_rank_masses_workspace_bytes(4, None) == _lib.E_BADARG


def test_the_masses_pass_refuses_in_order():
    lib = _lib.load()
    err = lib.stein_last_error

    def call(weights=P, n=40, mode=_lib.MASS_NORMALISED, masses=P, info=P, ws=P, ws_bytes=BIG):
        return lib.stein_predict_rank_masses(weights, n, mode, masses, info, ws, ws_bytes, None)
    for null in ("weights", "masses", "info"):
        assert call(**{null: None}) == _lib.E_BADARG and b"NULL" in err(), null
    assert call(mode=2) == _lib.E_BADARG and b"mode" in err()
    assert call(mode=-1) == _lib.E_BADARG
    for n in (0, -3, (1 << 30) + 1):
        assert call(n=n) == _lib.E_SHAPE and b"bad shape" in err()
    assert call(ws=None, ws_bytes=0) == _lib.E_WORKSPACE and b"workspace" in err()
    assert call(ws_bytes=23) == _lib.E_WORKSPACE and b"too small" in err()
    assert call(n=257, ws_bytes=47) == _lib.E_WORKSPACE
    assert call(ws=ctypes.c_void_p(P.value + 4)) == _lib.E_WORKSPACE and b"aligned" in err()
    assert call(weights=None, mode=7, n=0) == _lib.E_BADARG and b"NULL" in err()
    assert call(mode=7, n=0) == _lib.E_BADARG and b"mode" in err()
    assert call(n=0, ws=None) == _lib.E_SHAPE
