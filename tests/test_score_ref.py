"""CPU: the vectorised fp64 score references and their fp32 allowance (tests/score_ref.py), the case tables of
tests/test_gpu_score_matrix.py (tests/score_cases.py), and the shape refusals of the two score entry points.

(a) score_ref equals the per-particle functions of oracle/score_oracle.py;
(b) a NumPy float32 evaluation with sequential accumulation stays inside the allowance on the GPU cases' own inputs, so
    the bound is known to hold for a correct fp32 implementation before a GPU sees it; the preconditions of the GPU
    tests (ambiguous-mask share, heavy rows) hold on every case;
(c) the tables name every instantiation, both sides of every dispatch edge, the chunk edges and the grid-stride caps;
(d) bad shapes are refused with their code before anything is launched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from oracle import score_oracle as so
from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_cases as sc  # noqa: E402
import score_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_AMBIGUOUS = 0.02
CPU_CASES = [c for c in sc.GLM_CASES + sc.BNN_CASES if sc.cpu_sized(c)]


def _args(case):
    return sc.glm_args(case) if case["model"] == "glm" else sc.bnn_args(case)


# ---- (a) ------------------------------------------------------------------------------------------
def _close(a, b):
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("kind", ["linear", "logistic"])
@pytest.mark.parametrize("alpha", [None, "before", "after", "last"])
def test_glm_reference_matches_the_oracle(kind, alpha):
    rng = np.random.default_rng(5)
    F, n, B = 6, 7, 11
    w_col, a_col, d = sc.glm_layout(F, alpha)
    th, X, y = rng.normal(size=(n, d)), rng.normal(size=(B, F)), rng.uniform(size=B)
    got, allow = sr.glm_score(th, kind, w_col, F, a_col, X, y, scale=2.5, prior_precision=0.75, gamma_rate=0.125)
    ref = np.zeros_like(th)
    for i in range(n):
        w = th[i, w_col:w_col + F]
        if a_col >= 0:
            gw, ga = so.logistic_score(w, th[i, a_col], X, y, 2.5, gamma_rate=0.125)
            if kind == "linear":      # the same hierarchical prior around the linear likelihood (include/steinhip.h)
                gw = so.linear_score(w, X, y, prior_precision=np.exp(th[i, a_col]), scale=2.5)
            ref[i, w_col:w_col + F], ref[i, a_col] = gw, ga
        else:
            ref[i] = so.glm_score_matrix(th[i:i + 1], kind, w_col, F, -1, X, y, scale=2.5, prior_precision=0.75)[0]
    _close(got, ref)
    live = np.zeros(d, bool)
    live[w_col:w_col + F] = True
    if a_col >= 0:
        live[a_col] = True
    assert (allow[:, live] > 0).all() and (allow[:, ~live] == 0).all() and (got[:, ~live] == 0).all()


@pytest.mark.parametrize("n_in", [1, 2, 3, 4])
def test_bnn_reference_matches_the_oracle(n_in):
    rng = np.random.default_rng(n_in)
    H, n, B = 5 + n_in, 6, 9
    cols, d = sc.bnn_layout(n_in, H, sc.BNN_BLOCK_ORDERS[n_in % 3])
    th, X, y = rng.normal(size=(n, d)), rng.uniform(size=(B, n_in)), rng.normal(size=B)
    got, allow, share = sr.bnn_score(th, n_in, H, cols, X, y, n_train=64.0, ga=1.5, gb=0.25)
    _close(got, so.bnn_score_matrix(th, n_in, H, cols, X, y, n_train=64.0, ga=1.5, gb=0.25))
    assert share == 0.0 and (allow >= 0).all()


def test_an_ambiguous_relu_mask_is_charged_its_whole_term():
    """z = b1 + x w1 = 0 exactly: either branch is a correct fp32 answer, so b1 and w1 are allowed the whole term."""
    cols, d = (0, 1, 2, 3, 4, 5), 6
    th = np.array([[0.5, -0.5, 2.0, 0.25, 0.0, 0.0], [0.5, 0.5, 2.0, 0.25, 0.0, 0.0]])
    X, y = np.array([[1.0]]), np.array([3.0])
    _, allow, share = sr.bnn_score(th, 1, 1, cols, X, y, n_train=4.0)
    term = 4.0 * abs(3.0 - 0.25) * 2.0 / 4.0                  # cg |e w2| / n_train, cg = n_train / B
    assert share == 2.0 / (2 * 6)
    assert (allow[0, :2] >= term).all() and (allow[1, :2] < 1e-4 * term).all()


def test_row_weights_drop_a_row():
    case = sc.GLM_INST[2]
    a = sc.glm_args(case)
    rw = np.ones(case["B"])
    rw[3] = 0.0
    keep = rw > 0
    got, _, _ = sc.reference(case, a, row_weight=rw)
    ref, _ = sr.glm_score(a["theta"], a["kind"], a["w_col"], a["F"], a["alpha_col"], a["X"][keep], a["y"][keep], a["scale"],
                          a["prior_precision"], a["gamma_rate"])
    _close(got, ref)
    case = sc.BNN_INST[2]
    a = sc.bnn_args(case)
    rw = np.ones(case["B"])
    rw[3] = 0.0
    keep = rw > 0
    got, _, _ = sc.reference(case, a, row_weight=rw)
    # the likelihood scale n_train / B and the B / 2 of the log_gamma entry stay those of the full batch
    c = dict(zip(sr.BNN_ORDER, a["cols"]))
    ref, _, _ = sr.bnn_score(a["theta"], a["n_in"], a["H"], a["cols"], a["X"][keep], a["y"][keep],
                             a["n_train"] * (case["B"] - 1) / case["B"], a["ga"], a["gb"])
    ref *= (case["B"] - 1) / case["B"]
    cmp = np.ones(a["d"], bool)
    cmp[c["log_gamma"]] = False
    _close(got[:, cmp], ref[:, cmp])


# ---- (b) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c["model"] + "-" + c["name"])
def test_fp32_evaluation_stays_inside_the_allowance(case):
    a = _args(case)
    ref, allow, share = sc.reference(case, a)
    assert np.isfinite(ref).all() and np.isfinite(allow).all()
    assert share <= MAX_AMBIGUOUS, share
    if case["model"] == "glm":
        got = sr.glm_score_f32(a["theta"], a["kind"], a["w_col"], a["F"], a["alpha_col"], a["X"], a["y"], a["scale"],
                               a["prior_precision"], a["gamma_rate"])
    else:
        got = sr.bnn_score_f32(a["theta"], a["n_in"], a["H"], a["cols"], a["X"], a["y"], a["n_train"], a["ga"], a["gb"])
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    live = sc.live_columns(case, a)
    assert (err[:, ~live] == 0).all()
    ratio = (err[:, live] / allow[:, live]).max()
    print("%s %s: fp32 emulation max |err| / allowance = %.3f, ambiguous share %.4f" % (case["model"], case["name"], ratio, share))
    assert (err <= allow).all(), ratio
    if case["flavor"] == "chunk":
        shares = sc.heavy_row_shares(case, a)
        assert min(shares) >= 0.9, shares
    if case["flavor"] in ("saturated", "bigtarget", "dead"):
        sc.check_extreme_inputs(case, a)


@pytest.mark.parametrize("case", [c for c in sc.BNN_CASES if not sc.cpu_sized(c)], ids=lambda c: c["name"])
def test_large_bnn_cases_keep_the_ambiguous_share(case):
    a = sc.bnn_args(case)
    _, _, share = sc.reference(case, a)
    assert share <= MAX_AMBIGUOUS, share


# ---- (c) ------------------------------------------------------------------------------------------
def _source():
    return open(os.path.join(ROOT, "stein_amd", "csrc", "stein_score.hip")).read()


def test_tables_name_every_instantiation_and_edge():
    src = _source()
    glm_pairs = {(int(a), int(b)) for a, b in re.findall(r"\bSC_LAUNCH\((\d+),\s*(\d+)\)", src)}
    bnn_pairs = {(int(a), int(b)) for a, b in re.findall(r"\bBNN_LAUNCH\((\d+),\s*(\d+)\)", src)}
    assert len(glm_pairs) == 7 and len(bnn_pairs) == 7 and "k_score_glm_few" in src
    assert "SC_MAXLDS = 15 * 1024" in src and "SC_FEW = 8" in src and "BNN_FMAX = 4" in src
    # the thresholds that sc.glm_kernel / sc.bnn_kernel restate: a dispatch moved in the source must be moved there too
    assert "if (n_feats <= SC_FEW) {" in src and "n_feats <= 256 ? 16 : 64" in src and "n_hidden <= 128 ? 16 : 64" in src
    ladder = lambda macro: [(int(k), int(a), int(b)) for k, a, b in re.findall(r"if \(k[fh] <= (\d+)\) %s\((\d+),\s*(\d+)\)" % macro, src)]  # noqa: E731
    last = lambda macro: [(int(a), int(b)) for a, b in re.findall(r"else %s\((\d+),\s*(\d+)\)" % macro, src)]  # noqa: E731
    assert ladder("SC_LAUNCH") == [(1, 1, 16), (2, 2, 16), (4, 4, 16), (8, 8, 16), (8, 8, 64)] and last("SC_LAUNCH") == [(16, 16), (16, 64)]
    assert ladder("BNN_LAUNCH") == [(1, 1, 16), (2, 2, 16), (4, 4, 16), (4, 4, 64), (8, 8, 64)] and last("BNN_LAUNCH") == [(8, 16), (16, 64)]
    inst_f = [c["F"] for c in sc.GLM_INST]
    inst_h = [c["H"] for c in sc.BNN_INST]
    assert {sc.glm_kernel(F) for F in inst_f} == glm_pairs | {"few"}
    assert {sc.bnn_kernel(H) for H in inst_h} == bnn_pairs
    for lo, hi in sc.GLM_EDGES:
        assert lo in inst_f and hi in inst_f and sc.glm_kernel(lo) != sc.glm_kernel(hi)
    for lo, hi in sc.BNN_EDGES:
        assert lo in inst_h and hi in inst_h and sc.bnn_kernel(lo) != sc.bnn_kernel(hi)
    assert {1, 1024} <= set(inst_f) and {1, 1024} <= set(inst_h)
    # the edges are all there are: between two neighbouring edges the dispatch does not change
    for kern, edges in ((sc.glm_kernel, sc.GLM_EDGES), (sc.bnn_kernel, sc.BNN_EDGES)):
        changes = [(v, v + 1) for v in range(1, 1024) if kern(v) != kern(v + 1)]
        assert changes == [e for e in edges if kern(e[0]) != kern(e[1])] and len(changes) == len(edges)
    assert sorted({c["n_in"] for c in sc.BNN_INST}) == [1, 2, 3, 4]
    assert {c["kind"] for c in sc.GLM_INST} == {"linear", "logistic"}
    assert {c["alpha"] for c in sc.GLM_INST} == {None, "before", "after", "last"}
    assert 1 in [c["n"] for c in sc.GLM_INST] and 1 in [c["n"] for c in sc.BNN_INST]
    for c in sc.GLM_INST:            # n not a multiple of the particles per workgroup pass
        k = sc.glm_kernel(c["F"])
        assert c["n"] % (4 if k == "few" else 4 * (64 // k[1])) != 0
    for c in sc.BNN_INST:
        assert c["n"] % (4 * (64 // sc.bnn_kernel(c["H"])[1])) != 0
    # log alpha at a column >= LP that is not a multiple of LP (its zero fill and its value come from different lanes)
    assert any(sc.glm_layout(c["F"], c["alpha"])[1] >= 16 and sc.glm_layout(c["F"], c["alpha"])[1] % 16 and sc.glm_kernel(c["F"])[1] == 16
               for c in sc.GLM_INST if c["alpha"])
    assert any(sc.glm_layout(c["F"], c["alpha"])[1] >= 64 and sc.glm_layout(c["F"], c["alpha"])[1] % 64 and sc.glm_kernel(c["F"])[1] == 64
               for c in sc.GLM_INST if c["alpha"])


def test_bnn_layouts_are_unsorted_with_gaps():
    for order in sc.BNN_BLOCK_ORDERS:
        cols, d = sc.bnn_layout(3, 10, order)
        assert list(cols) != sorted(cols)
        live = np.zeros(d, bool)
        for k, c in zip(sr.BNN_ORDER, cols):
            n = dict(w1=30, b1=10, w2=10).get(k, 1)
            assert not live[c:c + n].any()
            live[c:c + n] = True
        assert not live[0] and not live[-1] and (~live).sum() >= 8


def test_tables_reach_chunk_edges_and_grid_caps():
    assert sorted({c["F"] for c in sc.GLM_CHUNK}) == [9, 70, 1024]
    assert sorted({c["n_in"] for c in sc.BNN_CHUNK}) == [1, 4]
    for cases, key in ((sc.GLM_CHUNK, "F"), (sc.BNN_CHUNK, "n_in")):
        for width in {c[key] for c in cases}:
            rows = 15360 // (width + 1)
            assert rows == sc.chunk_rows(width)
            assert sorted(c["B"] for c in cases if c[key] == width) == [rows - 1, rows, rows + 1, 2 * rows, 3 * rows + 1]
            assert sc.heavy_rows(3 * rows + 1, width) == [0, rows - 1, rows, 2 * rows - 1, 2 * rows, 3 * rows - 1, 3 * rows]
    assert min(sc.chunk_rows(n_in) for n_in in (1, 2, 3, 4)) == 3072
    want = {"few": 16384 + 5, ("glm", 16): 32768 + 17, ("glm", 64): 8192 + 3, ("bnn", 16): 65536 + 9, ("bnn", 64): 16384 + 3}
    seen = {}
    for c in sc.GLM_GRID:
        k = sc.glm_kernel(c["F"])
        seen["few" if k == "few" else ("glm", k[1])] = c["n"]
    for c in sc.BNN_GRID:
        seen[("bnn", sc.bnn_kernel(c["H"])[1])] = c["n"]
    assert seen == want
    for k, n in seen.items():
        assert sc.GRID_CAPS[k] < n < 2 * sc.GRID_CAPS[k]
    src = _source()
    assert "blocks > 4096) blocks = 4096" in src and "blocks > 2048) blocks = 2048" in src


# ---- (d) ------------------------------------------------------------------------------------------
def _glm(lib, n=4, d=8, kind=_lib.GLM_LOGISTIC, w_col=0, F=3, alpha_col=-1, batch=5):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return lib.stein_score_glm(p, n, d, kind, w_col, F, alpha_col, p, p, batch, 1.0, 1.0, 0.01, p, None)


def _bnn(lib, n=4, d=40, n_in=2, H=3, cols=(0, 6, 9, 12, 13, 14), batch=5, n_train=10.0):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return lib.stein_score_bnn(p, n, d, n_in, H, (ctypes.c_int64 * 6)(*cols), p, p, batch, n_train, 1.0, 0.01, p, None)


def test_score_entry_points_refuse_bad_shapes_before_any_launch():
    """Every refusal below returns from the argument checks, which precede the launch: the host pointers handed over
    are never dereferenced and no kernel is queued (a launch without a GPU would answer E_HIP instead)."""
    lib = _lib.load()
    assert _glm(lib, d=1030, F=1025) == _lib.E_UNSUPPORTED and b"1024 features" in lib.stein_last_error()
    assert _glm(lib, w_col=6, F=3) == _lib.E_SHAPE                         # the weights run past d
    assert _glm(lib, w_col=2, F=3, alpha_col=3) == _lib.E_SHAPE            # log alpha inside the weights
    assert _glm(lib, w_col=2, F=3, alpha_col=2) == _lib.E_SHAPE and _glm(lib, w_col=2, F=3, alpha_col=4) == _lib.E_SHAPE
    assert _glm(lib, alpha_col=8) == _lib.E_SHAPE                          # log alpha past d
    assert _glm(lib, kind=2) == _lib.E_BADARG
    for bad in (dict(n=0), dict(d=0), dict(batch=0), dict(F=0)):
        assert _glm(lib, **bad) == _lib.E_SHAPE
    assert _bnn(lib, n_in=5, cols=(0, 15, 18, 21, 22, 23)) == _lib.E_UNSUPPORTED and b"input features" in lib.stein_last_error()
    assert _bnn(lib, d=5000, n_in=1, H=1025, cols=(0, 1025, 2050, 3075, 3076, 3077)) == _lib.E_UNSUPPORTED
    assert b"1024 hidden" in lib.stein_last_error()
    assert _bnn(lib, cols=(0, 5, 9, 12, 13, 14)) == _lib.E_SHAPE and b"overlap" in lib.stein_last_error()   # b1 inside w1
    assert _bnn(lib, cols=(0, 6, 9, 12, 13, 13)) == _lib.E_SHAPE and b"overlap" in lib.stein_last_error()   # two scalars share a column
    assert _bnn(lib, cols=(0, 6, 9, 12, 13, 7)) == _lib.E_SHAPE                                              # log_gamma inside b1
    assert _bnn(lib, d=14) == _lib.E_SHAPE and b"does not fit" in lib.stein_last_error()                     # log_gamma at column d
    assert _bnn(lib, d=40, cols=(35, 6, 9, 12, 13, 14)) == _lib.E_SHAPE and b"does not fit" in lib.stein_last_error()
    assert _bnn(lib, cols=(-1, 6, 9, 12, 13, 14)) == _lib.E_SHAPE
    for nt in (0.0, -3.0, float("nan")):
        assert _bnn(lib, n_train=nt) == _lib.E_BADARG and b"n_train" in lib.stein_last_error()
    for bad in (dict(n=0), dict(batch=0), dict(n_in=0), dict(H=0)):
        assert _bnn(lib, **bad) == _lib.E_SHAPE
