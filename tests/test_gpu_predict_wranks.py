"""GPU: the weighted order statistics of the predictive outputs (stein_predict_glm_ranks_weighted /
stein_predict_bnn_ranks_weighted and stein_predict_rank_masses of csrc/stein_predict_ranks.hip) through the C ABI, always on
a workspace filled with 0xFF bytes.

  planted       f_pb = x_b * w_p exactly (tests/quantile_cases.py) crossed with hand-written masses (tests/wquantile_cases.py),
                every target through its half-step level, eight per call: equal to the sorted cumulative masses entry by
                entry; all ones equal stein_predict_glm_ranks bit for bit; counts equal np.sort(np.repeat(f, c)); one-hots;
                one mass of 2^31 with M = 2^32 - 1; mass 0 on the NaN particles (no NaN comes back) and only on them (NaN);
                M = 0 and M >= 2^32 give NaN rows with STEIN_OK
  ones          every network instantiation: masses of 1 equal stein_predict_bnn_ranks bit for bit, one call each
  own pred      every case of the table, masses from stein_predict_rank_masses read back, eight weight patterns and counts in
                COUNTS mode: exactly the definition applied to the pred that stein_predict_* writes
  masses        NORMALISED inside 0.5 + A of w_p / W 2^31 and M inside n / 2 + A of 2^31, A = n 2^-21 (W's summation error);
                COUNTS exact; every bad-weights kind; weights over 2^-150 .. 1; a 2^k rescaling changes no bit; info
  fp64          the result lies in [Q(q - delta) - df, Q(q + delta) + df], Q the fp64 weighted quantile function of
                tests/predict_ref.py's outputs, delta = (n / 2 + 1) / 2^31 + A 2^-31, df the largest perturbation
  independence  a repeat, the workspace's contents, every slice count, every digit width 1 .. 4, the company and order of the
                levels: the same bits
Each fp64 case prints its largest (distance outside [Q(q - delta), Q(q + delta)]) / df (run with -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import quantile_cases as qc  # noqa: E402
import wquantile_cases as wq  # noqa: E402

pytestmark = pytest.mark.gpu


def _model_args(case, a):
    out = _lib.PRED_MEAN if case["output"] == "mean" else _lib.PRED_LINK
    if case["model"] == "bnn":
        return "bnn", lambda th, n: [th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]), out]
    kind = _lib.GLM_LINEAR if case["model"] == "linear" else _lib.GLM_LOGISTIC
    return "glm", lambda th, n: [th.data_ptr(), n, a["d"], kind, out, a["w_col"], case["F"]]


def _device(a, dev):
    return tuple(torch.tensor(a[k], dtype=torch.float32, device=dev) for k in ("theta", "X"))


def _mass_tensor(m, dev):
    """uint32 masses (any integer array below 2^32) as the int32 device tensor that carries their bits"""
    return torch.tensor(np.asarray(m, np.uint64).astype(np.uint32).view(np.int32), device=dev)


def _wranks(case, a, masses, levels, dev, ws_fill=0xFF, tensors=None, sync=True):
    """one weighted ranks call -> out [len(levels), B]; ws_fill: a byte, or "nan" for float NaNs"""
    th, X = tensors or _device(a, dev)
    n, B, R = th.shape[0], case["B"], len(levels)
    out = torch.full((R, B), -12345.5, dtype=torch.float32, device=dev)
    need = _lib.predict_ranks_weighted_workspace_bytes(n, B, R)
    if ws_fill == "nan":
        ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
    else:
        ws = torch.full((need,), ws_fill, dtype=torch.uint8, device=dev)
    which, head = _model_args(case, a)
    _lib.call("stein_predict_%s_ranks_weighted" % which, *head(th, n), X.data_ptr(), B, masses.data_ptr(),
              (ctypes.c_double * R)(*levels), R, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if sync:
        torch.cuda.synchronize()
    return out


def _ranks(case, a, ranks, dev, tensors=None):
    th, X = tensors or _device(a, dev)
    n, B, R = th.shape[0], case["B"], len(ranks)
    out = torch.full((R, B), -12345.5, dtype=torch.float32, device=dev)
    ws = torch.full((_lib.predict_ranks_workspace_bytes(n, B, R),), 0xFF, dtype=torch.uint8, device=dev)
    which, head = _model_args(case, a)
    _lib.call("stein_predict_%s_ranks" % which, *head(th, n), X.data_ptr(), B, (ctypes.c_int64 * R)(*ranks), R, out.data_ptr(),
              ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def _pred(case, a, dev, tensors=None):
    th, X = tensors or _device(a, dev)
    n, B = th.shape[0], case["B"]
    pred = torch.full((n, B), float("nan"), dtype=torch.float32, device=dev)
    which, head = _model_args(case, a)
    tau = [1.0] if which == "glm" else []
    _lib.call("stein_predict_%s" % which, *head(th, n), X.data_ptr(), None, B, *tau, pred.data_ptr(), None, None, None, None, 0,
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return pred


def _masses(w, mode, dev, ws_fill=0xFF):
    """stein_predict_rank_masses -> (the int32 device tensor of the masses' bits, masses as uint64 NumPy, info [2])"""
    n = len(w)
    wt = torch.tensor(np.asarray(w, np.float64), dtype=torch.float64, device=dev)
    m = torch.full((n,), -1, dtype=torch.int32, device=dev)
    info = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.full((_lib.predict_rank_masses_workspace_bytes(n),), ws_fill, dtype=torch.uint8, device=dev)
    _lib.call("stein_predict_rank_masses", wt.data_ptr(), n, mode, m.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(),
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return m, m.cpu().numpy().view(np.uint32).astype(np.uint64), info.cpu().numpy()


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bits_equal(got, want):
    """float32 arrays equal bit for bit, any NaN equal to any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | both_nan).all())


_SHARED = {}


def _case_data(case, dev):
    """inputs, device tensors and the library's own pred of a case: computed once, shared, never changed"""
    if case["name"] not in _SHARED:
        a = pc.args(case)
        tensors = _device(a, dev)
        _SHARED[case["name"]] = (a, tensors, _pred(case, a, dev, tensors).cpu().numpy())
    return _SHARED[case["name"]]


PLANT_CASE = pc._case("planted", "linear", qc.PLANT_N, qc.PLANT_B, F=1)


def _planted_args(w):
    return dict(theta=w[:, None].astype(np.float32), X=qc.PLANT_X[:, None], d=1, w_col=0)


# ---- (a) planted exact outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [name for name, _ in qc.planted()])
def test_planted_outputs_and_masses_exact(cuda, name):
    w = dict(qc.planted())[name]
    a = _planted_args(w)
    tensors = _device(a, cuda)
    with np.errstate(invalid="ignore"):
        f = qc.planted_products(w) + np.float32(0.0)      # as the kernel forms it, fmaf(x, w, +0): a -0 product comes out +0
    for mname, masses in wq.planted_masses(w):
        M = int(masses.astype(object).sum())
        targets = wq.planted_targets(masses)
        mt = _mass_tensor(masses, cuda)
        outs = [_wranks(PLANT_CASE, a, mt, [wq.half_step(t, M) for t in g], cuda, tensors=tensors, sync=False)
                for g in wq.groups(targets)]
        torch.cuda.synchronize()
        got = np.concatenate([o.cpu().numpy() for o in outs], axis=0)
        want = np.stack([wq.by_definition(f[:, b], masses, targets) for b in range(qc.PLANT_B)], axis=1)
        assert got.shape == want.shape
        for i, t in enumerate(targets):
            assert _bits_equal(got[i], want[i]), "%s target %d of %d: %s, the definition gives %s" % (mname, t, M, got[i], want[i])
        nans = np.isnan(got)
        if nans.any():                                                      # quiet NaNs come back
            assert ((got[nans].view(np.uint32) & 0x7FC00000) == 0x7FC00000).all()
        if mname == "ones":                                                 # the unweighted call, bit for bit
            plain = np.concatenate([_ranks(PLANT_CASE, a, g, cuda, tensors=tensors).cpu().numpy() for g in wq.groups(targets)], axis=0)
            assert targets == list(range(qc.PLANT_N)) and _bits_equal(got, plain)
            assert (got.view(np.uint32) == plain.view(np.uint32)).all()
        if mname in ("counts", "zero_on_nans"):
            rep = np.sort(np.repeat(f, masses.astype(np.int64), axis=0), axis=0)   # NaNs last
            assert targets == list(range(M)) and np.array_equal(got, rep, equal_nan=True)
        if mname == "zero_on_nans":
            assert not nans.any()
        if mname == "only_on_nans":
            assert nans.all()
        if mname.startswith("one_hot"):
            at = int(np.flatnonzero(masses)[0])
            assert all(_bits_equal(row, f[at]) for row in got)


@pytest.mark.parametrize("mname", [k for k, _ in wq.POISON])
def test_untrusted_masses_poison_the_call(cuda, mname):
    w = dict(qc.planted())["repeated"]
    a = _planted_args(w)
    got = _wranks(PLANT_CASE, a, _mass_tensor(dict(wq.POISON)[mname], cuda), [0.0, 0.5, 1.0], cuda).cpu().numpy()   # STEIN_OK
    assert np.isnan(got).all(), got


# the smallest network case of the table for each n_in it covers
ONES_CASES = [min((c for c in wq.CASES if c["model"] == "bnn" and c["n_in"] == k), key=lambda c: c["n"] * c["B"])
              for k in sorted({c["n_in"] for c in wq.CASES if c["model"] == "bnn"})]


@pytest.mark.parametrize("case", ONES_CASES, ids=lambda c: c["name"])
def test_network_masses_of_one_are_the_unweighted_call(cuda, case):
    """k_predict_bnn_ranks<NIN, true> with every mass 1 and the levels that select the ranks themselves against
    k_predict_bnn_ranks<NIN, false>: one call each, bit for bit (the planted test has this for the GLM only)"""
    a, tensors, _ = _case_data(case, cuda)
    n = case["n"]
    ranks = list(dict.fromkeys([0, 1, n // 2, n - 2, n - 1, n // 3, n // 3 + 1, 2 * n // 3]))   # deduplicated, in order
    assert len(ranks) <= wq.LEVELS_MAX and all(0 <= r < n for r in ranks)
    assert [wq.target(wq.half_step(t, n), n) for t in ranks] == ranks
    weighted = _wranks(case, a, _mass_tensor(np.ones(n, np.uint64), cuda), [wq.half_step(t, n) for t in ranks], cuda,
                       tensors=tensors)
    plain = _ranks(case, a, ranks, cuda, tensors=tensors)
    torch.cuda.synchronize()
    assert not torch.isnan(plain).any() and _same(weighted, plain)


# ---- (b) every case against the library's own pred ------------------------------------------------------------------------
def _want_of(pred, masses, levels):
    M = int(masses.astype(object).sum())
    targets = [wq.target(q, M) for q in levels]
    return np.stack([wq.by_definition(pred[:, b], masses, targets) for b in range(pred.shape[1])], axis=1)


@pytest.mark.parametrize("case", wq.CASES, ids=lambda c: c["name"])
def test_against_the_librarys_own_pred_exact(cuda, case):
    a, tensors, pred = _case_data(case, cuda)
    assert np.isfinite(pred).all()
    runs = [(p, _lib.MASS_NORMALISED) for p in wq.PATTERNS if pwc.applies(case, p)] + [("counts", _lib.MASS_COUNTS)]
    for pattern, mode in runs:
        w = pwc.weights(case, pattern, a)
        mt, masses, info = _masses(w, mode, cuda)
        assert info[0] == float(masses.astype(object).sum()) and info[1] == (masses > 0).sum(), (pattern, info)
        if mode == _lib.MASS_COUNTS:
            assert (masses == w.astype(np.uint64)).all()
        got = _wranks(case, a, mt, wq.LEVELS, cuda, tensors=tensors).cpu().numpy()
        want = _want_of(pred, masses, wq.LEVELS)
        assert _bits_equal(got, want), "%s (mode %d): %d entries differ from the definition on pred" % (
            pattern, mode, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert not np.isnan(got).any()


# ---- (c) the masses pass against fp64 -----------------------------------------------------------------------------------
MASS_NS = (1, 37, 255, 256, 257, 300, 16400, 70001)     # one workgroup, its edges, several, more than one stride of 256 x 256


def _mass_weights(n, pattern):
    case = pc._case("m%d" % n, "linear", n, 5, F=3)
    return pwc.weights(case, pattern) if pwc.applies(case, pattern) else None


@pytest.mark.parametrize("n", MASS_NS)
def test_normalised_masses_against_fp64(cuda, n):
    A = n * 2.0 ** -21
    for pattern in wq.PATTERNS:
        w = _mass_weights(n, pattern)
        if w is None:
            continue
        _, m, info = _masses(w, _lib.MASS_NORMALISED, cuda)
        W = float(np.sum(w.astype(np.longdouble)))
        exact = w.astype(np.longdouble) / W * 2.0 ** 31
        err = float(np.abs(m.astype(np.longdouble) - exact).max())
        M = int(m.astype(object).sum())
        print("n %-6d %-15s max |m - w/W 2^31| = %.6f (bound %.6f)   |M - 2^31| = %d (bound %.1f)" % (
            n, pattern, err, 0.5 + A, abs(M - 2 ** 31), n / 2 + A))
        assert err <= 0.5 + A, (pattern, err)
        assert abs(M - 2 ** 31) <= n / 2 + A and M < 2 ** 32, (pattern, M)
        assert info[0] == float(M) and info[1] == (m > 0).sum()
        assert ((m == 0) == (np.rint(np.asarray(exact, np.float64)) == 0)).sum() >= n - 2   # below 2^-32 W: mass 0
        if pattern == "wide" and n > 100:
            assert (m == 0).sum() > n // 2 and m[-1] > 0 and (w[m == 0] < 2.0 ** -32 * W * 1.0000001).all()
        # a power-of-two rescaling of the weights, a second call and the workspace's contents change no bit
        for k in (-200, 37, 300):
            _, m2, info2 = _masses(w * 2.0 ** k, _lib.MASS_NORMALISED, cuda)
            assert (m2 == m).all() and (info2 == info).all(), (pattern, k)
        _, m3, info3 = _masses(w, _lib.MASS_NORMALISED, cuda, ws_fill=0)
        assert (m3 == m).all() and (info3 == info).all()


@pytest.mark.parametrize("n", (1, 37, 300, 70001))
def test_counts_masses_are_exact(cuda, n):
    rng = np.random.default_rng(n)
    c = rng.integers(0, 6, size=n).astype(np.float64)
    c[0] = 3.0
    _, m, info = _masses(c, _lib.MASS_COUNTS, cuda)
    assert (m == c.astype(np.uint64)).all() and info[0] == c.sum() and info[1] == (c > 0).sum()
    big = np.zeros(n)
    big[n // 2] = 2.0 ** 32 - 1.0                                           # the largest total there is
    _, m, info = _masses(big, _lib.MASS_COUNTS, cuda)
    assert int(m[n // 2]) == 2 ** 32 - 1 and info[0] == 2.0 ** 32 - 1.0 and info[1] == 1.0


@pytest.mark.parametrize("n", (37, 70001))
def test_bad_weights_zero_every_mass(cuda, n):
    cases = [(wq.bad_weights(n, kind), _lib.MASS_NORMALISED, kind) for kind in wq.BAD]
    cases += [(wq.bad_counts(n, kind), _lib.MASS_COUNTS, kind) for kind in wq.BAD_COUNTS]
    for w, mode, kind in cases:
        mt, m, info = _masses(w, mode, cuda)                                 # STEIN_OK
        assert (m == 0).all() and np.isnan(info[0]) and info[1] == 0.0, (kind, mode, info)
    # and a ranks call on such masses returns NaN rows
    w = dict(qc.planted())["repeated"]
    mt, _, _ = _masses(wq.bad_weights(qc.PLANT_N, "negative"), _lib.MASS_NORMALISED, cuda)
    assert np.isnan(_wranks(PLANT_CASE, _planted_args(w), mt, [0.1, 0.9], cuda).cpu().numpy()).all()


# ---- (d) end to end against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in wq.CASES if pc.cpu_sized(c)], ids=lambda c: c["name"])
def test_against_fp64_inside_the_quantised_probability(cuda, case):
    a, tensors, _ = _case_data(case, cuda)
    n = case["n"]
    f64, df = pc.reference(case, a)["pred"]
    f64, df = np.asarray(f64), np.asarray(df)
    allow = df.max(0)
    A = n * 2.0 ** -21
    delta = (n / 2 + 1) / 2.0 ** 31 + A * 2.0 ** -31
    worst = 0.0
    for pattern in ("positive", "counts", "zero_slices", "wide", "uniform", "one_hot_ragged"):
        if not pwc.applies(case, pattern):
            continue
        w = pwc.weights(case, pattern, a)
        mt, _, _ = _masses(w, _lib.MASS_NORMALISED, cuda)
        got = _wranks(case, a, mt, wq.LEVELS, cuda, tensors=tensors).cpu().numpy().astype(np.float64)
        for i, q in enumerate(wq.LEVELS):
            lo = wq.fp64_weighted_quantile(f64, w, q - delta)
            hi = wq.fp64_weighted_quantile(f64, w, q + delta)
            out = np.maximum(np.maximum(lo - got[i], got[i] - hi), 0.0)
            worst = max(worst, float((out / allow).max()))
            assert (out <= allow).all(), (pattern, q, float((out / allow).max()))
    print("%-14s largest distance outside [Q(q - delta), Q(q + delta)] / df = %.3f" % (case["name"], worst))


# ---- (e) what changes no bit --------------------------------------------------------------------------------------------
def _some_masses(case, a, dev, pattern="positive"):
    return _masses(pwc.weights(case, pattern, a), _lib.MASS_NORMALISED, dev)[0]


def test_repeat_workspace_and_level_sets_change_no_bit(cuda):
    for case in (wq.CASES[1], wq.CASES[2], wq.CASES[4]):
        a, tensors, _ = _case_data(case, cuda)
        mt = _some_masses(case, a, cuda)
        levels = list(wq.LEVELS)
        first = _wranks(case, a, mt, levels, cuda, tensors=tensors)
        assert _same(first, _wranks(case, a, mt, levels, cuda, tensors=tensors)), "a second call differs"
        for fill in (0, 0x5A, "nan"):
            assert _same(first, _wranks(case, a, mt, levels, cuda, ws_fill=fill, tensors=tensors)), "the workspace's contents matter"
        perm = [3, 0, 6, 6, 2, 5, 0, 1]                                    # permuted, with repeats; levels 4 and 7 left out
        mixed = _wranks(case, a, mt, [levels[i] for i in perm], cuda, tensors=tensors)
        for row, i in enumerate(perm):
            assert _same(mixed[row], first[i]), "level %g changes with its company" % levels[i]
        for i, q in enumerate(levels):                                     # alone (for q_chunked that is also 4 against 3 bits a level)
            assert _same(_wranks(case, a, mt, [q], cuda, tensors=tensors)[0], first[i]), "level %g alone differs" % q


@pytest.mark.parametrize("case", [wq.CASES[7], wq.CASES[5], PLANT_CASE], ids=lambda c: c["name"])
def test_any_particle_slicing_gives_the_same_bits(cuda, case):
    if case is PLANT_CASE:
        a = _planted_args(dict(qc.planted())["repeated"])
        tensors = _device(a, cuda)
        mt = _mass_tensor(dict(wq.planted_masses(dict(qc.planted())["repeated"]))["big"], cuda)
    else:
        a, tensors, _ = _case_data(case, cuda)
        mt = _some_masses(case, a, cuda, "counts")
    first = _wranks(case, a, mt, wq.LEVELS, cuda, tensors=tensors)
    try:
        for slices in (1, 2, 7, 1024):
            _lib.debug_predict_ranks_slices(slices)
            assert _same(first, _wranks(case, a, mt, wq.LEVELS, cuda, tensors=tensors)), "%d slices differ" % slices
    finally:
        _lib.debug_predict_ranks_slices(0)


@pytest.mark.parametrize("case", [wq.CASES[0], wq.CASES[2], wq.CASES[3], wq.CASES[4], wq.CASES[5], wq.CASES[6], PLANT_CASE],
                         ids=lambda c: c["name"])
def test_every_digit_width_gives_the_same_bits(cuda, case):
    if case is PLANT_CASE:
        a = _planted_args(dict(qc.planted())["zeros_infs"])
        tensors = _device(a, cuda)
        mt = _mass_tensor(dict(wq.planted_masses(dict(qc.planted())["zeros_infs"]))["big"], cuda)
    else:
        a, tensors, _ = _case_data(case, cuda)
        mt = _some_masses(case, a, cuda)
    pairs = ([0.05, 0.95], [0.5, 1.0], [0.0, 1.0 / 3.0])                    # two levels: 4 bits fit beside every tile
    first = [_wranks(case, a, mt, p, cuda, tensors=tensors) for p in pairs]
    eight = _wranks(case, a, mt, wq.LEVELS, cuda, tensors=tensors)          # the rule's own width at eight levels (3 bits for q_chunked, else 4)
    for p, f in zip(pairs, first):
        for i, q in enumerate(p):
            assert _same(f[i], eight[wq.LEVELS.index(q)])
    try:
        for bits in (1, 2, 3, 4):
            _lib.debug_predict_ranks_weighted_bits(bits)
            for p, f in zip(pairs, first):
                assert _same(f, _wranks(case, a, mt, p, cuda, tensors=tensors)), "%d bits a level differ" % bits
    finally:
        _lib.debug_predict_ranks_weighted_bits(0)
