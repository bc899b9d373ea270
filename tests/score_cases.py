"""The case tables of tests/test_gpu_score_matrix.py and the inputs of every case (NumPy, seeded), shared with
tests/test_score_ref.py, which checks on the CPU that the tables reach every instantiation of csrc/stein_score.hip and
that a correct fp32 evaluation stays inside the allowance on these very inputs.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

SC_MAXLDS = 15 * 1024      # SC_MAXLDS of stein_score.hip: floats of X per LDS chunk; a chunk holds SC_MAXLDS // (F + 1) rows
GLM_EDGES = ((8, 9), (16, 17), (32, 33), (64, 65), (128, 129), (256, 257), (512, 513))   # F: last / first of a dispatch arm
BNN_EDGES = ((16, 17), (32, 33), (64, 65), (128, 129), (256, 257), (512, 513))            # H
# particles a grid covers before its grid-stride loop goes round again: workgroup cap * particles per workgroup
GRID_CAPS = {"few": 4096 * 4, ("glm", 16): 2048 * 16, ("glm", 64): 2048 * 4, ("bnn", 16): 4096 * 16, ("bnn", 64): 4096 * 4}


def glm_kernel(F):
    """the instantiation stein_score_glm dispatches F features to: "few" or (KF, LP)"""
    if F <= 8:
        return "few"
    lp = 16 if F <= 256 else 64
    kf = -(-F // lp)
    return (next(k for k in ((1, 2, 4, 8, 16) if lp == 16 else (8, 16)) if kf <= k), lp)


def bnn_kernel(H):
    lp = 16 if H <= 128 else 64
    kh = -(-H // lp)
    return (next(k for k in ((1, 2, 4, 8) if lp == 16 else (4, 8, 16)) if kh <= k), lp)


def chunk_rows(width):
    return SC_MAXLDS // (width + 1)


def chunk_batches(width):
    c = chunk_rows(width)
    return (c - 1, c, c + 1, 2 * c, 3 * c + 1)


def heavy_rows(B, width):
    """row 0, both sides of every chunk edge, and the last row"""
    c = chunk_rows(width)
    rows = {0, B - 1}
    for e in range(c, B, c):
        rows |= {e - 1, e}
    return sorted(r for r in rows if 0 <= r < B)


# ---- GLM -----------------------------------------------------------------------------------------
# alpha placement -> (w_col, alpha_col, d): spare (zero-score) columns before, between and after the model's
def glm_layout(F, alpha):
    if alpha is None:
        return 1, -1, F + 3
    if alpha == "before":
        return 3, 1, F + 5
    if alpha == "after":
        return 2, F + 3, F + 5
    if alpha == "last":
        return 1, F + 2, F + 3
    raise ValueError(alpha)


def _glm(name, kind, F, alpha, n, B, flavor="plain"):
    return dict(name=name, model="glm", kind=kind, F=F, alpha=alpha, n=n, B=B, flavor=flavor)


GLM_INST = [_glm("F%d" % F, kind, F, alpha, n, B) for F, kind, alpha, n, B in [
    (1, "linear", None, 1, 1000), (8, "logistic", "before", 7, 130), (9, "logistic", "after", 19, 50),
    (16, "linear", None, 33, 40), (17, "logistic", "last", 5, 33), (32, "logistic", "after", 37, 21),
    (33, "linear", "before", 18, 30), (64, "logistic", None, 21, 25), (65, "logistic", "last", 1, 20),
    (128, "linear", None, 17, 16), (129, "logistic", "after", 23, 12), (256, "logistic", "last", 9, 10),
    (257, "logistic", "after", 7, 9), (512, "linear", None, 5, 8), (513, "logistic", "last", 6, 7),
    (1024, "logistic", "before", 3, 6)]]
GLM_CHUNK = [_glm("chunkF%d_B%d" % (F, B), kind, F, alpha, n, B, "chunk") for F, kind, alpha, n in [
    (9, "logistic", None, 19), (70, "linear", "after", 5), (1024, "logistic", "before", 3)] for B in chunk_batches(F)]
GLM_GRID = [_glm("grid_few", "logistic", 2, "after", 16384 + 5, 3), _glm("grid_lp16", "linear", 9, "before", 32768 + 17, 3),
            _glm("grid_lp64", "logistic", 257, None, 8192 + 3, 2)]
GLM_EXTREME = [_glm("sat_few", "logistic", 3, "after", 41, 70, "saturated"), _glm("sat_lp16", "logistic", 40, "before", 41, 30, "saturated"),
               _glm("sat_lp64", "logistic", 300, "last", 9, 12, "saturated"), _glm("big_few", "linear", 5, "before", 41, 70, "bigtarget"),
               _glm("big_lp16", "linear", 20, "after", 41, 30, "bigtarget")]
GLM_CASES = GLM_INST + GLM_CHUNK + GLM_GRID + GLM_EXTREME


# ---- BNN -----------------------------------------------------------------------------------------
BNN_BLOCK_ORDERS = (("log_gamma", "w2", "b2", "w1", "log_lambda", "b1"), ("b1", "log_lambda", "w1", "log_gamma", "b2", "w2"),
                    ("w2", "w1", "log_gamma", "b1", "b2", "log_lambda"))


def bnn_layout(n_in, H, order):
    """-> (cols in the ABI's order, d): the blocks in `order`, one or two spare columns in front of each and one at the end"""
    size = dict(w1=n_in * H, b1=H, w2=H, b2=1, log_lambda=1, log_gamma=1)
    at, col = {}, 0
    for i, name in enumerate(order):
        col += 1 + i % 2
        at[name] = col
        col += size[name]
    return tuple(at[k] for k in sr.BNN_ORDER), col + 1


def _bnn(name, n_in, H, n, B, flavor="plain", seed=0):
    return dict(name=name, model="bnn", n_in=n_in, H=H, n=n, B=B, flavor=flavor, seed=seed)


BNN_INST = [_bnn("H%d" % H, n_in, H, n, B) for H, n_in, n, B in [
    (1, 1, 1, 7), (16, 2, 17, 20), (17, 3, 5, 12), (32, 4, 33, 9), (33, 1, 18, 30), (64, 2, 7, 16), (65, 3, 19, 10),
    (128, 4, 21, 8), (129, 1, 5, 25), (256, 2, 9, 12), (257, 3, 6, 10), (512, 4, 5, 8), (513, 1, 3, 12), (1024, 4, 2, 6)]]
# (seeds: a case whose ambiguous-mask share exceeded 2 % on the reference -- one unit of a 5 x 18 matrix is 2.2 % -- was reseeded)
BNN_CHUNK_SEEDS = {(1, 23041): 1}
BNN_CHUNK = [_bnn("chunkIn%d_B%d" % (n_in, B), n_in, 5, 5, B, "chunk", BNN_CHUNK_SEEDS.get((n_in, B), 0))
             for n_in in (1, 4) for B in chunk_batches(n_in)]
BNN_GRID = [_bnn("grid_lp16", 1, 2, 65536 + 9, 4), _bnn("grid_lp64", 1, 129, 16384 + 3, 2)]
BNN_EXTREME = [_bnn("dead_lp16", 2, 20, 21, 30, "dead"), _bnn("dead_lp64", 1, 200, 9, 12, "dead"),
               _bnn("sat_lp16", 3, 40, 21, 30, "saturated"), _bnn("sat_lp64", 4, 300, 5, 12, "saturated")]
BNN_CASES = BNN_INST + BNN_CHUNK + BNN_GRID + BNN_EXTREME


def cpu_sized(case):
    """is the case small enough for the NumPy reference and the fp32 emulation to cost well under a second?"""
    width = case["F"] if case["model"] == "glm" else case["H"] * (case["n_in"] + 2)
    return case["n"] * case["B"] * width <= 5_000_000


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _seed(case):
    return [sum(map(ord, case["name"])), case["n"], case["B"], case.get("seed", 0)]


def _signed(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.5, 1.5, size=shape)


def glm_args(case):
    """-> dict(theta, X, y [fp64 holding fp32 values], kind, w_col, F, alpha_col, scale, prior_precision, gamma_rate, d)"""
    rng = np.random.default_rng(_seed(case) + [1])
    F, n, B = case["F"], case["n"], case["B"]
    w_col, a_col, d = glm_layout(F, case["alpha"])
    th = rng.normal(size=(n, d)) * 0.5
    X = rng.normal(size=(B, F))
    y = rng.normal(size=B) if case["kind"] == "linear" else (rng.uniform(size=B) < 0.5).astype(np.float64)
    args = dict(kind=case["kind"], w_col=w_col, F=F, alpha_col=a_col, n_train=16000, scale=16000.0 / B, prior_precision=0.7, gamma_rate=0.01, d=d)
    if case["flavor"] == "saturated":        # |z| up to about 200, fractional labels, log alpha over [-20, 20]
        z = np.abs(X @ th[:, w_col:w_col + F].T).max()
        th[:, w_col:w_col + F] *= 200.0 / z
        y = rng.uniform(size=B)
    if case["flavor"] == "bigtarget":
        y = 1e4 * _signed(rng, B)
    if case["flavor"] in ("saturated", "bigtarget") and a_col >= 0:
        th[:, a_col] = rng.uniform(-20.0, 20.0, size=n)
        th[0, a_col], th[1, a_col] = 20.0, -20.0
    args.update(theta=_r32(th), X=_r32(X), y=_r32(y))
    if case["flavor"] == "chunk":
        rows = heavy_rows(B, F)
        Xh, yh = _signed(rng, (len(rows), F)), _signed(rng, len(rows)) * 4.0
        t = 4.0
        while True:                           # scale the heavy rows until dropping any one of them is far outside the allowance
            X[rows], y[rows] = t * Xh, t * yh
            args.update(X=_r32(X), y=_r32(y))
            if heavy_rows_matter(case, args) or t >= 2.0 ** 40:
                break
            t *= 4.0
    return args


def bnn_args(case):
    """-> dict(theta, X, y, n_in, H, cols, n_train, ga, gb, d)"""
    rng = np.random.default_rng(_seed(case) + [2])
    n_in, H, n, B = case["n_in"], case["H"], case["n"], case["B"]
    cols, d = bnn_layout(n_in, H, BNN_BLOCK_ORDERS[(H + n_in) % 3])
    c = dict(zip(sr.BNN_ORDER, cols))
    th = rng.normal(size=(n, d)) * 0.7
    X, y = rng.uniform(size=(B, n_in)), rng.normal(size=B)
    args = dict(n_in=n_in, H=H, cols=cols, n_train=float(5 * B), ga=1.0, gb=0.01, d=d)
    w1 = slice(c["w1"], c["w1"] + n_in * H)
    if case["flavor"] == "saturated":         # |z| up to about 200
        th[:, w1] *= 200.0 / np.abs(np.einsum("bf,pfh->pbh", X, th[:, w1].reshape(n, n_in, H))).max()
    if case["flavor"] == "dead":              # every third hidden unit is dead for every row
        th[:, c["b1"]:c["b1"] + H:3] = -100.0
    if case["flavor"] in ("saturated", "dead"):
        for k in ("log_lambda", "log_gamma"):
            th[:, c[k]] = rng.uniform(-20.0, 20.0, size=n)
        th[0, c["log_lambda"]], th[1, c["log_lambda"]], th[0, c["log_gamma"]], th[1, c["log_gamma"]] = 20.0, -20.0, -20.0, 20.0
    args.update(theta=_r32(th), X=_r32(X), y=_r32(y))
    if case["flavor"] == "chunk":
        # every hidden unit active on the heavy rows (w1 > 0, x > 0) and no small w2, so that a heavy row reaches every entry
        th[:, w1] = rng.uniform(0.5, 1.5, size=(n, n_in * H))
        th[:, c["w2"]:c["w2"] + H] = _signed(rng, (n, H))
        rows = heavy_rows(B, n_in)
        Xh, yh = rng.uniform(0.5, 1.5, size=(len(rows), n_in)), _signed(rng, len(rows)) * 40.0
        t = 4.0
        while True:
            X[rows], y[rows] = t * Xh, t * yh
            args.update(theta=_r32(th), X=_r32(X), y=_r32(y))
            if heavy_rows_matter(case, args) or t >= 2.0 ** 40:
                break
            t *= 4.0
    return args


def reference(case, args, row_weight=None, to=lambda a: a):
    """(score, allowance, ambiguous share) of a case from its args; `to` moves an array to where the reference runs"""
    th, X, y = to(args["theta"]), to(args["X"]), to(args["y"])
    rw = None if row_weight is None else to(row_weight)
    if case["model"] == "glm":
        s, al = sr.glm_score(th, args["kind"], args["w_col"], args["F"], args["alpha_col"], X, y, args["scale"],
                             args["prior_precision"], args["gamma_rate"], row_weight=rw)
        return s, al, 0.0
    return sr.bnn_score(th, args["n_in"], args["H"], args["cols"], X, y, args["n_train"], args["ga"], args["gb"], row_weight=rw)


def live_columns(case, args):
    """boolean [d]: the columns that belong to the model (every other column must come back exactly 0)"""
    live = np.zeros(args["d"], bool)
    if case["model"] == "glm":
        live[args["w_col"]:args["w_col"] + args["F"]] = True
        if args["alpha_col"] >= 0:
            live[args["alpha_col"]] = True
    else:
        size = dict(w1=args["n_in"] * args["H"], b1=args["H"], w2=args["H"], b2=1, log_lambda=1, log_gamma=1)
        for k, c in zip(sr.BNN_ORDER, args["cols"]):
            live[c:c + size[k]] = True
    return live


def heavy_row_shares(case, args):
    """for every heavy row of a chunk case: the share of the live entries that dropping the row moves by at least four
    times their allowance -- from the reference alone"""
    width = case["F"] if case["model"] == "glm" else case["n_in"]
    live = live_columns(case, args)
    full, allow, _ = reference(case, args)
    shares = []
    for r in heavy_rows(case["B"], width):
        rw = np.ones(case["B"])
        rw[r] = 0.0
        dropped, _, _ = reference(case, args, row_weight=rw)
        moved = np.abs(dropped - full)[:, live] >= 4.0 * allow[:, live]
        shares.append(float(moved.mean()))
    return shares


def heavy_rows_matter(case, args):
    return min(heavy_row_shares(case, args)) >= 0.9


def check_extreme_inputs(case, args):
    """assert that an extreme case's inputs are what its flavor promises (from the inputs alone): a later edit of
    glm_args / bnn_args that dropped one of these would otherwise leave the case passing and testing nothing"""
    th, X, y = args["theta"], args["X"], args["y"]
    if case["model"] == "glm":
        if case["flavor"] == "saturated":
            z = np.abs(X @ th[:, args["w_col"]:args["w_col"] + args["F"]].T).max()
            assert 150.0 <= z <= 250.0, z
            assert ((y > 0) & (y < 1)).all() and np.unique(y).size == y.size            # fractional labels
        if case["flavor"] == "bigtarget":
            assert case["kind"] == "linear" and 5e3 <= np.abs(y).min() and np.abs(y).max() <= 1.5e4
        assert args["alpha_col"] >= 0
        logs = [args["alpha_col"]]
    else:
        n_in, H = args["n_in"], args["H"]
        c = dict(zip(sr.BNN_ORDER, args["cols"]))
        w1 = th[:, c["w1"]:c["w1"] + n_in * H].reshape(-1, n_in, H)
        z = th[:, None, c["b1"]:c["b1"] + H] + np.einsum("bf,pfh->pbh", X, w1)          # [n, B, H]
        if case["flavor"] == "saturated":
            assert 150.0 <= np.abs(z).max() <= 250.0, np.abs(z).max()
        if case["flavor"] == "dead":
            dead = np.arange(H) % 3 == 0
            assert (th[:, c["b1"]:c["b1"] + H][:, dead] == -100.0).all() and (th[:, c["b1"]:c["b1"] + H][:, ~dead] != -100.0).all()
            assert (z[:, :, dead] < -50.0).all()                  # dead for every particle and every row, and far from the mask's edge
            assert (z[:, :, ~dead] > 0).any(axis=1).mean() > 0.5  # while most of the other units are live on some row
        logs = [c["log_lambda"], c["log_gamma"]]
    for col in logs:                                              # the log precisions span [-20, 20], both ends included
        assert th[:, col].min() == -20.0 and th[:, col].max() == 20.0
        assert np.abs(th[2:, col]).max() < 20.0 and np.ptp(th[2:, col]) > 10.0
