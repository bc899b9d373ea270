"""The case table of the Stein importance weights' tests (a helper, not a test; tests/test_weights_cases.py proves on the CPU
what the table claims, tests/test_gpu_weights.py runs it on the GPU).

Inputs: a standard-normal target (score G = -X) and X = 1.3 z + 0.5, z ~ N(0, I), rounded to fp32 -- wider than the target
and off its centre, so that the weights have something to correct -- at the median-heuristic bandwidth.  `kind="near"`: every
coordinate |z| + 0.5 at the fixed bandwidth h2 = 50: the Stein-kernel matrix is close to the rank-one g g^T, all the mass goes
to the particle of the least |g| in ONE step (gamma = 1) and the iteration has converged: every later step has gamma = 0.
Every case must leave at least DECISIVE_SHARE of its steps decisive (weights_ref.py) under the fp64 iteration: a case that
misses it gets another seed, n or step count, never a lower share.

The arms of k_weights_step (stein_amd/csrc/stein_weights.hip) are k_thin_step's, mirrored by thin_cases.arm:
    vec      16-byte units (d % 4 == 0 and aligned bases) or 4-byte units
    lg       lanes per row: the power of two that covers a row's units, 1 .. 64
    chunks   d <= 512: the vertex's row is staged once; beyond that in chunks of 512 columns inside the row loop
and a virtual workgroup takes 16 * (64 / lg) rows at a time; there are min(1024, ceil(n / that)) of them (`parts`).
"""
import functools

import numpy as np

import weights_ref as R
from thin_cases import arm, rows_per_workgroup

DECISIVE_SHARE = 0.9
DUP_ROW = 51    # (the row the fp64 path of 90 x 8 picks first; tests/test_weights_cases.py checks that it is picked)


class Case:
    def __init__(self, n, d, kernel, iters, seed=0, kind="wide", dup=()):
        self.n, self.d, self.kernel, self.iters, self.seed, self.kind, self.dup = n, d, kernel, iters, seed, kind, tuple(dup)
        self.name = "%dx%d_%s_t%d%s%s" % (n + len(dup), d, kernel, iters, "_near" if kind == "near" else "", "_dup" if dup else "")

    def inputs(self):
        """(X, G, h2): fp32 arrays [n, d] and the fp32-rounded bandwidth^2.  dup: these rows of the base sample are
        appended again, in this order, as exact copies"""
        rng = np.random.default_rng(3000 + self.seed)
        z = rng.standard_normal((self.n, self.d))
        X = (np.abs(z) + 0.5 if self.kind == "near" else 1.3 * z + 0.5).astype(np.float32)
        if self.dup:
            X = np.concatenate([X, X[list(self.dup)]], 0)
        return X, -X, R.f32(50.0) if self.kind == "near" else R.median_h2(X)


def parts(n, d, aligned=True):
    return min(1024, (n + rows_per_workgroup(d, aligned) - 1) // rows_per_workgroup(d, aligned))


def grids(n, d):
    """the workgroup counts every case is run at besides the default: 1, 2, 3 and an odd count above the virtual workgroups"""
    return (1, 2, 3, (parts(n, d) + 2) | 1)


# The four shapes the feature was specified on.  Under the crude stand-in of the specification (2e-6 of the row mean of |U|)
# 63 or 64 of their first 64 steps are decisive; under the derived A_0 of weights_ref.py -- a worst-case bound, two to three
# orders of magnitude above the stand-in -- the paths stay 90 % decisive for 16, 8, 64 and 12 steps at these seeds (the early
# steps are the decisive ones: as the iteration converges the entries of g approach each other)
PATH_CASES = [Case(200, 3, "imq", 16, seed=3), Case(300, 5, "rbf", 8), Case(257, 17, "imq", 64, seed=5),
              Case(130, 33, "rbf", 12, seed=4)]
CASES = PATH_CASES + [
    # the 16-byte arms, one per group width (1 .. 64 lanes), and two chunks of them
    Case(70, 4, "rbf", 16, seed=4), Case(90, 8, "imq", 16), Case(100, 16, "rbf", 16), Case(150, 32, "imq", 16),
    Case(140, 64, "rbf", 12, seed=2), Case(100, 128, "imq", 16, seed=5), Case(40, 256, "rbf", 6, seed=4),
    Case(24, 520, "imq", 8, seed=4),
    # the 4-byte group widths the path cases leave out (1, 2 and 16 lanes), and d past one chunk: the second holds 3 columns.
    # (Wide rows: the distances concentrate and the allowance grows with d, so these are small and short.)
    Case(20, 1, "imq", 10, seed=3), Case(60, 2, "rbf", 12), Case(110, 13, "imq", 16), Case(40, 515, "rbf", 6, seed=1),
    Case(2, 3, "imq", 1, seed=7),       # the least n (its one step is interior; the optimum of two particles is a tie for good)
    Case(1300, 7, "imq", 10, seed=4),   # eleven virtual workgroups
    Case(40, 3, "imq", 8, kind="near"), Case(40, 3, "rbf", 8, kind="near"),   # gamma = 1, then gamma = 0 for good
    # an exact duplicate: row DUP_ROW of the base sample again at the end -- equal g, the lower index must win
    Case(90, 8, "imq", 16, dup=(DUP_ROW,)),
    Case(200, 3, "rbf", 0),             # iters = 0
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


class Ref:
    """X, G, h2;  model: weights_ref.Model;  w, idx, gamma, f: weights_ref.frank_wolfe;  forced: weights_ref.teacher_forced
    of that path"""


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per process and shared -- treat the arrays as read-only"""
    c = BY_NAME[name]
    r = Ref()
    r.X, r.G, r.h2 = c.inputs()
    r.model = R.Model(r.X, r.G, r.h2, c.kernel)
    r.w, r.idx, r.gamma, r.f = R.frank_wolfe(r.model, c.iters)
    r.forced = R.teacher_forced(r.model, r.idx, r.gamma)
    return r
