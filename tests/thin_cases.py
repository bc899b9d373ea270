"""The case table of the Stein thinning tests (a helper, not a test; tests/test_thin_cases.py proves on the CPU what the table
claims, tests/test_gpu_thin.py runs it on the GPU).

Inputs: a standard-normal target (score G = -X) and X ~ 1.5 N(0, I) + 0.3 rounded to fp32 -- wider than the target and off
its centre, so that the greedy picks have something to correct -- at the median-heuristic bandwidth, under both kernels.
Every case must leave at least DECISIVE_SHARE of its steps decisive (thin_ref.py) under the fp64 loop: a case that
misses it gets another seed or n, never a lower share.  A dense 1-d cloud is no case: at 700 x 1 a fifth to two fifths of
the steps are decisive, the rest real near-ties.

The arms of k_thin_step (stein_amd/csrc/stein_thin.hip), mirrored by `arm`:
    vec      16-byte units (d % 4 == 0 and aligned bases) or 4-byte units
    lg       lanes per row: the power of two that covers a row's units, 1 .. 64
    chunks   d <= 512: the picked row is staged once; beyond that in chunks of 512 columns inside the row loop
A workgroup takes 16 * (64 / lg) rows at a time (`rows_per_workgroup`).
"""
import functools

import numpy as np

import thin_ref as R

DECISIVE_SHARE = 0.75
CHUNK = 512


class Case:
    def __init__(self, n, d, m, seed=0, h2=None, dup=()):
        self.n, self.d, self.m, self.seed, self.h2, self.dup = n, d, m, seed, h2, tuple(dup)
        self.name = "%dx%d_m%d%s" % (n + len(dup), d, m, "_dup" if dup else "")

    def inputs(self):
        """(X, G, h2): fp32 arrays [n, d] and the fp32-rounded bandwidth^2 (the median heuristic's unless the case fixes it).
        dup: these rows of the base sample are appended again, in this order, as exact copies"""
        rng = np.random.default_rng(1000 + self.seed)
        X = (1.5 * rng.standard_normal((self.n, self.d)) + 0.3).astype(np.float32)
        if self.dup:
            X = np.concatenate([X, X[list(self.dup)]], 0)
        G = -X
        return X, G, R.f32(self.h2) if self.h2 is not None else R.median_h2(X)


def arm(d, aligned=True):
    """(vec, lg, chunks) of the kernel for rows of d columns"""
    vec = d % 4 == 0 and aligned
    units = d // 4 if vec else d
    lg = 1
    while lg < 64 and lg < units:
        lg *= 2
    return vec, lg, (d + CHUNK - 1) // CHUNK


def rows_per_workgroup(d, aligned=True):
    return 16 * (64 // arm(d, aligned)[1])


def grids(n, d):
    """the workgroup counts every case is run at besides the default: 1, 2, 3 and an odd count above what the rows fill"""
    full = (n + rows_per_workgroup(d) - 1) // rows_per_workgroup(d)
    return (1, 2, 3, (full + 2) | 1)


CASES = [
    Case(40, 1, 24),
    Case(130, 2, 40),
    Case(300, 5, 64),
    Case(513, 33, 64),
    Case(257, 130, 64),
    Case(96, 515, 32, seed=2),    # d past one chunk, 4-byte units: the second chunk holds 3 columns
    Case(17, 2001, 16, seed=13),  # four chunks.  (The distances of wide rows concentrate and the allowance grows with d:
                                  # at 129 x 2001 fewer than 3/4 of the steps are decisive under it, at any seed tried.)
    Case(2500, 7, 40),            # several workgroups
    Case(20, 3, 40),              # m > n: most picks are repeats
    Case(1, 3, 5, h2=1.0),        # n = 1: every pick is 0 (no median of one particle: the bandwidth is given)
    # the 16-byte arms, one per group width, and two chunks of them
    Case(70, 4, 16), Case(90, 8, 16), Case(600, 16, 24), Case(150, 32, 24), Case(140, 64, 24), Case(100, 128, 16),
    Case(80, 256, 16), Case(64, 520, 16),
    # the 4-byte group widths the cases above leave out (16 and 32 lanes)
    Case(110, 13, 16), Case(120, 21, 16),
    # exact duplicates: rows 40 and 17 of the base sample again at the end -- equal objectives, the lower index must win
    # (the fp64 loop picks a duplicated row four times under either kernel: those steps are ties, not decisive)
    Case(48, 6, 24, dup=(40, 17)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name, kernel):
    """(X, G, h2, picks, forced): the case's inputs, the fp64 greedy picks and thin_ref.teacher_forced of them; computed
    once per process and shared -- treat the arrays as read-only"""
    X, G, h2 = BY_NAME[name].inputs()
    picks, _ = R.greedy(X, G, h2, kernel, BY_NAME[name].m)
    return X, G, h2, picks, R.teacher_forced(X, G, h2, kernel, picks)
