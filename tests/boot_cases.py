"""The case table of the KSD-test tests (a helper, not a test; tests/test_boot_cases.py proves on the CPU what the table
claims, tests/test_gpu_boot.py runs it on the GPU).

Inputs: a standard-normal target (score G = -X) and X ~ N(0, I) (+ `shift` in every coordinate) rounded to fp32, at the
median-heuristic bandwidth (fp64, rounded to fp32 and handed to the library: both sides use the same h2).  Weights: row 0
is all ones (the statistic itself), the others are sign processes (boot_ref.sign_rows) or, `multinomial`, Liu et al.'s
centred multinomial weights m_i / n - 1 / n -- general fp32 values of mixed magnitude.

The arms of stein_ksd_boot (stein_amd/csrc/stein_boot.hip), mirrored by `arm`:
    row_tiles   ceil(n / 128): the last tile's rows >= n are masked in the tail, its columns >= n by the select
    ntk         ceil(d / 32) k tiles of the Gram products
    cblocks     ceil(reps / 128) blocks of replicates; an odd count leaves the last group's second four waves without a block
    col_groups  ceil(reps / 256)
    jsplit      j ranges (forced through stein_debug_boot_jsplit; at most row_tiles)
The P cases are the p-value cases: for them the fp64 reference must be DECISIVE -- no replicate within 4 x (its allowance +
the statistic's) of Q_0 (boot_ref.undecided == 0; the cap is 0, a case that misses it gets another seed, never a cap).  Under
the null Q_0 lies inside the replicates' spread, whose spacing shrinks with their number while the worst-case allowance grows
with n: the null cases are small (48 x 3, 63 replicates); the shifted samples reject with every replicate far below Q_0.
"""
import functools

import numpy as np

import boot_ref as R


class Case:
    def __init__(self, n, d, reps, kernel, seed=0, shift=0.0, multinomial=False, flip_prob=0.5, pvalue=None):
        self.n, self.d, self.reps, self.kernel, self.seed, self.shift = n, d, reps, kernel, seed, shift
        self.multinomial, self.flip_prob, self.pvalue = multinomial, flip_prob, pvalue
        self.name = "%dx%d_r%d_%s%s%s" % (n, d, reps, kernel, "_mn" if multinomial else "",
                                          "_" + pvalue if pvalue else "")

    def inputs(self):
        """(X, G, h2, W): fp32 arrays [n, d], [n, d], the fp32-rounded bandwidth^2, fp32 weights [reps, n]"""
        rng = np.random.default_rng(7000 + self.seed)
        X = (rng.standard_normal((self.n, self.d)) + self.shift).astype(np.float32)
        G = -X
        if self.multinomial:
            W = (rng.multinomial(self.n, np.full(self.n, 1.0 / self.n), size=self.reps) / self.n - 1.0 / self.n).astype(np.float32)
        else:
            W = R.sign_rows(self.reps, self.n, 9000 + self.seed, self.flip_prob)
        W[0] = 1.0
        return X, G, R.median_h2(X), W

    def splits(self):
        """the forced j splits that give distinct plans: 1, 2, 3 capped at the row tiles"""
        return sorted({min(k, arm(self.n, self.d, self.reps)[0]) for k in (1, 2, 3)})


def arm(n, d, reps):
    """(row_tiles, ntk, cblocks, col_groups)"""
    return (n + 127) // 128, (d + 31) // 32, (reps + 127) // 128, (reps + 255) // 256


SHAPES = [(2, 1, 1), (3, 3, 2), (127, 31, 31), (128, 32, 32), (129, 33, 33), (257, 3, 128), (300, 260, 129), (257, 33, 257),
          (300, 1, 2), (129, 260, 31)]
CASES = [Case(n, d, reps, kernel, multinomial=(n == 127)) for n, d, reps in SHAPES for kernel in R.KERNELS]
P_CASES = [
    Case(48, 3, 64, "imq", seed=1, pvalue="null"),
    Case(48, 3, 64, "rbf", seed=1, pvalue="null"),
    Case(192, 3, 256, "imq", seed=1, shift=0.6, pvalue="shift"),
    Case(257, 5, 128, "rbf", seed=2, shift=0.6, flip_prob=0.1, pvalue="shift"),
]
CASES += P_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(X, G, h2, W, forms): the case's inputs and boot_ref.quadratic_forms of them; computed once per process and shared
    -- treat the arrays as read-only"""
    c = BY_NAME[name]
    X, G, h2, W = c.inputs()
    return X, G, h2, W, R.quadratic_forms(X, G, h2, c.kernel, W)
