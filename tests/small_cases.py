"""Case tables of the one-kernel path (csrc/stein_small.hip, n <= 160) and a model of its run-time dispatch (a helper of
test_small_cases.py and test_gpu_small_matrix.py, not a test).

k_svgd_small picks its code shape from n and d.  `classify` restates those choices so that the tables below can be shown
-- by assertion, in test_small_cases.py -- to reach every one of them; it DESCRIBES cases and is never a yardstick for a
result (the GPU tests compare with the fp64 oracle).  Where it says a shape is on the path, test_small_cases.py asks the
library's own layout, and every GPU test asserts `eng._one_kernel` first.

    distances<RR>       R = ceil(n / 32)                                  1 ... 5
    phi_rows<RW, .>     n <= 32, <= 64, <= 128, else                      2, 4, 8, 10
    phi_rows<., CLW>    columns of THAT workgroup: <= 8, <= 16, else      8, 16, 32   (the last workgroup usually differs)
    theta chunk ck      small_chunk(n, d)                                 32 ... 256: ceil(d / ck) passes, the last one ragged
    grid                ceil(d / 32) workgroups                           1 writes |phi|^2 itself, more go through the sum kernel

n fixes (R, RW): (1, 2) for n <= 32, (2, 4) to 64, (3, 8) to 96, (4, 8) to 128, (5, 10) to 160.
"""
import numpy as np

SM_MAXN, SM_COLS, SM_CK, SM_STG, SM_THREADS = 160, 32, 32, 5, 1024     # copies of the constants of stein_small.hip
MAX_WORK = 2200000          # n * n * d bound of stein_small_ok
MAX_BLOCKS = 1024           # ceil(d / 32) bound of stein_small_ok


def small_chunk(n, d):
    """theta columns staged per pass of the distance loop (small_chunk, stein_small.hip)"""
    ck = SM_STG * SM_THREADS // n // SM_CK * SM_CK
    ck = min(max(ck, SM_CK), 256)
    return min(ck, (d + SM_CK - 1) // SM_CK * SM_CK)


def full_chunk(n):
    """the chunk of a matrix at least that wide: what n alone allows"""
    return small_chunk(n, 1 << 20)


def _clw(ncols):
    return 8 if ncols <= 8 else (16 if ncols <= 16 else 32)


def classify(n, d):
    """the code shape k_svgd_small takes at (n, d), and whether the fused call takes that kernel at all"""
    blocks = (d + SM_COLS - 1) // SM_COLS
    ck = small_chunk(n, d)
    return dict(R=(n + 31) // 32, RW=2 if n <= 32 else (4 if n <= 64 else (8 if n <= 128 else 10)),
                clw_first=_clw(min(SM_COLS, d)), clw_last=_clw(d - SM_COLS * (blocks - 1)), ck=ck, chunks=(d + ck - 1) // ck,
                blocks=blocks, on_path=2 <= n <= SM_MAXN and n * n * d <= MAX_WORK and blocks <= MAX_BLOCKS)


def chunk_role(n, d):
    """why (n, d) is a case of the chunk loop: d one short of, at, or one past a multiple of the chunk n allows; and / or n
    on either side of a step of that chunk"""
    ck = full_chunk(n)
    roles = []
    if d >= ck - 1 and (d + 1) % ck == 0:
        roles.append("k*ck-1")
    if d % ck == 0:
        roles.append("k*ck")
    if d > ck and (d - 1) % ck == 0:
        roles.append("k*ck+1")
    if full_chunk(n + 1) != ck or (n > 2 and full_chunk(n - 1) != ck):
        roles.append("ck step")
    return roles


# ---- the tables ----------------------------------------------------------------------------------------------------------
# both sides of every R / RW step, the ck step at 80, and the ends of the path
EDGE_N = (2, 3, 16, 17, 31, 32, 33, 63, 64, 65, 80, 95, 96, 97, 127, 128, 129, 159, 160)
# one workgroup with 1, 8, 9, 16, 17, 32 columns (each CLW, both of its ends); then a last workgroup with 1, 8, 9, 16, 17, 32
# and (three workgroups) 1 columns behind full ones
EDGE_D = (1, 8, 9, 16, 17, 32, 33, 40, 41, 48, 49, 64, 65)
EDGE_CASES = [(n, d) for n in EDGE_N for d in EDGE_D if n * n * d <= MAX_WORK]

# d = k ck - 1, k ck, k ck + 1 for the chunk of that n, on both sides of the ck steps 256 | 224 (n = 20 | 21), 128 | 96
# (40 | 41) and 64 | 32 (80 | 81); one, two, three and five / six passes
CHUNK_CASES = [(20, 256), (20, 257), (20, 511), (20, 512), (20, 513), (21, 224), (21, 225), (40, 128), (40, 129), (41, 96),
               (41, 97), (53, 96), (53, 97), (53, 193), (80, 64), (80, 65), (81, 32), (81, 33), (81, 160), (100, 97),
               (100, 161), (160, 65)]

# d far beyond anything else that stays on the path: up to 1024 workgroups, whose |phi|^2 (and KSD) partials the layout
# sizes by columns, not by its own finish pass; (13, 13000) sits under the n^2 d bound
WIDE_CASES = [(2, 32768), (3, 20000), (5, 4097), (8, 30000), (13, 13000)]

# (on the path, its neighbour off it): the workgroup bound, the n^2 d bound twice (once met exactly), the particle bound
EDGE_OF_PATH = [((2, 32768), (2, 32769)), ((160, 85), (160, 86)), ((100, 220), (100, 221)), ((160, 40), (161, 40))]

RANDOM_SEED = 20261019


def _random_cases():
    rng = np.random.default_rng(RANDOM_SEED)
    out = []
    while len(out) < 24:
        n = int(rng.integers(2, SM_MAXN + 1))
        d = int(np.exp(rng.uniform(0.0, np.log(min(600.0, MAX_WORK / (n * n))))))
        if (n, d) not in out:
            out.append((n, d))
    return out


RANDOM_CASES = _random_cases()

MATRIX_CASES = EDGE_CASES + [c for c in CHUNK_CASES if c not in EDGE_CASES]
MATRIX_CASES += [c for c in RANDOM_CASES if c not in MATRIX_CASES]

# the KSD instantiation: per (R, RW) class its smallest and its largest n; one workgroup with each CLW, then a last
# workgroup with each CLW behind full ones (two and three workgroups); and the widest launch (3 x 1024 partials)
_KSD_N = ((3, 32), (33, 64), (65, 96), (97, 128), (129, 160))
KSD_CASES = [(n, d) for lo, hi in _KSD_N for n, d in ((lo, 1), (hi, 9), (lo, 17), (hi, 40), (lo, 41), (hi, 64), (lo, 65))]
KSD_CASES.append((2, 32768))

# bit-level invariants: one shape per R, three workgroups with a ragged last one
BIT_CASES = [(20, 70), (50, 70), (80, 70), (120, 70), (150, 70)]

# the exact select on integer lattices (tests/select_inputs.py) where the distance stage is distances<3>, and on both sides
# of its edges; odd (65, 33, 97) and even (80, 96) counts n * n
SELECT_N = (65, 80, 96, 33, 97)
