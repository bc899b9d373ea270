"""The case table of tests/test_gpu_predict_ranks.py (the order statistics of the predictive outputs, stein_predict_*_ranks
of csrc/stein_predict_ranks.hip), the planted multisets of its exact test, and a NumPy model of the select itself: digit by digit
over the order-preserving 32-bit keys, every NaN on the top key.  tests/test_quantile_cases.py checks all three on the CPU.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402

# the constants of the select in stein_predict_ranks.hip (tests/test_quantile_cases.py reads them back from the source)
PQ_BITS = 4            # digit bits per level; a GLM call takes one less when that keeps two workgroups on a CU (glm_bits)
PQ_FLUSH = 15          # passes of PR_PASS particles between two flushes of a lane's byte counters
PQ_WORDS = 19          # workspace words per (row, rank)
RANKS_MAX = 8
NAN_KEY = 0xFFFFFFFF


def workspace_bytes(B, R):
    return 4 * PQ_WORDS * B * R


def glm_bits(F, R):
    """the digit width stein_predict_glm_ranks takes: the X tile, the staged weights and the counters -- per lane 2^bits
    bytes per rank and a word of padding -- of two workgroups fit the CU's 160 KiB with 4 bits, or else with 3"""
    fc = min(F, pc.PR_FC)
    tile = 4 * (pc.PR_ROWS * (fc | 1) + fc * pc.PR_PASS)
    counters = lambda bits: 4 * pc.PR_ROWS * (R * (1 << bits) // 4 + 1)   # noqa: E731
    return 3 if tile + counters(4) > 80 * 1024 and tile + counters(3) <= 80 * 1024 else 4


# ---- the model ------------------------------------------------------------------------------------------------------
def f32_key(x):
    """f32_key of stein_common.h on a float32 array, with the NaN rule of the ranks calls -> uint32"""
    x = np.asarray(x, np.float32)
    u = x.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(NAN_KEY), key).astype(np.uint32)


def key_f32(k):
    k = np.asarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    out = u.view(np.float32).copy()
    out[k == np.uint32(NAN_KEY)] = np.nan
    return out


def radix_select(values, ranks, bits=PQ_BITS):
    """the ranks[i]-th smallest of `values` (float32 [n]) for every i, as the kernels find it: per level count the digits
    of the keys that share the prefix, take the digit at which the running count passes the remaining rank -> float32"""
    keys = f32_key(values).astype(np.uint64)
    out = []
    for r in ranks:
        prefix, rem, hi = 0, int(r), 32
        while hi > 0:                       # the key's bits from the top, `bits` at a time; the last level takes what is left
            width = min(bits, hi)
            shift = hi - width
            hi = shift
            match = (keys >> (shift + width)) == (prefix >> (shift + width))
            hist = np.bincount(((keys[match] >> shift) & ((1 << width) - 1)).astype(np.int64), minlength=1 << width)
            for dg, c in enumerate(hist):
                if rem < c:
                    break
                rem -= int(c)
            else:
                raise AssertionError("rank %d is not among %d values" % (r, len(values)))
            prefix |= dg << shift
        out.append(prefix)
    return key_f32(np.array(out, np.uint32))


# ---- the cases against the library's own pred and against fp64 ---------------------------------------------------------
CASES = [
    pc._case("q_linear", "linear", 37, 5, F=3),                                         # three slices, a ragged last pass
    pc._case("q_logit_mean", "logistic", 45, 300, F=7, output="mean", alpha="before"),  # two row tiles with a row tail
    pc._case("q_chunked", "logistic", 50, 9, F=pc.PR_FC + 1),                           # the GLM kernel's chunked arm
    pc._case("q_bnn_H64", "bnn", 33, 20, n_in=4, H=pc.PR_HC),                           # one hidden chunk, full
    pc._case("q_bnn_H65", "bnn", 40, 17, n_in=1, H=pc.PR_HC + 1),                       # one unit into the second chunk
    pc._case("q_bnn_rows", "bnn", 100, 300, n_in=2, H=10),
    pc._case("q_bnn_in3", "bnn", 21, 6, n_in=3, H=7),
    pc._case("q_flush", "logistic", 300, 40, F=5, alpha="after"),   # 19 passes in one slice under the slices hook: a flush
    pc._case("q_cap", "linear", 16 * pc.PR_SLICE_CAP + 16, 3, F=2),                     # the slice cap binds
]


def ranks_of(n):
    k = n // 3
    return [0, 1, k, k + 1, n // 2, n - 2, n - 1]


# ---- planted outputs: f_pb = x_b * w_p exactly ---------------------------------------------------------------------
PLANT_N, PLANT_B = 37, 5
PLANT_X = np.array([1.0, 2.0, 0.5, 1024.0, 2.0 ** -10], np.float32)     # powers of two: the products are exact


def _chain(start, count):
    out = [np.float32(start)]
    for _ in range(count - 1):
        out.append(np.nextafter(out[-1], np.float32(np.inf), dtype=np.float32))
    return np.array(out, np.float32)


def planted():
    """-> [(name, w float32 [PLANT_N])], each shuffled by a seeded permutation"""
    rng = np.random.default_rng(11)
    n = PLANT_N
    below = np.float32(2.0)
    for _ in range(15):
        below = np.nextafter(below, np.float32(0.0), dtype=np.float32)
    chain = _chain(below, 30)                                            # 15 floats below 2.0, 2.0, 14 above
    fill = lambda k: (rng.uniform(0.5, 3.0, size=k) * rng.choice([-1.0, 1.0], size=k)).astype(np.float32)  # noqa: E731
    nan_neg = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    sets = [
        ("chain", np.concatenate([chain, fill(n - 30)])),
        ("chain_negative", np.concatenate([-chain, fill(n - 30)])),
        ("repeated", np.concatenate([np.full(5, 1.25, np.float32), fill(n - 5)])),
        ("all_equal", np.full(n, 1.5, np.float32)),
        ("zeros_infs", np.concatenate([np.array([0.0, -0.0, 0.0, -0.0, np.inf, -np.inf, np.inf, -np.inf], np.float32),
                                       fill(n - 8)])),
        ("one_nan", np.concatenate([np.array([np.nan], np.float32), fill(n - 1)])),
        ("several_nans", np.concatenate([np.array([np.nan, nan_neg, np.nan, nan_neg, np.nan], np.float32), fill(n - 5)])),
    ]
    return [(name, w[rng.permutation(n)].astype(np.float32)) for name, w in sets]


def planted_products(w):
    """-> float32 [PLANT_N, PLANT_B], f_pb = x_b * w_p (exact: tests/test_quantile_cases.py proves it)"""
    with np.errstate(invalid="ignore"):
        return (w[:, None].astype(np.float32) * PLANT_X[None, :]).astype(np.float32)


def rank_groups(n):
    """every rank 0 .. n-1, RANKS_MAX at a time"""
    return [list(range(at, min(at + RANKS_MAX, n))) for at in range(0, n, RANKS_MAX)]
