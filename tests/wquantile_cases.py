"""The tables of tests/test_gpu_predict_wranks.py (the weighted order statistics of the predictive outputs,
stein_predict_*_ranks_weighted and stein_predict_rank_masses of csrc/stein_predict_ranks.hip): a NumPy model of the weighted
select -- digit by digit over the keys of tests/quantile_cases.py, any digit width 1 .. 4, every output adding its
particle's integer mass -- the definition it has to meet (the sorted cumulative masses, np.repeat for counts), the mass
patterns of the planted test and the levels of the case table.  tests/test_wquantile_cases.py checks all of it on the CPU.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import quantile_cases as qc  # noqa: E402

# the constants of the weighted select in stein_predict_ranks.hip (tests/test_wquantile_cases.py reads them back)
PQW_MPARTS = 64        # 64-bit partial sums of the masses ahead of the select's state in the workspace
PQW_CUS = 256          # a grid of no more workgroups than this has no second workgroup to place on a CU
PQW_LDS_CU = 160 * 1024
PM_BLOCKS = 256        # workgroups of the masses pass at most
LEVELS_MAX = qc.RANKS_MAX
MASS_SCALE = 2 ** 31
CASES = qc.CASES


def workspace_bytes(B, R):
    return 8 * PQW_MPARTS + qc.workspace_bytes(B, R)


def masses_workspace_bytes(n):
    return 24 * min(-(-n // 256), PM_BLOCKS)


def counters_bytes(R, bits):
    """the word counters of a weighted counting workgroup: per lane 2^bits words per level and a word of padding"""
    return 4 * pc.PR_ROWS * (R * (1 << bits) + 1)


def glm_other_bytes(F):
    """the LDS of the GLM call beside its counters: the X tile, the staged weights, the pass's masses"""
    fc = min(F, pc.PR_FC)
    return 4 * (pc.PR_ROWS * (fc | 1) + fc * pc.PR_PASS + pc.PR_PASS)


def bnn_other_bytes(n_in):
    """the static LDS of the network call: the staged particles and their four words each"""
    return 4 * (pc.PR_PASS * (n_in + 2) * pc.PR_HC + pc.PR_PASS * 4)


def default_bits(R, other, workgroups):
    """predict_wranks_bits restated: the width of the least passes / min(2, workgroups that fit a CU), the wider on a tie;
    a grid of at most PQW_CUS workgroups counts as one per CU"""
    best, best_cost = 1, None
    for bits in (4, 3, 2, 1):
        lds = other + counters_bytes(R, bits)
        if lds > PQW_LDS_CU:
            continue
        passes = -(-32 // bits)
        cost = passes if workgroups > PQW_CUS and 2 * lds <= PQW_LDS_CU else 2 * passes
        if best_cost is None or cost < best_cost:
            best, best_cost = bits, cost
    return best


def case_bits(case, R):
    rt, slices, _ = pc.plan(case["n"], case["B"])
    other = bnn_other_bytes(case["n_in"]) if case["model"] == "bnn" else glm_other_bytes(case["F"])
    return default_bits(R, other, rt * slices)


def glm_lds_bytes(F, R, bits):
    return glm_other_bytes(F) + counters_bytes(R, bits)


# ---- the definition and the model ---------------------------------------------------------------------------------------
def target(q, M):
    """max(0, ceil(q M) - 1) as the device computes it: one fp64 multiply, then ceil"""
    c = np.ceil(np.float64(q) * np.float64(M))
    return 0 if c < 1.0 else int(c) - 1


def half_step(t, M):
    """the level that selects target t among M"""
    return (t + 0.5) / M


def by_definition(values, masses, targets):
    """out[i] = the smallest value, among the particles of positive mass, at which the cumulative mass in key order exceeds
    targets[i]; NaN when there is none (M <= t) -> float32"""
    values, masses = np.asarray(values, np.float32), np.asarray(masses, np.uint64)
    live = masses > 0
    keys = np.sort(qc.f32_key(values[live]), kind="stable")
    order = np.argsort(qc.f32_key(values[live]), kind="stable")
    cum = np.cumsum(masses[live][order], dtype=np.uint64)          # n masses below 2^32 each: no overflow
    out = []
    for t in targets:
        at = int(np.searchsorted(cum, np.uint64(t), side="right"))
        out.append(np.uint32(qc.NAN_KEY) if at >= len(cum) else keys[at])
    return qc.key_f32(np.array(out, np.uint32))


def weighted_select(values, masses, targets, bits=4):
    """the same as the kernels find it: per level of `bits` bits (the last takes what is left) the masses of the keys that
    share the prefix are summed per digit, and the digit is taken at which the running sum passes the remaining target; no
    digit passes it: the top digit, as k_predict_ranks_narrow does -> float32"""
    keys = qc.f32_key(values).astype(np.uint64)
    masses = np.asarray(masses, np.uint64)
    keys, masses = keys[masses > 0], masses[masses > 0]
    out = []
    for t in targets:
        prefix, rem, hi = 0, int(t), 32
        while hi > 0:
            width = min(bits, hi)
            shift = hi - width
            hi = shift
            match = (keys >> np.uint64(shift + width)) == np.uint64(prefix >> (shift + width))
            digits = ((keys[match] >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
            hist = [0] * (1 << width)
            for dg, m in zip(digits, masses[match]):
                hist[dg] += int(m)
            dg = (1 << width) - 1
            for b, c in enumerate(hist):
                if rem < c:
                    dg = b
                    break
                rem -= c
            prefix |= dg << shift
        out.append(prefix)
    return qc.key_f32(np.array(out, np.uint32))


# ---- the mass patterns of the planted test -----------------------------------------------------------------------------
def planted_masses(w):
    """-> [(name, masses uint64 [PLANT_N])] for a planted weight vector w (the NaN particles are w's NaNs)"""
    n = qc.PLANT_N
    rng = np.random.default_rng(23)
    nan = np.isnan(w)
    counts = rng.integers(0, 5, size=n).astype(np.uint64)
    counts[rng.permutation(n)[:9]] = 0
    counts[0] = max(int(counts[0]), 1)
    out = [("ones", np.ones(n, np.uint64)), ("counts", counts)]
    for name, at in (("one_hot_first", 0), ("one_hot_middle", n // 2), ("one_hot_last", n - 1)):
        m = np.zeros(n, np.uint64)
        m[at] = 3
        out.append((name, m))
    big = np.ones(n, np.uint64)
    big[5] = 2 ** 31
    big[20] = 2 ** 32 - 1 - 2 ** 31 - (n - 2)                     # M = 2^32 - 1
    out.append(("big", big))
    if nan.any():
        out.append(("zero_on_nans", np.where(nan, 0, counts + np.uint64(1)).astype(np.uint64)))
        out.append(("only_on_nans", np.where(nan, 2, 0).astype(np.uint64)))
    return out


def planted_targets(masses):
    """every target below M when M is small, otherwise every target within 40 of a point where the answer can change"""
    M = int(np.asarray(masses, np.uint64).astype(object).sum())
    if M <= 200:
        return list(range(M))
    edges = {0, M}
    for m in masses:
        edges |= {int(m), M - int(m)}
    return sorted({t for e in edges for t in range(e - 40, e + 40) if 0 <= t < M})


def groups(items):
    items = list(items)
    return [items[at:at + LEVELS_MAX] for at in range(0, len(items), LEVELS_MAX)]


POISON = (("all_zero", np.zeros(qc.PLANT_N, np.uint64)),                                   # M = 0
          ("overflow", np.full(qc.PLANT_N, 2 ** 32 - 1, np.uint64)),                       # M far past 2^32
          ("overflow_by_one", np.array([2 ** 31, 2 ** 31] + [0] * (qc.PLANT_N - 2), np.uint64)))   # M = 2^32 exactly


# ---- the levels of the case table and the weights of the masses pass ------------------------------------------------------
LEVELS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 1.0 / 3.0)
PATTERNS = pwc.PATTERNS
BAD = pwc.BAD + ("overflow",)


def bad_weights(n, kind):
    if kind == "overflow":
        return np.full(n, 1e308)
    return pwc.bad_weights(n, kind)


BAD_COUNTS = ("fraction", "too_large", "sum_too_large", "negative", "nan", "all_zero")


def bad_counts(n, kind):
    w = np.ones(n)
    if kind == "all_zero":
        return np.zeros(n)
    if kind == "sum_too_large":
        w[:2] = 2.0 ** 31
        return w
    w[n // 2] = {"fraction": 1.5, "too_large": 2.0 ** 32, "negative": -1.0, "nan": float("nan")}[kind]
    return w


def fp64_weighted_quantile(f, w, q):
    """Q(q) of the discrete distribution with atoms f [n, B] (fp64) and weights w: per column the smallest atom whose
    cumulative probability reaches q; q <= 0 gives the smallest live atom, q >= 1 the largest -> [B]"""
    f, w = np.asarray(f, np.float64), np.asarray(w, np.float64)
    live = w > 0
    f, w = f[live], w[live]
    out = np.empty(f.shape[1])
    for b in range(f.shape[1]):
        order = np.argsort(f[:, b], kind="stable")
        cum = np.cumsum(w[order]) / w.sum()
        at = int(np.searchsorted(cum, q, side="left")) if q > 0.0 else 0
        out[b] = f[order[min(at, len(order) - 1)], b]
    return out
