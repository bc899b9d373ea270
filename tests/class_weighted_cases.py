"""The case tables of tests/test_gpu_class_weighted.py: the predictive cases of tests/softmax_cases.py and
tests/netclass_cases.py (padded class counts, features / hidden units, staged pairs, rows, particle counts) crossed with the
eight weight patterns of tests/predict_weighted_cases.py, a Python mirror of what the WEIGHTED kernels skip, and the
references of one (model, case, pattern).  Shared with tests/test_class_weighted_cases.py, which proves on the CPU what the
tables reach and that a correct fp32 evaluation stays inside the allowance on these very inputs.

TEST INFRASTRUCTURE ONLY.

The patterns are predict_weighted_cases.PATTERNS and the weights of a (case, pattern) are predict_weighted_cases.weights':
positive, counts, one_hot_first | one_hot_last | one_hot_ragged, zero_slices (needs three slices: the 40-particle cases), wide
(2^-150 ... 1) and uniform.  The particle-count tables take every pattern that applies; the class, feature / hidden, staged
and row tables take one pattern each, in rotation.  The network's own tables have at most two staging units per slice
wherever a particle has more than one tile, so UNITS adds two small networks with five and nine units in their one slice --
three items (one and a half particles) and eight items (two and two thirds) per unit, so unit boundaries cut particles -- under
every pattern: the counts pattern leaves a dead unit between live ones there.

A staging unit of the softmax kernel is a pass of PP = max(16, CP) / CP particles; of the network kernel it is `ps` (particle,
tile) items of the slice's sequence.  Without pred a unit is dead -- neither staged nor computed -- when every particle that
has an item in it has lane weight zero.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_weighted_ref as cwr  # noqa: E402
import netclass_cases as ncc  # noqa: E402
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import softmax_cases as smc  # noqa: E402

PATTERNS = pwc.PATTERNS
BAD = pwc.BAD
bad_weights = pwc.bad_weights
PW_HEAD = pwc.PW_HEAD
PS_WB = PC_WB = 64     # csrc/stein_predict_softmax.hip, csrc/stein_predict_bnn_class.hip: lane weights staged at a time
MODELS = ("softmax", "netclass")


def _slice_bound(n):
    return min(-(-n // pc.PR_PASS), pc.PR_SLICE_CAP)


def workspace_bytes(model, n, B, C):
    """the weight pass's header of the slice bound (W, sum w^2, three doubles per slice) ahead of the unweighted states"""
    base = (smc if model == "softmax" else ncc).predict_workspace_bytes(n, B, C)
    return 8 * (PW_HEAD + 3 * _slice_bound(n)) + base


def weights(case, pattern):
    """-> w [n] float64: predict_weighted_cases.weights of the case's (name, n, B)"""
    return pwc.weights(dict(case, flavor=""), pattern)


def applies(case, pattern):
    return pwc.applies(case, pattern)


def _crossed(single, counts):
    out = []
    for i, case in enumerate(single):
        pat = PATTERNS[i % len(PATTERNS)]
        out.append((case, pat if applies(case, pat) else "positive"))
    for case in counts:
        out += [(case, pat) for pat in PATTERNS if applies(case, pat)]
    return out


UNITS = [ncc._pred("units_F128C3_n13", 128, 20, 3, 7, 13), ncc._pred("units_F100C7_n12", 100, 40, 7, 7, 12)]
CROSSED = {"softmax": _crossed(smc.PRED_CLASSES + smc.PRED_FEATS + smc.PRED_ROWS, smc.PRED_COUNTS),
           "netclass": _crossed(ncc.PRED_CLASSES + ncc.PRED_HIDDEN + ncc.PRED_STAGED + ncc.PRED_ROWS, ncc.PRED_COUNTS + UNITS)}
ALL = [(m, case, pat) for m in MODELS for case, pat in CROSSED[m]]


def triple_id(t):
    return "%s-%s-%s" % (t[0], t[1]["name"], t[2])


def args(model, case):
    return smc.predict_args(case) if model == "softmax" else ncc.predict_args(case)


def plan(model, case):
    """-> dict(cp, slices, per, unit, nt): unit = particles per pass (softmax) or items per staging unit (network), nt = tiles
    per particle (1 for softmax)"""
    if model == "softmax":
        p = smc.predict_plan(case["F"], case["C"], case["n"], case["B"])
        return {"cp": p["cp"], "slices": p["slices"], "per": p["per"], "unit": p["pp"], "nt": 1}
    p = ncc.predict_plan(case["F"], case["H"], case["C"], case["n"], case["B"])
    return {"cp": p["cp"], "slices": p["slices"], "per": p["per"], "unit": p["ps"], "nt": p["tiles"]}


def units(model, case, w):
    """-> per slice a list of (first particle, last particle, alive) of its staging units, particles counted in the whole set;
    alive: some particle with an item in the unit has a lane weight above zero"""
    pl = plan(model, case)
    vh = cwr.lane_weights(w)
    n, per, unit, nt = case["n"], pl["per"], pl["unit"], pl["nt"]
    out = []
    for s in range(pl["slices"]):
        begin, end = s * per, min(n, (s + 1) * per)
        items = (end - begin) * nt
        row = []
        for j0 in range(0, items, unit):
            cnt = min(unit, items - j0)
            k0, k1 = begin + j0 // nt, begin + (j0 + cnt - 1) // nt
            row.append((k0, k1, bool((vh[k0:k1 + 1] > 0).any())))
        out.append(row)
    return out


def dead_places(model, case, w):
    """-> the places at which a live slice has a dead unit: a subset of {"start", "inside", "end"}"""
    found = set()
    for row in units(model, case, w):
        alive = [u[2] for u in row]
        if not any(alive):
            continue
        first, last = alive.index(True), len(alive) - 1 - alive[::-1].index(True)
        if first > 0:
            found.add("start")
        if last < len(alive) - 1:
            found.add("end")
        if not all(alive[first:last + 1]):
            found.add("inside")
    return found


def reference(model, case, a, w, to=lambda v: v, z=None, tight=False):
    """class_weighted_ref.summaries of the case under the weights w; z: the call's own logits in the place of the fp64 ones"""
    th, X, w, labels = to(a["theta"]), to(a["X"]), to(w), to(a["labels"])
    if model == "softmax":
        zz, dz = cwr.softmax_logits(th, a["w_col"], a["F"], a["C"], X)
    else:
        zz, dz = cwr.netclass_logits(th, a["F"], a["H"], a["C"], a["cols"], X)
    if z is not None:
        zz = z
    return cwr.summaries(zz, dz, labels, w, plan(model, case)["per"], tight=tight)


def emulate_f32(model, case, a, w):
    per = plan(model, case)["per"]
    if model == "softmax":
        return cwr.softmax_f32(a["theta"], a["w_col"], a["F"], a["C"], a["X"], a["labels"], w, per)
    return cwr.netclass_f32(a["theta"], a["F"], a["H"], a["C"], a["cols"], a["X"], a["labels"], w, per)
