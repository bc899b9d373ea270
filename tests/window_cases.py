"""The speculative median window, placed by hand: a NumPy model of one windowed step and the table of placements the GPU
tests run (a helper of test_window_cases.py and test_gpu_window_placed.py, not a test).

The model is written from the contract stein_common.h states for SpecState, the window table and median_init_body, not
from the kernels:

    grant     a window [lo_key, lo_key + width] = [center - halfwidth, center + halfwidth] is granted when the state carries
              a magic word, halfwidth <= SPEC_HW_MAX and 0x80000000 + halfwidth <= center < 0xff000000 - halfwidth;
              otherwise lo_key = 0xffffffff, width = 0.  (halfwidth = 0 passes the rule and still opens nothing: width 0.)
    producer  every entry with a weight (upper-triangle rule: 2 above the diagonal, 1 on it; a rectangular block: 1) whose
              key lies below lo_key adds its weight to `below`; one whose key lies in [lo_key, lo_key + width] is queued by
              the workgroup that computed it.  A queue holds `capacity` entries; one entry more sets `overflow`.
    table     [0] below, [1] invalid (no window, overflow, more entries than SPEC_CAP), [2] entries, [8 + k] the weight of
              key lo_key + k -- no key counter is written when [1] is set.
    select    the targets are ranks r0 | r1 of `total`; they are found when below <= r0 and r1 - below < the weight inside.

Outcomes: hit, no_window, lo_below, lo_above, hi_above, overflow, over_capacity, empty.  For a hit the model also says
which form of spec_select_body's first pass the fused call takes (register: at most 16 x 1024 entries and at most eight
high-byte bins; ballot: more bins; loop: more entries) and whether the targets lie in different high bytes (two_hb).

The constants are read from the sources (constants()), so that a changed capacity fails the tests that depend on it
instead of silently testing the old value.
"""
import os
import re

import numpy as np

import select_inputs as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTCOMES = ("hit", "no_window", "lo_below", "lo_above", "hi_above", "overflow", "over_capacity", "empty")
KEY_ZERO, KEY_INF = 0x80000000, 0xff000000          # keys of +0.0 and of +inf: the grant rule's bounds
NO_WINDOW_KEY = 0xffffffff


# ---- constants, from the sources ---------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "stein_amd", "csrc", name)) as f:
        return f.read()


def _constant(text, name, where):
    m = re.search(r"constexpr\s+(?:u32|int)\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, "%s no longer defines %s as a constexpr" % (where, name)
    expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)u\b", r"\1", m.group(1)).replace("/", "//")
    assert re.fullmatch(r"[0-9A-Fa-fx\s()<+*/-]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}))       # (digits, brackets and operators only)


_CONSTANTS = None


def constants():
    """SPEC_QCAP, SPEC_CAP, SPEC_SLOTS, SPEC_HW_MAX, SPEC_TABLE_HDR (stein_common.h), DP_QCAP (stein_dpanel.hip), EPT
    (spec_select_body, stein_select.hip) and what follows from them"""
    global _CONSTANTS
    if _CONSTANTS is None:
        common, panel, select = _source("stein_common.h"), _source("stein_dpanel.hip"), _source("stein_select.hip")
        c = {k: _constant(common, k, "stein_common.h") for k in ("SPEC_QCAP", "SPEC_CAP", "SPEC_SLOTS", "SPEC_HW_MAX",
                                                                 "SPEC_TABLE_HDR")}
        c["DP_QCAP"] = _constant(panel, "DP_QCAP", "stein_dpanel.hip")
        c["EPT"] = _constant(select, "EPT", "stein_select.hip")
        assert re.search(r"sx\.qn\s*>=\s*\(u32\)\(DP_QCAP\s*/\s*2\)", panel), "the panel kernel no longer flushes at DP_QCAP / 2"
        assert re.search(r"cnt\s*<=\s*1024u\s*\*\s*EPT", select), "spec_select_body no longer holds 1024 x EPT entries in registers"
        # a wave of the panel kernel flushes its queue behind a strip that left DP_QCAP / 2 entries or more in it, so it
        # enters a strip with less than that: a strip can queue DP_QCAP - (DP_QCAP / 2 - 1) entries whatever came before
        c["DP_STRIP_SAFE"] = c["DP_QCAP"] - (c["DP_QCAP"] // 2 - 1)
        c["INREG"] = 1024 * c["EPT"]
        c["SPEC_TABLE"] = c["SPEC_TABLE_HDR"] + 2 * c["SPEC_HW_MAX"] + 2
        _CONSTANTS = c
    return dict(_CONSTANTS)


# ---- multisets: keys, weights and the workgroup that produces every entry ----------------------------------------------
class Entries:
    """A weighted multiset of fp32 values as the producing kernels see it: key, weight, and for both tile geometries the
    queue an entry goes to (per-tile kernels: one 128 x 128 tile per workgroup; panel kernel: one [128][32] strip at a
    time per wave)."""

    def __init__(self, values, weights, tile, strip, n):
        self.n = n
        self.values = np.asarray(values, dtype=np.float32)
        self.keys = si.f32_key(self.values).astype(np.int64)
        self.w = np.asarray(weights, dtype=np.int64)
        self.tile, self.strip = np.asarray(tile, dtype=np.int64), np.asarray(strip, dtype=np.int64)
        self.total = int(self.w.sum())
        self.lo, self.hi, self.med = si.exact_median(self.values, self.w)
        self.key_lo, self.key_hi = int(si.f32_key(self.lo)), int(si.f32_key(self.hi))
        self.distinct = np.unique(self.keys)
        self._sorted = None

    def targets(self, total=None):
        """(lo, hi, med) at the target ranks of `total` (the staged calls take it as an argument; default: the weight of
        the multiset), by a sort"""
        if total is None or total == self.total:
            return self.lo, self.hi, self.med
        if self._sorted is None:
            order = np.argsort(self.keys, kind="stable")
            self._sorted = (self.values[order], np.cumsum(self.w[order]))
        v, cum = self._sorted
        r0, r1 = si.target_ranks(total)
        assert r1 < cum[-1]
        lo, hi = v[np.searchsorted(cum, r0, side="right")], v[np.searchsorted(cum, r1, side="right")]
        return np.float32(lo), np.float32(hi), (np.float32(0.5) * (lo + hi) if r0 != r1 else np.float32(lo))


def entries_sym(D):
    """upper-triangle rule over a symmetric int64 D: weight 2 above the diagonal, 1 on it"""
    n = D.shape[0]
    r, c = np.triu_indices(n)
    nt32 = (n + 31) // 32
    return Entries(D[r, c], np.where(r == c, 1, 2), (r // 128) * nt32 + c // 128, (r // 128) * nt32 + c // 32, n)


def entries_rows(D, row0, nl):
    """rows [row0, row0 + nl) of D as a rectangular block, weight 1; the tiles start at the block's first row"""
    n = D.shape[1]
    r, c = np.indices((nl, n))
    r, c = r.reshape(-1), c.reshape(-1)
    nt32 = (n + 31) // 32
    return Entries(D[row0:row0 + nl].reshape(-1), np.ones(r.size, dtype=np.int64), (r // 128) * nt32 + c // 128,
                   (r // 128) * nt32 + c // 32, n)


def entries_blocks(D, bounds):
    """row blocks [(row0, n_local), ...] of D, every one a rectangular block with tiles (and queues) of its own"""
    parts = [entries_rows(D, row0, nl) for row0, nl in bounds]
    step = max(int(max(p.tile.max(), p.strip.max())) for p in parts) + 1
    return Entries(np.concatenate([p.values for p in parts]), np.concatenate([p.w for p in parts]),
                   np.concatenate([p.tile + k * step for k, p in enumerate(parts)]),
                   np.concatenate([p.strip + k * step for k, p in enumerate(parts)]), D.shape[1])


def entries_image(M, upper):
    """the same for an fp32 image the kernel stored (counting proof on the kernel's own values)"""
    M = np.asarray(M, dtype=np.float32)
    nl, n = M.shape
    nt32 = (n + 31) // 32
    if upper:
        r, c = np.triu_indices(n)
        return Entries(M[r, c], np.where(r == c, 1, 2), (r // 128) * nt32 + c // 128, (r // 128) * nt32 + c // 32, n)
    r, c = np.indices((nl, n))
    r, c = r.reshape(-1), c.reshape(-1)
    return Entries(M.reshape(-1), np.ones(r.size, dtype=np.int64), (r // 128) * nt32 + c // 128, (r // 128) * nt32 + c // 32, n)


# ---- the model ----------------------------------------------------------------------------------------------------
def grant(center, halfwidth, magic_ok=True):
    """(lo_key, width) as median_init_body words it"""
    hw_max = constants()["SPEC_HW_MAX"]
    if magic_ok and halfwidth <= hw_max and KEY_ZERO + halfwidth <= center < KEY_INF - halfwidth:
        return center - halfwidth, 2 * halfwidth
    return NO_WINDOW_KEY, 0


class Step:
    """what one windowed step leaves: see the module's docstring"""


def window_step(ent, center, halfwidth, geometry="tiles", reps=1, total=None):
    """One windowed step over `ent`, submitted `reps` times between one begin and one tally (total defaults to reps x the
    multiset's weight).  geometry: "tiles" or "panel"."""
    c = constants()
    s = Step()
    s.reps, s.geometry = reps, geometry
    s.total = reps * ent.total if total is None else total
    s.r0, s.r1 = si.target_ranks(s.total)
    s.lo_key, s.width = grant(center, halfwidth)
    s.granted = s.width != 0
    s.table = np.zeros(c["SPEC_TABLE_HDR"] + s.width + 1, dtype=np.int64)
    s.below = s.count = s.max_queue = 0
    s.overflow = False
    s.count_exact = True
    s.path, s.two_hb, s.lo, s.hi = None, None, None, None
    if not s.granted:
        s.table[1] = 1
        s.outcome = "no_window"
        return s
    inside = (ent.keys >= s.lo_key) & (ent.keys <= s.lo_key + s.width) & (ent.w > 0)
    s.below = reps * int(ent.w[ent.keys < s.lo_key].sum())
    group = (ent.tile if geometry == "tiles" else ent.strip)[inside]
    per = np.bincount(group) if group.size else np.zeros(1, dtype=np.int64)
    per = per[per > 0] if (per > 0).any() else np.zeros(1, dtype=np.int64)
    s.max_queue = int(per.max())
    if geometry == "tiles":
        s.capacity = c["SPEC_QCAP"]
        s.overflow = s.max_queue > s.capacity
        s.count = reps * int(np.minimum(per, s.capacity).sum())
    else:
        # a wave enters a strip with at most DP_QCAP / 2 - 1 entries queued: no overflow while every strip stays within
        # DP_STRIP_SAFE; a strip with more than DP_QCAP overflows whatever came before.  Between the two the outcome
        # depends on which wave drew which strips: such a case is not run on the panel kernel (Case.panel_ok).
        s.capacity = c["DP_STRIP_SAFE"]
        s.overflow = s.max_queue > s.capacity
        s.panel_decided = s.max_queue <= c["DP_STRIP_SAFE"] or s.max_queue > c["DP_QCAP"]
        s.count = reps * int(per.sum())
        s.count_exact = not s.overflow          # (after an overflow the queues drop what did not fit)
    s.table[0] = s.below
    s.table[2] = s.count
    weight_inside = reps * int(ent.w[inside].sum())
    if s.overflow:
        s.table[1] = 1
        s.outcome = "overflow"
        return s
    if s.count > c["SPEC_CAP"]:
        s.table[1] = 1
        s.outcome = "over_capacity"
        return s
    s.table[c["SPEC_TABLE_HDR"]:] = reps * np.bincount(ent.keys[inside] - s.lo_key, weights=ent.w[inside],
                                                       minlength=s.width + 1).astype(np.int64)
    if s.count == 0:
        s.outcome = "empty"
    elif s.r0 < s.below:
        s.outcome = "lo_below"
    elif s.r0 - s.below >= weight_inside:
        s.outcome = "lo_above"
    elif s.r1 - s.below >= weight_inside:
        s.outcome = "hi_above"
    else:
        s.outcome = "hit"
        cum = np.cumsum(s.table[c["SPEC_TABLE_HDR"]:])
        k0 = int(np.searchsorted(cum, s.r0 - s.below, side="right"))
        k1 = int(np.searchsorted(cum, s.r1 - s.below, side="right"))
        s.lo = np.float32(si.key_f32(np.uint32(s.lo_key + k0)))
        s.hi = np.float32(si.key_f32(np.uint32(s.lo_key + k1)))
        s.two_hb = (k0 >> 8) != (k1 >> 8)
        nb = (s.width >> 8) + 1
        s.path = "loop" if s.count > c["INREG"] else ("register" if nb <= 8 else "ballot")
    return s


def predictor_update(before, key_lo, width, hit, count):
    """spec_update_dev's rule as stein_common.h and DESIGN.md describe it, replayed on the host.  before: the state
    words in front of the call (magic, center, halfwidth, earned_hw, last_key, n_steps, n_hits); key_lo: the key of this
    step's lower target; width / hit / count: this step's window words.  -> the words after."""
    c = constants()
    m1, m2 = _magic()
    hw, nxt, earned = 4096, key_lo, 0
    after = dict(before)
    if before["magic"] in (m1, m2):
        lo = np.float32(si.key_f32(np.uint32(key_lo)))
        with np.errstate(over="ignore", invalid="ignore"):
            pred = np.float32(2) * lo - np.float32(si.key_f32(np.uint32(before["last_key"])))
        k = int(si.f32_key(pred if pred == pred else lo))
        nxt = min(max(k, 65536), 0xfffe0000)
        if before["magic"] == m2 and width != 0:
            err = abs(key_lo - before["center"])
            hw = c["SPEC_HW_MAX"] if err > c["SPEC_HW_MAX"] // 4 else 4 * err + 48
            hw = max(hw, before["earned_hw"] - before["earned_hw"] // 4)
            earned = hw
            if hit and count > c["SPEC_CAP"] // 2 and hw > before["halfwidth"] // 2:
                hw = before["halfwidth"] // 2 + 1
        after.update(magic=m2, n_steps=before["n_steps"] + 1, n_hits=before["n_hits"] + (1 if hit else 0))
    else:
        after.update(magic=m1, n_steps=1, n_hits=0)
    after.update(last_key=key_lo, center=nxt, halfwidth=min(hw, c["SPEC_HW_MAX"]), earned_hw=min(earned, c["SPEC_HW_MAX"]))
    return after


def _magic():
    import workspace_state as wsx
    return wsx.spec_magic_words()


# ---- the case table -----------------------------------------------------------------------------------------------------
SCATTER_384_SEED = 13       # the first seed whose targets lie on different values at n = 384 (test_window_cases.py asserts it)
FAMILIES = (("grid", 384), ("scatter", 384), ("line", 384), ("simplex4_64_1", 384), ("grid", 768), ("scatter", 768),
            ("line", 768), ("grid", 1536), ("scatter", 1536))
ROW_BLOCK = (172, 212)      # the non-symmetric form: rows [172, 384), ragged at both ends, the same at every n
EDGES = ("lo_first", "lo_below", "hi_last", "hi_above", "lo_above", "lo_last")


def lattice_points(family, n):
    if family == "scatter" and n not in si.SCATTER_SEED:
        return si.scatter(n, SCATTER_384_SEED)
    return si.lattice(family, n)


_D, _ENTRIES = {}, {}


def lattice_D(family, n):
    if (family, n) not in _D:
        _D[(family, n)] = si.lattice_D(lattice_points(family, n))
    return _D[(family, n)]


def entries_of(family, n, form):
    """form: "sym" (the whole matrix by the upper-triangle rule) or "rows" (ROW_BLOCK as a rectangular block)"""
    if (family, n, form) not in _ENTRIES:
        D = lattice_D(family, n)
        _ENTRIES[(family, n, form)] = entries_sym(D) if form == "sym" else entries_rows(D, *ROW_BLOCK)
    return _ENTRIES[(family, n, form)]


class Case:
    def __init__(self, family, n, form, name, lo_key=None, width=None, center=None, halfwidth=None, expect=None, reps=1,
                 edge=False, total=None):
        if center is None:
            assert width % 2 == 0 and width >= 0, (name, width)
            center, halfwidth = lo_key + width // 2, width // 2
        self.family, self.n, self.form, self.name = family, n, form, name
        self.center, self.halfwidth, self.expect, self.reps, self.edge = int(center), int(halfwidth), expect, reps, edge
        self.total = total          # None: the weight of what is submitted; a number: what spec_begin is told (staged calls only)
        self._steps = {}

    @property
    def id(self):
        return "%s-%d-%s-%s" % (self.family, self.n, self.form, self.name)

    @property
    def entries(self):
        return entries_of(self.family, self.n, self.form)

    def step(self, geometry="tiles"):
        if geometry not in self._steps:
            self._steps[geometry] = window_step(self.entries, self.center, self.halfwidth, geometry, self.reps, self.total)
        return self._steps[geometry]

    def targets(self):
        """(lo, hi, med) the select must return, from a sort"""
        return self.entries.targets(self.total)

    @property
    def panel_ok(self):
        """the panel kernel's outcome does not depend on which wave drew which strip"""
        s = self.step("panel")
        return self.n % 128 == 0 and (not s.granted or s.panel_decided)


def _even_up(x):
    return x + (x & 1)


def placements(family, n, form):
    """the placements of one multiset, every one defined by the reference's key(lo) and key(hi)"""
    c = constants()
    ent = entries_of(family, n, form)
    kl, kh = ent.key_lo, ent.key_hi
    two = kl != kh
    wb = _even_up(kh - kl + 96)                     # the narrowest width used that holds both targets with room to spare
    below = ent.distinct[ent.distinct < kl]
    gap = kl - 1 - int(below[-1]) if below.size else None     # keys from the value in front of lo to the key in front of lo
    above = ent.distinct[ent.distinct > kl]
    reach = int(above[0]) - (kl + 1)                          # keys from the key behind lo to the next value (hi, if lo != hi)
    mk = lambda name, **kw: Case(family, n, form, name, **kw)
    out = []
    heavy = family == "line" or family.startswith("simplex4")
    if heavy:
        # one tile holds more of the targets' tie than a queue does: whatever the placement, a window over the tie overflows
        out.append(mk("tie", center=kl, halfwidth=48 if not two else _even_up(kh - kl) // 2 + 48, expect="overflow"))
        out.append(mk("tie_first", lo_key=kl, width=wb, expect="overflow"))
        out.append(mk("beside_tie", lo_key=kl + 1 + (kh - kl), width=96, expect="empty"))
        out.append(mk("halfwidth_0", center=kl, halfwidth=0, expect="no_window"))
        return out
    # the six edge placements
    out.append(mk("lo_first", lo_key=kl, width=wb, expect="hit", edge=True))
    # (a window without an entry is `empty` before anything is compared: the one that starts behind lo reaches the next value)
    # (... where the widest window can: the integers of [128, 256) lie 65536 keys apart)
    if _even_up(max(wb, reach)) <= 2 * c["SPEC_HW_MAX"]:
        out.append(mk("lo_below", lo_key=kl + 1, width=_even_up(max(wb, reach)), expect="lo_below", edge=True))
    out.append(mk("hi_last", lo_key=kh - wb, width=wb, expect="hit", edge=True))
    if two:
        out.append(mk("hi_above", lo_key=kh - 1 - wb, width=wb, expect="hi_above", edge=True))
        out.append(mk("lo_last", lo_key=kl - wb, width=wb, expect="hi_above", edge=True))
    if gap is not None and _even_up(max(gap, 96)) <= 2 * c["SPEC_HW_MAX"]:
        wa = _even_up(max(gap, 96))
        out.append(mk("lo_above", lo_key=kl - 1 - wa, width=wa, expect="lo_above", edge=True))
    # r0 == below: lo is the very first buffered entry.  The staged calls are told `total`, so the ranks can be put there;
    # the fused call cannot reach it ("Median select, exact": the weight below a window and r0 differ in parity)
    first = int(ent.w[ent.keys < kl].sum())
    out.append(mk("lo_is_first_entry", lo_key=kl, width=wb, total=2 * (first + 1), expect="hit"))
    # the others
    out.append(mk("empty", lo_key=kl - 50, width=48, expect="empty" if gap is None or gap > 50 else None))
    out.append(mk("centred_8192", center=kl, halfwidth=4096, expect="hit" if kh - kl <= 4096 else "hi_above"))
    if two and kh - kl < 1500:
        out.append(mk("register_two_hb", center=kl + (kh - kl) // 2, halfwidth=1000, expect="hit"))
    out.append(mk("halfwidth_0", center=kl, halfwidth=0, expect="no_window"))
    out.append(mk("halfwidth_max", center=kl, halfwidth=c["SPEC_HW_MAX"], expect="hit"))
    out.append(mk("halfwidth_max_plus_1", center=kl, halfwidth=c["SPEC_HW_MAX"] + 1, expect="no_window"))
    # the grant rule's two bounds, failed by one key and passed by zero: the lowest window starts on the key of +0.0 and
    # holds the diagonal's zeros (lo lies above it), the highest ends one key in front of +inf and holds nothing
    out.append(mk("lowest_window", center=KEY_ZERO + 48, halfwidth=48, expect="lo_above"))
    out.append(mk("below_lowest", center=KEY_ZERO + 47, halfwidth=48, expect="no_window"))
    out.append(mk("highest_window", center=KEY_INF - 49, halfwidth=48, expect="empty"))
    out.append(mk("above_highest", center=KEY_INF - 48, halfwidth=48, expect="no_window"))
    if (family, n, form) == ("scatter", 1536, "sym"):
        # more entries than the buffer holds, no queue anywhere near its capacity: the widest window, submitted often enough
        one = window_step(ent, kl, c["SPEC_HW_MAX"]).count
        out.append(mk("over_capacity", center=kl, halfwidth=c["SPEC_HW_MAX"], reps=c["SPEC_CAP"] // one + 1,
                      expect="over_capacity"))
        out.append(mk("under_capacity", center=kl, halfwidth=c["SPEC_HW_MAX"], reps=c["SPEC_CAP"] // one, expect="hit"))
    return out


_TABLE = {}


def case_table(form="sym"):
    if form not in _TABLE:
        _TABLE[form] = [case for family, n in FAMILIES for case in placements(family, n, form)]
    return list(_TABLE[form])
