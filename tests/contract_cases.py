"""Case tables of the split contraction kernel (k_phi_x3fs, csrc/stein_x3.hip) and a model of its run-time dispatch (a
helper of test_contract_cases.py and test_gpu_contract_matrix.py, not a test).

k_phi_x3fs picks much of its code path at run time from (n, n_local, d, split, jchunk, upper).  `classify` restates the
plan (stein_make_layout: tiles_m, cblocks, wpm, split, jchunk) and the kernel's predicates so that the table below can be
shown -- by assertion, in test_contract_cases.py -- to reach every one of them in every operand form; it DESCRIBES cases
and is never a yardstick for a result (the GPU tests compare with the fp64 formulae).  Where it names a split or a range
count, test_contract_cases.py asks the library's own layout calls, and every GPU case asserts the path it took first.

    launch      map     "xcd" (wpm > 4, wpm % 4 == 0, tiles_m % 8 == 0: 8 row tiles x 4 column blocks per 32 ids) | "plain"
                rot     class of wpm: "1", "2", "3", "4+"  (rot = (cb % 4) * (wpm >= 4 ? 1 : 4 / wpm) % 4, full stages only)
                cblocks odd | even (fold: the spare half workgroup of an odd count stores nothing)
                theta   fold with dK or the statistic: tiles_m x wpm more workgroups over the whole j range
    j range     ntile, nstage = ceil(ntile / 4), tile tail ntile % 4, column tail (jend - jbeg) % 32,
                permute / xmask per row tile, ntr per row tile (stages read from the mirror image)

Operand forms: "unfolded" (fp32 inputs, K.[G | theta]), "bf16" (the same kernel's one-plane instantiation), "fold" (fp32
inputs, K.W); a row block (n_local < n, upper = 0) is an unfolded or a bf16 case."""
import math
from collections import namedtuple

import numpy as np

BM = BN = 128               # copies of the constants of stein_common.h / stein_x3.hip / stein_host.h
BK, FS_KT = 32, 4
RESIDENT = 256.0            # RESIDENT_ONE_PER_CU
SMALL_MAXN = 160            # the one-kernel path's reach: small=False wherever n <= 160


def choose_split(n, base_wgs, forced=0):
    """(ranges, jchunk) of stein_make_layout's rule on the split path; forced: stein_debug_fold_split's count"""
    jt = (n + BK - 1) // BK
    max_split = min(16, max(1, jt // 8))
    split, best = 1, -1.0
    if forced > 0:
        split = min(forced, jt)
    else:
        for s in range(1, max_split + 1):
            rounds = float(base_wgs * s) / RESIDENT
            eff = rounds / math.ceil(rounds) - 0.004 * float(s - 1)
            if eff > best + 1e-9:
                best, split = eff, s
    tiles_per = ((jt + split - 1) // split + 3) // 4 * 4
    return (jt + tiles_per - 1) // tiles_per, tiles_per * BK


def _range(n, jbeg, jend, tiles_m, wpm, upper, fold):
    ntile = (jend - jbeg + BK - 1) // BK if jend > jbeg else 0
    nstage = (ntile + FS_KT - 1) // FS_KT
    group = 32 // wpm if wpm <= 32 else 1
    permute = bool(upper and (fold or (jbeg == 0 and jend == n and nstage == tiles_m)) and wpm & (wpm - 1) == 0 and
                   wpm <= 4 and nstage * FS_KT == ntile and nstage & (nstage - 1) == 0 and nstage >= 2 * group)
    return dict(jbeg=jbeg, jend=jend, ntile=ntile, nstage=nstage, tile_tail=ntile % FS_KT, col_tail=(jend - jbeg) % BK,
                permute=permute, group=group,
                xmask=[tm & ~(group - 1) & (nstage - 1) if permute else 0 for tm in range(tiles_m)],
                ntr=[max(0, min(nstage, (tm * BM - jbeg) // (FS_KT * BK))) if upper else 0 for tm in range(tiles_m)])


def classify(n, d, n_local=None, fold=False, fold_ranges=0, upper=True, with_theta=False):
    """the plan and the code path of one k_phi_x3fs launch"""
    n_local = n if n_local is None else n_local
    assert not fold or (n_local == n and upper), "the fold is the single-rank fused call's"
    assert fold or not with_theta
    tiles_m, cblocks = (n_local + BM - 1) // BM, (d + BN - 1) // BN
    wpm = (cblocks + 1) // 2 if fold else cblocks
    split, jchunk = choose_split(n, tiles_m * wpm, fold_ranges if fold else 0)
    ranges = [_range(n, z * jchunk, min(n, (z + 1) * jchunk), tiles_m, wpm, upper, fold) for z in range(split)]
    return dict(n=n, d=d, n_local=n_local, fold=fold, upper=upper, tiles_m=tiles_m, cblocks=cblocks, wpm=wpm, split=split,
                jchunk=jchunk, ranges=ranges,
                theta_range=_range(n, 0, n, tiles_m, wpm, upper, fold) if with_theta else None,
                map="xcd" if wpm > 4 and wpm % 4 == 0 and tiles_m % 8 == 0 else "plain",
                rot="4+" if wpm >= 4 else str(wpm), cblocks_odd=cblocks % 2 == 1, theta=bool(with_theta),
                grid=tiles_m * wpm * (split + (1 if with_theta else 0)))


def workgroup(c, logical):
    """logical workgroup id (behind xcd_remap) -> (row tile, column block, range, half) as the kernel derives them"""
    plane = c["wpm"] * c["tiles_m"]
    half = 1 if c["fold"] and logical >= plane * c["split"] else 0
    lw = logical - half * plane * c["split"]
    l2, z = lw % plane, lw // plane
    if c["map"] == "xcd":
        sb, inn, cgroups = l2 >> 5, l2 & 31, c["wpm"] >> 2
        return (sb // cgroups) * 8 + (inn >> 2), (sb % cgroups) * 4 + (inn & 3), z, half
    return l2 // c["wpm"], l2 % c["wpm"], z, half


# ---- the cases ------------------------------------------------------------------------------------------------------------
# form: "unfolded" | "bf16" | "fold";  n_local / row0: a row block (upper = 0) when n_local < n;  k: the fold's forced range
# count (0: the library's rule);  dk: the call asks for dK (fold: that brings the theta workgroups)
Case = namedtuple("Case", "form n d n_local row0 k dk")


def _c(form, n, d, dk, n_local=None, row0=0, k=0):
    return Case(form, n, d, n if n_local is None else n_local, row0, k, dk)


CASES = [
    # -- unfolded, fp32: short ranges, every wpm class, the tails
    _c("unfolded", 20, 7, True), _c("unfolded", 40, 5, False), _c("unfolded", 70, 200, True), _c("unfolded", 96, 129, False),
    _c("unfolded", 129, 127, True), _c("unfolded", 161, 1, False), _c("unfolded", 223, 300, True),
    _c("unfolded", 255, 48, False), _c("unfolded", 289, 385, True),
    _c("unfolded", 961, 897, True), _c("unfolded", 1024, 1024, False), _c("unfolded", 8192, 385, True),
    # -- row blocks (upper = 0)
    _c("unfolded", 2048, 1024, False, n_local=1024, row0=1024), _c("unfolded", 1990, 897, True, n_local=961, row0=517),
    _c("unfolded", 700, 255, True, n_local=255, row0=128),
    # -- bf16
    _c("bf16", 20, 7, False), _c("bf16", 40, 5, True), _c("bf16", 70, 200, False), _c("bf16", 129, 127, True),
    # (the ragged XCD shapes have d = 1023 here, not 897: K is rounded to bf16 and is nearly constant along a row at this d, so
    # the partial sum of a j range that misses the diagonal is c * sum_j x_j plus little -- in a ONE-column last block that
    # is one random number per range and matrix for all rows, near zero often enough that the rounding of K alone passes
    # the tile bound on most seeds; test_contract_cases.py holds the documented bf16 arithmetic to half the bound instead)
    _c("bf16", 223, 300, False), _c("bf16", 255, 48, True), _c("bf16", 289, 385, False), _c("bf16", 961, 1023, True),
    _c("bf16", 1024, 1024, True), _c("bf16", 8192, 385, False),
    _c("bf16", 1990, 1023, False, n_local=961, row0=517), _c("bf16", 2048, 1024, True, n_local=1024, row0=1024),
    # -- folded
    _c("fold", 20, 7, False), _c("fold", 40, 129, True), _c("fold", 70, 200, False, k=3), _c("fold", 129, 127, True),
    _c("fold", 223, 300, True), _c("fold", 255, 641, False), _c("fold", 289, 385, True), _c("fold", 640, 130, True, k=3),
    _c("fold", 640, 130, False, k=4),
    _c("fold", 961, 1800, True), _c("fold", 1024, 2048, False),
    _c("fold", 2048, 1024, False, k=1), _c("fold", 2048, 1024, True, k=0), _c("fold", 2017, 769, True, k=1),
    _c("fold", 4096, 300, False, k=1), _c("fold", 4096, 1024, True, k=2),
]

# 2048 x 1024 folded: one permuted range (k = 1) against the library's four unpermuted ones, on the same planes
PERMUTE_PAIR = (_c("fold", 2048, 1024, False, k=1), _c("fold", 2048, 1024, True, k=0))


def case_id(c):
    rows = "" if c.n_local == c.n else "-rows%d+%d" % (c.row0, c.n_local)
    return "%s-%dx%d%s%s%s" % (c.form, c.n, c.d, rows, "-k%d" % c.k if c.form == "fold" else "", "-dK" if c.dk else "")


def classify_case(c):
    fold = c.form == "fold"
    return classify(c.n, c.d, c.n_local, fold=fold, fold_ranges=c.k, upper=c.n_local == c.n, with_theta=fold and c.dk)


def classes(c):
    """the named classes ("Contraction kernel, every path") that a case reaches"""
    m = classify_case(c)
    out = {"map_" + m["map"], "rot_wpm" + m["rot"], "cblocks_odd" if m["cblocks_odd"] else "cblocks_even",
           "d%16==0" if c.d % 16 == 0 else "d%16!=0", "with_dK" if c.dk else "without_dK"}
    every = m["ranges"] + ([m["theta_range"]] if m["theta_range"] else [])
    if m["map"] == "xcd":
        out.add("map_xcd_aligned" if c.n % 128 == c.n_local % 128 == c.d % 128 == 0 else "map_xcd_ragged")
        if c.n % 128 and c.n_local % 128 and c.d % 128:
            out.add("map_xcd_ragged_in_n_nlocal_d")
    if m["wpm"] >= 4 and any(r["ntile"] >= 2 * FS_KT for r in every):
        out.add("rot_all_four_rotations")
    for r in every:
        if r["ntile"] in (1, 2, 3):
            out.add("range_of_%d_tiles" % r["ntile"])
        if r["ntile"] > FS_KT and r["tile_tail"]:
            out.add("last_stage_of_%d_tiles" % r["tile_tail"])
        if r["col_tail"] in (1, 8, 31):
            out.add("last_tile_of_%d_columns" % r["col_tail"])
        if m["upper"]:
            if not any(r["ntr"]):
                out.add("ntr_none")
                if r["jbeg"] > 0 and m["tiles_m"] > 1:
                    out.add("ntr_none_behind_the_diagonal")
            if any(t == r["nstage"] and t > 0 for t in r["ntr"]):
                out.add("ntr_all_stages")
            if any(0 < t < r["nstage"] for t in r["ntr"]):
                out.add("ntr_both_kinds")
    if not m["upper"]:
        out.add("upper0")
        out.add("row0_on_grid" if c.row0 % 128 == 0 else "row0_off_grid")
        if m["split"] > 1 and c.n_local % 128:
            out.add("rows_split_with_ragged_n_local")
    if c.n_local % 128 in (1, 127):
        out.add("n_local%%128==%d" % (c.n_local % 128))
    if c.d % 128 in (1, 127):
        out.add("d%%128==%d" % (c.d % 128))
    if m["fold"]:
        out.add("fold_theta" if m["theta"] else "fold_no_theta")
        if m["cblocks_odd"] and m["cblocks"] in (1, 3, 7, 15):
            out.add("fold_cblocks_%d" % m["cblocks"])
        perm = [r for r in m["ranges"] if r["permute"]]
        if perm and len(perm) == len(m["ranges"]):
            if m["wpm"] == 4:
                out.add("permute_fold_wpm4_%s" % {1: "one_range", 2: "two_ranges"}.get(len(perm), "more_ranges"))
            if m["wpm"] == 2:
                out.add("permute_fold_wpm2")
            if 97 <= c.n % 128 <= 127:
                out.add("permute_fold_ragged_last_tile")
        if m["theta_range"] and m["theta_range"]["permute"] and not perm:
            out.add("permute_theta_only")
        if c.k and m["split"] < min(c.k, (c.n + BK - 1) // BK):
            out.add("fold_dropped_tail")
        if (c.n, c.d) == PERMUTE_PAIR[0][1:3] and m["wpm"] == 4:
            out.add("permute_pair_true" if perm else "permute_pair_false")
    elif any(r["permute"] for r in m["ranges"]):
        assert m["split"] == 1
        out.add("permute_unfolded_split1")
    return out


def form_of(c):
    return c.form


# ---- inputs and the fp64 yardstick ----------------------------------------------------------------------------------------
def inputs(n, d, seed=0):
    """theta, score as float64 arrays of float32 values: normal entries times a seeded scale per matrix
    (test_gpu_random_shapes.py)"""
    rng = np.random.default_rng([20261019, seed, n, d])
    T = rng.normal(size=(n, d)) * rng.uniform(0.3, 3.0)
    G = rng.normal(size=(n, d)) * rng.uniform(0.1, 10.0)
    return T.astype(np.float32).astype(np.float64), G.astype(np.float32).astype(np.float64)


def reference(T, G, h2, row0=0, n_local=None, ranges=None, chunk=1024):
    """The fp64 formulae (tests/test_gpu_baseline_sizes.py: fp64_rows) for the rows [row0, row0 + n_local) over all n
    columns, with torch on T's device in row chunks.  T, G: float64 tensors [n, d]; h2: a float.
    -> dict phi, dK [n_local, d], rs [n_local] = rowsum(K); with ranges = [(jbeg, jend), ...] also the partial sums of
    every j range on its own: part_g, part_t [R, n_local, d], part_rs [R, n_local]."""
    import torch
    n, d = T.shape
    n_local = n if n_local is None else n_local
    ra = (T * T).sum(1)
    phi = torch.empty(n_local, d, dtype=torch.float64, device=T.device)
    dK, rs = torch.empty_like(phi), torch.empty(n_local, dtype=torch.float64, device=T.device)
    parts = None
    if ranges is not None:
        parts = (torch.empty(len(ranges), n_local, d, dtype=torch.float64, device=T.device),
                 torch.empty(len(ranges), n_local, d, dtype=torch.float64, device=T.device),
                 torch.empty(len(ranges), n_local, dtype=torch.float64, device=T.device))
    for lo in range(0, n_local, chunk):
        hi = min(n_local, lo + chunk)
        Ti = T[row0 + lo:row0 + hi]
        K = torch.exp(-(ra[row0 + lo:row0 + hi, None] + ra[None, :] - 2.0 * (Ti @ T.T)) / h2 / 2.0)
        s = K.sum(1)
        KT = K @ T
        rs[lo:hi] = s
        dK[lo:hi] = (s[:, None] * Ti - KT) / h2
        phi[lo:hi] = (K @ G + dK[lo:hi]) / n
        for z, (jb, je) in enumerate(ranges or ()):
            parts[0][z, lo:hi] = K[:, jb:je] @ G[jb:je]
            parts[1][z, lo:hi] = K[:, jb:je] @ T[jb:je]
            parts[2][z, lo:hi] = K[:, jb:je].sum(1)
    out = dict(phi=phi, dK=dK, rs=rs)
    if parts is not None:
        out.update(part_g=parts[0], part_t=parts[1], part_rs=parts[2])
    return out


def tiles(x):
    """[r, c] -> the Frobenius norms of its 128 x 128 tiles, [ceil(r / 128), ceil(c / 128)] (torch, on x's device)"""
    import torch
    r, c = x.shape
    rp, cp = (r + 127) // 128 * 128, (c + 127) // 128 * 128
    full = torch.zeros(rp, cp, dtype=torch.float64, device=x.device)
    full[:r, :c] = x
    return full.view(rp // 128, 128, cp // 128, 128).pow(2).sum(dim=(1, 3)).sqrt()


def assert_finite(tag, what, got):
    """the poison check: what a call left unwritten still holds NaN, and is named by its 128 x 128 tiles"""
    import torch
    bad = ~torch.isfinite(got)
    if bool(bad.any()):
        x = bad if bad.dim() == 2 else bad.reshape(-1, 1)
        where = (tiles(x.double()) > 0).nonzero().tolist()
        raise AssertionError((tag, what, "%d non-finite entries in %d tiles (row tile, column block), the first %s" %
                              (int(bad.sum()), len(where), where[:6])))


def fold_sections(n, d, fsplit, offs, total):
    """Byte offsets (fold_ow, fold_ot, fold_rs) of the folded contraction's partial sums K.W [fsplit][n][d], K.theta [n][d]
    and rowsum(K) [fsplit][n] inside a folding workspace -- stein_make_layout's rule restated (the ABI has no call for
    them): in storage that is dead by then where that fits, else appended to the PLANES section.  `offs`, `total`: what
    stein_workspace_layout gave for the same call; the arm taken is read off the total."""
    a256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    rows, dk, dc, nk = (n + 127) // 128 * 128 + 128, (d + 31) // 32 * 32, (d + 127) // 128 * 128, (n + 31) // 32 * 32
    t3, tt3, scb = a256(3 * rows * dk * 2), a256(3 * dc * nk * 2), a256((6 * dc + 4) * 4)
    ow, ot, rs = a256(fsplit * n * d * 4), a256(n * d * 4), a256(fsplit * n * 4)
    planes, part_g, part_rs = offs[9], offs[4], offs[6]          # WS_PLANES, WS_PART_G, WS_PART_RS
    inside = ow <= part_rs - part_g and ot + rs <= t3
    assert total == a256(planes + t3 + 2 * tt3 + scb + (0 if inside else ow + ot + rs)), "the fold's storage is not where the rule puts it"
    if inside:
        return part_g, planes, planes + ot
    base = planes + t3 + 2 * tt3 + scb
    return base, base + ow, base + ow + ot
