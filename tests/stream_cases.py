"""Case table of the streaming steps (k_phi_stream{,_ksd}, csrc/stein_stream.hip; k_phi_imq{,_ksd}, csrc/stein_imq.hip; the
shared phases, finish pass and k_stream_sum of csrc/stein_stream_tile.h) and a model of what their host side and the kernels
decide at run time (a helper of test_stream_cases.py and test_gpu_stream_matrix.py, not a test).

`plan` restates stream_make_layout (csrc/stein_stream_host.h): row tiles, column units, the wanted range count before and
after its two clamps, the ranges.  `sections` restates its `put` rule: the byte offsets of
r | sc | t3 | planes[..] | o[..] | rs | sq | (rd | kpart).  `vec` restates stream_vec, `xcd_remap` the workgroup map of
stein_common.h.  `classes` names the run-time choices a case reaches ("Streaming steps, every path"),
so that the table below can be shown -- by assertion, in test_stream_cases.py -- to reach every one of them in every form.
The model DESCRIBES cases and says where the partial sums lie; it is never a yardstick for a result: the GPU test compares
with the fp64 sums of `reference`, and test_stream_cases.py holds the model to the library's own plan and size calls.

Forms: "rbf", "rbf-ksd", "imq", "imq-ksd" (the four contraction kernels with their finish kernels)."""
import functools
from collections import namedtuple

import numpy as np

import contract_cases as cc

ROWS = JT = 128             # ST_ROWS, ST_JT (csrc/stein_stream_tile.h)
RESIDENT = 256.0            # RESIDENT_ONE_PER_CU (csrc/stein_host.h)
UNIT = {"rbf": 256, "imq": 128}      # StreamKind::unit: columns of phi one workgroup owns
NSETS = {"rbf": 1, "imq": 2}         # StreamKind::planes and ::osets
N_RESIDUES = (0, 1, 31, 32, 33, 64, 96, 127)


def _ceil(a, b):
    return (a + b - 1) // b


def _a256(b):
    return _ceil(b, 256) * 256


# ---- the plan ------------------------------------------------------------------------------------------------------------
def plan(kind, n, d, hook=0):
    """stream_make_layout's plan; hook: stein_debug_stream_jsplit's count (0: the rule)"""
    row_tiles, cblocks, col_units = _ceil(n, ROWS), _ceil(d, 128), _ceil(d, UNIT[kind])
    jtiles = row_tiles
    want_asked = hook if hook > 0 else int(RESIDENT / float(row_tiles * col_units))
    want = min(max(want_asked, 1), jtiles)
    per = _ceil(jtiles, want)
    jsplit = _ceil(jtiles, per)
    return dict(kind=kind, n=n, d=d, hook=hook, row_tiles=row_tiles, cblocks=cblocks, col_units=col_units, jtiles=jtiles,
                want_asked=want_asked, want=want, jtiles_per=per, jsplit=jsplit,
                ranges=[(z * per, min(jtiles, (z + 1) * per)) for z in range(jsplit)],
                nblk=row_tiles * col_units * jsplit, sq_blocks=min(1024, _ceil(n * d, 1024)))


def sections(kind, n, d, jsplit, ksd):
    """byte offsets of the workspace sections, and `total` (the plain forms: without rd and kpart)"""
    rows, dk, dc = _ceil(n, ROWS) * ROWS, _ceil(d, 32) * 32, _ceil(d, 128) * 128
    sqb = min(1024, _ceil(n * d, 1024))
    out, at = {}, 0

    def put(name, nbytes):
        nonlocal at
        out[name] = at
        at = _a256(at + nbytes)

    put("r", rows * 4)
    put("sc", (6 * dc + 4) * 4)
    put("t3", 3 * rows * dk * 2)
    for p in range(NSETS[kind]):
        put("planes%d" % p, 3 * dc * rows * 2)
    for p in range(NSETS[kind]):
        put("o%d" % p, jsplit * n * d * 4)
    put("rs", jsplit * n * 4)
    put("sq", sqb * 8)
    if ksd:
        put("rd", jsplit * n * 4)
        put("kpart", 2 * sqb * 8)
    out["total"] = at
    return out


def vec(d, misalign="", phi_null=False):
    """stream_vec: bit 0 the 16-byte finish, bit 1 (read by the KSD finish on that path only) an aligned score"""
    v0 = d % 4 == 0 and "t" not in misalign and (phi_null or "p" not in misalign)
    return (1 if v0 else 0) | (0 if "s" in misalign else 2)


def xcd_remap(bid, nblk):
    """stein_common.h's map from the hardware's workgroup id to the logical one"""
    q, r, x = nblk >> 3, nblk & 7, bid & 7
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (bid >> 3)


def workgroup(p, logical):
    """logical id -> (row tile, column unit, range) as both kernels derive them (the column unit fastest)"""
    return (logical // p["col_units"]) % p["row_tiles"], logical % p["col_units"], logical // (p["col_units"] * p["row_tiles"])


# ---- the cases -----------------------------------------------------------------------------------------------------------
# misalign: which of theta ("t"), phi ("p"), score ("s") start 4 bytes off a 16-byte boundary; mult: h2 is the median
# heuristic's value (the fp64 oracle's, rounded to fp32) times this power of two
Case = namedtuple("Case", "kind ksd n d hook misalign phi_null mult")
FORMS = ("rbf", "rbf-ksd", "imq", "imq-ksd")


def _c(form, n, d, hook=0, misalign="", phi_null=False, mult=1.0):
    return Case(form.split("-")[0], form.endswith("-ksd"), n, d, hook, misalign, phi_null, mult)


def _table():
    out = []
    for form in FORMS:
        rbf, ksd = form.startswith("rbf"), form.endswith("-ksd")
        out += [
            _c(form, 1, 1),                                       # one particle: the diagonal alone
            _c(form, 159, 32, misalign="s" if ksd else ""),       # the 16-byte finish (KSD: scalar loads of the score), two ranges
            _c(form, 160, 31),                                    # one k tile of theta, the tail in a wave's second 16 columns
            _c(form, 161, 260, misalign="t" if rbf else "p"),     # d % 4 == 0 on the scalar finish; two column groups
            _c(form, 192, 130),
            _c(form, 224, 144),
            _c(form, 255, 5),
            _c(form, 640, 130, hook=4),                           # ranges of 2, 2, 1 j tiles, the empty fourth dropped
            _c(form, 640, 256, hook=1000, phi_null=ksd),          # the hook clamped to five ranges of one tile
            _c(form, 768, 33, hook=4),                            # three ranges of two tiles
            _c(form, 1000, 300, hook=1),                          # one range by the hook; 293 blocks of the finish pass
            _c(form, 2100, 512),                                  # the finish pass's grid-stride loop under a j split
            _c(form, 4224, 2001 if rbf else 1025),                # one range by the rule: 33 x 8 and 33 x 9 > 256
        ]
    out += [_c("rbf", 640, 130, hook=2), _c("rbf-ksd", 640, 130, hook=3), _c("imq", 640, 130, hook=5),
            _c("imq-ksd", 640, 130, hook=2)]                      # the other hooks at five j tiles: 3 + 2, 2 + 2 + 1, 5 x 1
    out += [_c("rbf", 192, 130, mult=0.25), _c("rbf-ksd", 192, 130, mult=4.0), _c("imq", 192, 130, mult=4.0),
            _c("imq-ksd", 192, 130, mult=0.25)]                   # other bandwidths on a shape of the table
    return out


CASES = _table()


def form_of(c):
    return c.kind + ("-ksd" if c.ksd else "")


def case_id(c):
    return "%s-%dx%d%s%s%s%s" % (form_of(c), c.n, c.d, "-hook%d" % c.hook if c.hook else "",
                                 "-off:" + c.misalign if c.misalign else "", "-phiNULL" if c.phi_null else "",
                                 "-h2x%g" % c.mult if c.mult != 1.0 else "")


def plan_of(c):
    return plan(c.kind, c.n, c.d, c.hook)


def classes(c):
    """the named classes ("Streaming steps, every path") that a case reaches"""
    p = plan_of(c)
    n, d = c.n, c.d
    out = {form_of(c)}
    # columns
    out.add("cg1" if p["col_units"] == 1 else "cg>1")
    if c.kind == "rbf":                      # the second 128-column block of a column group of 256
        if p["cblocks"] % 2 == 1:
            out.add("dead-half")
        if p["cblocks"] >= 2:
            out.add("both-halves")
    tail = d % 128
    if tail:
        out.add("d-tail-in-block")
        if tail < 16:
            out.add("d-tail<16")
        if tail % 32 > 16:
            out.add("d-tail-in-second-16")
        if tail % 32 == 0:
            out.add("d-tail%32==0")
    if d < 32:
        out.add("d<32")
    ntk = _ceil(d, 32)
    if ntk == 1:
        out.add("ntk==1")
    if ntk > 8:
        out.add("ntk>8")
    out.add("d%4==0" if d % 4 == 0 else "d%4!=0")
    # rows / j
    if n % 128 in N_RESIDUES:
        out.add("n%%128==%d" % (n % 128))
    if n < 128:
        out.add("n<128")
    if n == 1:
        out.add("n==1")
    out.add("one-row-tile" if p["row_tiles"] == 1 else "many-row-tiles")
    # ranges
    lens = [b - a for a, b in p["ranges"]]
    if p["jsplit"] == 1 and c.hook == 0 and p["row_tiles"] * p["col_units"] > RESIDENT:
        out.add("jsplit1-by-rule")
    if p["jsplit"] == 1 and c.hook == 1 and p["jtiles"] > 1:
        out.add("jsplit1-by-hook")
    if p["jsplit"] > 1:
        out.add("equal-ranges" if len(set(lens)) == 1 else "ragged-last-range")
    if c.hook > p["jtiles"]:
        out.add("hook-clamped")
    if p["jsplit"] < p["want"]:
        out.add("empty-tails-dropped")
    if 1 in lens:
        out.add("range-of-one-tile")
    if any(x % 2 for x in lens):
        out.add("range-odd")
    if any(x % 2 == 0 for x in lens):
        out.add("range-even")
    # grid
    r8 = p["nblk"] % 8
    out.add("nblk<8" if p["nblk"] < 8 else "nblk%8==0" if r8 == 0 else "nblk%8in1..4" if r8 <= 4 else "nblk%8in5..7")
    # finish
    v = vec(d, c.misalign, c.phi_null)
    if v & 1:
        out.add("vec1")
    else:
        out.add("vec0-by-d" if d % 4 else "vec0-by-misalign")
    if c.ksd:
        if v & 1:                            # (bit 1 is read on the 16-byte path only)
            out.add("ksd-score-aligned" if v & 2 else "ksd-score-misaligned")
        if c.phi_null:
            out.add("phi-null")
            if p["jsplit"] > 1:
                out.add("phi-null-with-jsplit")
    sqb = p["sq_blocks"]
    out.add("sq_blocks==1" if sqb == 1 else "sq_blocks==1024" if sqb == 1024 else "1<sq_blocks<1024")
    if sqb == 1024 and n * d > 1 << 20:
        out.add("finish-grid-stride")
        if p["jsplit"] > 1:
            out.add("finish-grid-stride-with-jsplit")
    if sqb > 256:
        out.add("sq_blocks>256")
    if c.mult != 1.0:
        out.add("other-bandwidth")
    return out


# ---- inputs, the bandwidth and the fp64 yardstick ---------------------------------------------------------------------------
def inputs(n, d):
    """contract_cases.inputs: theta, score as float64 arrays of float32 values"""
    return cc.inputs(n, d)


@functools.lru_cache(maxsize=None)
def heuristic_h2(n, d):
    """the median heuristic's h2 of inputs(n, d) from the fp64 oracle (oracle/svgd_oracle.py), rounded to fp32, as a float.
    One particle has no heuristic (it divides by ln 1): h2 = 1 there -- the lone diagonal entry is k_11 = 1 whatever h2."""
    if n == 1:
        return 1.0
    from oracle import svgd_oracle as orc
    T64, _ = inputs(n, d)
    med = orc.median_all(orc.pairwise_sq_dists(T64, np.float64))
    return float(np.float32(orc.bandwidth_sq(med, n, np.float64)))


def h2_of(c):
    return float(np.float32(heuristic_h2(c.n, c.d) * c.mult))     # (mult is a power of two: still an fp32 value)


def reference(kind, T, G, h2, ranges, chunk=1024):
    """The fp64 sums of one step, with torch on T's device in row chunks (contract_cases.reference's scheme).  T, G: float64
    tensors [n, d] of fp32 values; h2: a float; ranges: the plan's [(jt0, jt1), ...] in j tiles of 128 columns.  With
    K = exp(-D / 2 h2) (rbf) or K = k = (1 + D / 2 h2)^(-1/2), K3 = k^3, K5 = k^5 (imq) and, per range z, K_z the columns of
    the range:

        phi, phi_allow   [n, d]      the direction, and its forward-error allowance |phi| + rs |theta| / (c n), c = h2 (rbf:
                                     rs = rowsum(K)) or 2 h2 (imq: rs = rowsum(K3)): the two terms of that size cancel in phi
        o, o_allow       [S][R, n, d]  rbf: K_z (G - theta / h2), K_z (|G| + |theta| / h2); imq: K_z G and K3_z theta with
                                     K_z |G| and K3_z |theta|
        rs               [R, n]      rowsum(K_z)   (imq: of K3_z)
        rd, rd_allow     [R, n]      sum_z K D     (imq: K5 D), and sum_z K (r_i + r_j) (imq: K5): the fp32 Gram distance
                                     carries an absolute error in units of r_i + r_j"""
    import torch
    n, d = T.shape
    R, dev = len(ranges), T.device
    ra = (T * T).sum(1)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)   # noqa: E731
    nsets = NSETS[kind]
    out = dict(phi=new(n, d), phi_allow=new(n, d), o=[new(R, n, d) for _ in range(nsets)],
               o_allow=[new(R, n, d) for _ in range(nsets)], rs=new(R, n), rd=new(R, n), rd_allow=new(R, n))
    W, Wa, Ga, Ta = G - T / h2, G.abs() + T.abs() / h2, G.abs(), T.abs()
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        rows = slice(lo, hi)
        D = ra[rows, None] + ra[None, :] - 2.0 * (T[rows] @ T.T)
        if kind == "rbf":
            K = torch.exp(-D / (2.0 * h2))
            Ks, Kd = K, K
        else:
            D = D.clamp_min(0.0)
            K = (1.0 + D / (2.0 * h2)) ** -0.5
            Ks = K * K * K
            Kd = Ks * K * K
        rsum = ra[rows, None] + ra[None, :]
        for z, (jt0, jt1) in enumerate(ranges):
            cols = slice(jt0 * JT, min(n, jt1 * JT))
            if kind == "rbf":
                out["o"][0][z, rows] = K[:, cols] @ W[cols]
                out["o_allow"][0][z, rows] = K[:, cols] @ Wa[cols]
            else:
                out["o"][0][z, rows] = K[:, cols] @ G[cols]
                out["o_allow"][0][z, rows] = K[:, cols] @ Ga[cols]
                out["o"][1][z, rows] = Ks[:, cols] @ T[cols]
                out["o_allow"][1][z, rows] = Ks[:, cols] @ Ta[cols]
            out["rs"][z, rows] = Ks[:, cols].sum(1)
            out["rd"][z, rows] = (Kd[:, cols] * D[:, cols]).sum(1)
            out["rd_allow"][z, rows] = (Kd[:, cols] * rsum[:, cols]).sum(1)
    rs = out["rs"].sum(0)[:, None]
    if kind == "rbf":
        out["phi"] = (out["o"][0].sum(0) + rs * T / h2) / n
        out["phi_allow"] = out["phi"].abs() + rs * Ta / (h2 * n)
    else:
        out["phi"] = (out["o"][0].sum(0) + (rs * T - out["o"][1].sum(0)) / (2.0 * h2)) / n
        out["phi_allow"] = out["phi"].abs() + rs * Ta / (2.0 * h2 * n)
    return out


def tiles(x):
    """contract_cases.tiles, and for a vector [r] the norms of its 128-row tiles, [ceil(r / 128)]"""
    return cc.tiles(x) if x.dim() == 2 else cc.tiles(x[:, None])[:, 0]


def tile_max(x):
    """[r, c] -> the largest entry of every 128 x 128 tile, spread back over the tile's entries: [r, c]"""
    import torch
    r, c = x.shape
    rp, cp = _ceil(r, 128) * 128, _ceil(c, 128) * 128
    full = torch.zeros(rp, cp, dtype=torch.float64, device=x.device)
    full[:r, :c] = x
    m = full.view(rp // 128, 128, cp // 128, 128).amax(dim=(1, 3), keepdim=True)
    return m.expand(rp // 128, 128, cp // 128, 128).reshape(rp, cp)[:r, :c]
