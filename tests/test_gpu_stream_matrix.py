"""GPU: the streaming RBF and IMQ steps across their dispatch domain -- every case of tests/stream_cases.py
(test_stream_cases.py shows that they reach every class of the run-time choices of k_phi_stream{,_ksd}, k_phi_imq{,_ksd}, the
four finish kernels and k_stream_sum, in every form) against the fp64 sums of stream_cases.reference on the same inputs, over
ALL rows and columns, per 128 x 128 tile and per j range.

Driver: the C ABI through HipStages.svgd_phi_stream{,_ksd} / svgd_phi_imq{,_ksd}, below the engine, so that the test owns the
workspace (sized by the MODEL, with a guard behind it), can misalign theta, phi and the score and can pass phi = NULL.  The
bandwidth is the median heuristic's of the fp64 oracle, rounded to fp32 (four cases: a quarter and four times it).

Checks per case (TOL = test_gpu_conditioning.TOL = 1e-5, the project's parity tolerance):
  path          the library's plan and workspace size equal the model's, under the case's hook
  poison        the workspace (0xFF bytes), phi and the output doubles hold NaN before the call; after it phi, the doubles,
                every O[z], RS[z], the |phi|^2 block partials and (KSD) RD[z] and the S / S_diag block partials are finite --
                anything else is named by its 128 x 128 tile; the guard behind the workspace is untouched
  phi           every 128 x 128 tile: Frobenius error <= 2 TOL |allowance tile|, and per element
                |err| <= TOL (max over the tile of the allowance + the allowance), with the allowance matrix
                |phi_ref| + rowsum(K) |theta| / (h2 n) (RBF: test_gpu_stream.py's test_other_bandwidths, per element) or
                |phi_ref| + rowsum(K3) |theta| / (2 h2 n) (IMQ: imq_ref.phi_allowance, per element)
  ranges        every j range z on its own, read from the workspace at the model's offsets, against the fp64 sums over that
                range's columns: RBF O[z] = K_z (G - theta / h2) per tile within 2 TOL |K_z (|G| + |theta| / h2)|; IMQ O1[z] =
                K_z G and O2[z] = K3_z theta within 2 TOL |K_z |G|| and 2 TOL |K3_z |theta||; RS[z] per 128-row tile within TOL,
                relative; RD[z] = sum_z K D (IMQ: K5 D) per row tile within TOL |sum_z K (r_i + r_j)| (IMQ: K5 in the place
                of K) -- the fp32 Gram distance carries an absolute error in units of r_i + r_j, not of D
  scalars       |phi|^2 within 2e-5 of fp64 (the existing rule); KSD: S and S_diag against stream_ksd_ref.rowsum_sums /
                imq_ref.rowsum_sums over ksd_ref / imq_ref.pairwise_sums' scale within test_gpu_ksd.TOL_F32 = 1e-6, as
                test_gpu_stream_ksd.py and test_gpu_imq.py hold them; every output double against the fp64 sum of its block
                partials within count x 2^-53 of the sum of their magnitudes (k_stream_sum adds at most 1024 doubles)
  consistency   a second call is bit-identical in phi, the doubles and every partial section; the KSD form's phi and |phi|^2
                equal the plain form's to the bit; phi = NULL leaves the three doubles bit-identical; a misaligned theta, phi
                or score gives the aligned call's bits while the finish sums in the same order (vec bit 0 unchanged), and
                stays within the phi and |phi|^2 bounds where the order changes
The allowances follow from the form of the sums (the hi + lo fp16 image is good to about 2^-22, 40 x below TOL), not from the
code under test; the asserted bounds are the project's own, not the observed values.  -s prints every figure as
error / allowance and the module's worst per form and check at the end (recorded in DESIGN.md section 4)."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contract_cases as cc  # noqa: E402
import imq_ref  # noqa: E402
import ksd_ref  # noqa: E402
import stream_cases as sc  # noqa: E402
import stream_ksd_ref  # noqa: E402
import test_gpu_conditioning as tc  # noqa: E402
from test_gpu_ksd import TOL_F32  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import HipStages  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = tc.TOL            # 1e-5
SQ_TOL = 2e-5           # |phi|^2 against fp64 (test_gpu_stream.py, test_gpu_imq.py)
GUARD = 4096            # bytes behind the workspace that no call may touch
IDS = [sc.case_id(c) for c in sc.CASES]
_WORST = {}             # (form, check) -> (largest error / allowance, case id)
_REFS = {}              # (kind, n, d, hook, mult) -> the fp64 reference on the device, shared by the forms
_T0 = [None]

_PLAN = {"rbf": _lib.stream_plan, "imq": _lib.imq_plan}
_BYTES = {("rbf", False): _lib.stream_workspace_bytes, ("rbf", True): _lib.stream_ksd_workspace_bytes,
          ("imq", False): _lib.imq_workspace_bytes, ("imq", True): _lib.imq_ksd_workspace_bytes}


@pytest.fixture(scope="module", autouse=True)
def _print_the_worst_ratios():
    _T0[0] = time.time()
    yield
    _REFS.clear()
    for (form, check), (ratio, where) in sorted(_WORST.items()):
        print("\nworst error / allowance: %-8s %-16s %.3f  (%s)" % (form, check, ratio, where), end="")
    print("\n%d cases in %.1f s" % (len(sc.CASES), time.time() - _T0[0]))


def _note(c, check, ratio):
    ratio = float(ratio)
    key = (sc.form_of(c), check)
    if not ratio <= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (ratio, sc.case_id(c))
    return ratio


# ---------------------------------------------------------------------------------------------------------------
# inputs, references
# ---------------------------------------------------------------------------------------------------------------
def _reference(c, cuda):
    """the fp64 sums of the case's shape, hook and bandwidth on the device, and the statistic's sums and scale: computed once
    and shared by the plain and the KSD form"""
    key = (c.kind, c.n, c.d, c.hook, c.mult)
    if key not in _REFS:
        T64, G64 = sc.inputs(c.n, c.d)
        Td, Gd = torch.tensor(T64, device=cuda), torch.tensor(G64, device=cuda)
        h2 = sc.h2_of(c)
        ref = sc.reference(c.kind, Td, Gd, h2, sc.plan_of(c)["ranges"])
        ref.update(T=Td, G=Gd, h2=h2, sq=float((ref["phi"] * ref["phi"]).sum()))
        _REFS[key] = ref
    return _REFS[key]


def _statistic(c, ref):
    """(S, S_diag, scale) in fp64, once per reference"""
    if "S" not in ref:
        if c.kind == "rbf":
            S, Sd = stream_ksd_ref.rowsum_sums(ref["T"], ref["G"], ref["h2"])
            scale = ksd_ref.pairwise_sums(ref["T"], ref["G"], ref["h2"])[2]
        else:
            S, Sd = imq_ref.rowsum_sums(ref["T"], ref["G"], ref["h2"])[:2]
            scale = imq_ref.pairwise_sums(ref["T"], ref["G"], ref["h2"])[2]
        ref.update(S=S, S_diag=Sd, scale=scale)
    return ref["S"], ref["S_diag"], ref["scale"]


def _matrix(x64, off):
    """x64 as a contiguous float32 [n, d] view that starts on a 16-byte boundary, or (off) 4 bytes behind one"""
    n, d = x64.shape
    base = torch.zeros(n * d + 4, dtype=torch.float32, device=x64.device)
    v = (base[1:1 + n * d] if off else base[:n * d]).view(n, d)
    v.copy_(x64)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 if off else 0)
    return v


# ---------------------------------------------------------------------------------------------------------------
# one call at the ABI on a poisoned workspace, and everything it leaves
# ---------------------------------------------------------------------------------------------------------------
def _call(c, p, ksd, T, G, h2t, misalign, phi_null):
    """-> dict: phi (None if NULL was passed), out (1 or 3 doubles), o [sets][jsplit, n, d], rs, rd (KSD) [jsplit, n],
    sq [sq_blocks], kpart (KSD) [2, sq_blocks] -- clones"""
    n, d, js, dev = c.n, c.d, p["jsplit"], T.device
    sec = sc.sections(c.kind, n, d, js, ksd)
    ws = torch.full((sec["total"] + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    phi = None if phi_null else _matrix(torch.full((n, d), float("nan"), dtype=torch.float64, device=dev), "p" in misalign)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    name = "svgd_phi_%s%s" % ("stream" if c.kind == "rbf" else "imq", "_ksd" if ksd else "")
    getattr(HipStages(), name)(T, G, n, d, h2t, phi, out, ws[:sec["total"]])
    torch.cuda.synchronize()
    assert bool((ws[sec["total"]:] == 0xFF).all()), (sc.case_id(c), name, "wrote behind its workspace")

    def f32(at, *shape):
        count = 1
        for s in shape:
            count *= s
        return ws[at:at + 4 * count].view(torch.float32).view(*shape).clone()

    res = dict(phi=phi, out=out[:3 if ksd else 1].clone(), o=[f32(sec["o%d" % k], js, n, d) for k in range(sc.NSETS[c.kind])],
               rs=f32(sec["rs"], js, n), sq=ws[sec["sq"]:sec["sq"] + 8 * p["sq_blocks"]].view(torch.float64).clone())
    if ksd:
        res["rd"] = f32(sec["rd"], js, n)
        res["kpart"] = ws[sec["kpart"]:sec["kpart"] + 16 * p["sq_blocks"]].view(torch.float64).view(2, p["sq_blocks"]).clone()
    return res


def _assert_finite(tag, res):
    for what in ("phi", "out", "sq", "kpart"):
        if res.get(what) is not None:
            cc.assert_finite(tag, what, res[what])
    for k, o in enumerate(res["o"]):
        for z in range(o.shape[0]):
            cc.assert_finite(tag, "O%d[%d]" % (k + 1, z), o[z])
    for what in ("rs", "rd"):
        if what in res:
            for z in range(res[what].shape[0]):
                cc.assert_finite(tag, "%s[%d]" % (what.upper(), z), res[what][z])


def _same(tag, a, b, keys=None):
    """bit identity of two calls' results (all of them, or `keys`)"""
    for what in keys or sorted(a):
        xs, ys = (a[what], b[what]) if isinstance(a[what], list) else ([a[what]], [b[what]])
        for k, (x, y) in enumerate(zip(xs, ys)):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), \
                (tag, what, k, "differs in %d entries" % int((x != y).sum()))


# ---------------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------------
def _check_tiles(c, tag, what, key, got, ref, allow, factor, lines):
    """every 128 x 128 tile (a vector: every 128-row tile): |err tile| <= factor TOL |allowance tile|"""
    den = sc.tiles(allow)
    assert bool((den > 0).all()), (tag, what, "an all-zero allowance tile")
    ratio = sc.tiles(got.double() - ref) / den / (factor * TOL)
    worst = _note(c, key, ratio.max())
    at = divmod(int(ratio.argmax()), ratio.shape[1]) if ratio.dim() == 2 else (int(ratio.argmax()),)
    lines.append("%s %.3f at %s" % (what, worst, at))
    assert worst <= 1.0, (tag, what, "tile error / (%g TOL x allowance)" % factor, worst, "tile (row tile, column block) %s" % (at,))


def _check_phi(c, tag, phi, ref, lines, key="phi"):
    _check_tiles(c, tag, "phi tile", key + " tile", phi, ref["phi"], ref["phi_allow"], 2.0, lines)
    ratio = (phi.double() - ref["phi"]).abs() / (TOL * (sc.tile_max(ref["phi_allow"]) + ref["phi_allow"]))
    worst = _note(c, key + " elementwise", ratio.max())
    at = divmod(int(ratio.argmax()), ratio.shape[1])
    lines.append("phi elementwise %.3f at %s" % (worst, at))
    assert worst <= 1.0, (tag, "phi elementwise error / allowance", worst, "row %d, column %d" % at)


def _check_sq(c, tag, sq, ref, lines, key="|phi|^2"):
    ratio = _note(c, key, abs(sq - ref["sq"]) / (SQ_TOL * ref["sq"]))
    lines.append("|phi|^2 %.3f" % ratio)
    assert ratio <= 1.0, (tag, "|phi|^2", sq, ref["sq"])


def _check_ranges(c, tag, res, ref, lines):
    names = ("O",) if c.kind == "rbf" else ("O1", "O2")
    for z in range(res["rs"].shape[0]):
        for k, name in enumerate(names):
            _check_tiles(c, tag, "%s[%d]" % (name, z), name + "[z] tile", res["o"][k][z], ref["o"][k][z], ref["o_allow"][k][z], 2.0, lines)
        _check_tiles(c, tag, "RS[%d]" % z, "RS[z] row tile", res["rs"][z], ref["rs"][z], ref["rs"][z], 1.0, lines)
        if "rd" in res:
            _check_tiles(c, tag, "RD[%d]" % z, "RD[z] row tile", res["rd"][z], ref["rd"][z], ref["rd_allow"][z], 1.0, lines)


def _check_block_sums(c, tag, res, lines):
    """k_stream_sum: every output double is the sum of its block partials (any order: count x 2^-53 of their magnitudes)"""
    parts = [res["sq"]] + ([res["kpart"][0], res["kpart"][1]] if "kpart" in res else [])
    worst = 0.0
    for k, part in enumerate(parts):
        allowed = part.numel() * 2.0 ** -53 * float(part.abs().sum())
        err = abs(float(res["out"][k]) - float(part.sum()))
        worst = max(worst, err / allowed if allowed > 0 else (0.0 if err == 0 else float("inf")))
    lines.append("block sums %.3f" % _note(c, "block sums", worst))
    assert worst <= 1.0, (tag, "an output double is not the sum of its block partials", worst)


def _check_statistic(c, tag, res, ref, lines):
    S, Sd, scale = _statistic(c, ref)
    for what, got, want in (("S", float(res["out"][1]), S), ("S_diag", float(res["out"][2]), Sd)):
        ratio = _note(c, what, abs(got - want) / scale / TOL_F32)
        lines.append("%s %.3f" % (what, ratio))
        assert ratio <= 1.0, (tag, what, got, want, scale)


# ---------------------------------------------------------------------------------------------------------------
# the test
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_streaming_case(cuda, case):
    c, p, tag = case, sc.plan_of(case), sc.case_id(case)
    print("\n%s: plan %s ranges %s vec %d; classes %s" % (tag, (p["row_tiles"], p["col_units"], p["jsplit"]), p["ranges"],
                                                         sc.vec(c.d, c.misalign, c.phi_null), " ".join(sorted(sc.classes(c)))))
    ref = _reference(c, cuda)
    h2t = torch.tensor([ref["h2"]], dtype=torch.float32, device=cuda)
    assert float(h2t.item()) == ref["h2"]
    aligned = (_matrix(ref["T"], False), _matrix(ref["G"], False))
    T = _matrix(ref["T"], True) if "t" in c.misalign else aligned[0]
    G = _matrix(ref["G"], True) if "s" in c.misalign else aligned[1]
    lines = []
    try:
        _lib.debug_stream_jsplit(c.hook)
        # the path: the library's plan and sizes are the model's
        assert _PLAN[c.kind](c.n, c.d) == (p["row_tiles"], p["col_units"], p["jsplit"]), tag
        for ksd in (False, True):
            assert _BYTES[c.kind, ksd](c.n, c.d) == sc.sections(c.kind, c.n, c.d, p["jsplit"], ksd)["total"], (tag, ksd)
        first = _call(c, p, c.ksd, T, G, h2t, c.misalign, c.phi_null)
        _assert_finite(tag, first)
        _same(tag + " second call", _call(c, p, c.ksd, T, G, h2t, c.misalign, c.phi_null), first)
        base = first
        if c.misalign or c.phi_null:
            # the aligned call with phi: the same sums; the same bits wherever the finish adds in the same order
            base = _call(c, p, c.ksd, aligned[0], aligned[1], h2t, "", False)
            _assert_finite(tag + " aligned", base)
            _same(tag + " against the aligned call", first, base, ["o", "rs"] + (["rd"] if c.ksd else []))
            if sc.vec(c.d, c.misalign, c.phi_null) & 1 == sc.vec(c.d) & 1:
                _same(tag + " against the aligned call", first, base, ["out", "sq"] + (["kpart"] if c.ksd else []) +
                      ([] if c.phi_null else ["phi"]))
            else:
                lines.append("vec bit 0 changed: phi bit-identical %s" % torch.equal(first["phi"], base["phi"]))
        if c.ksd:
            # the plain form on the same buffers: phi and |phi|^2 to the bit
            plain = _call(c, p, False, T, G, h2t, c.misalign, False)
            _assert_finite(tag + " plain form", plain)
            with_phi = first if not c.phi_null else base
            assert torch.equal(plain["phi"], with_phi["phi"]), (tag, "the KSD form's phi is not the plain form's")
            assert torch.equal(plain["out"], first["out"][:1]), (tag, "the KSD form's |phi|^2 is not the plain form's")
    finally:
        _lib.debug_stream_jsplit(0)
    # against fp64
    if not c.phi_null:
        _check_phi(c, tag, first["phi"], ref, lines)
    else:
        _check_phi(c, tag, base["phi"], ref, lines)         # (the aligned call's: its doubles are this call's, bit for bit)
    _check_sq(c, tag, float(first["out"][0]), ref, lines)
    _check_ranges(c, tag, first, ref, lines)
    _check_block_sums(c, tag, first, lines)
    if c.ksd:
        _check_statistic(c, tag, first, ref, lines)
    print("%s: error / allowance: %s" % (tag, "; ".join(lines)))
