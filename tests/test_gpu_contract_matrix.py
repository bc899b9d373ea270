"""GPU: the split contraction kernel (k_phi_x3fs, csrc/stein_x3.hip) across its dispatch domain -- every case of
tests/contract_cases.py (test_contract_cases.py shows that they reach every class of the kernel's run-time choices: the
two workgroup maps, the four rotation classes, the stage permutation, mirrored stages, every tail, the fold's extras, row
blocks) against the fp64 formulae on the same inputs at the bandwidth the device reported, over ALL rows and columns.

Drivers: unfolded and bf16, upper: SvgdEngine(fold=False, small=False); row blocks: _RowBlock of test_gpu_conditioning.py
(stein_contract_partial / _finish, upper = 0); folded: SvgdEngine(fold=True, small=False) under stein_debug_fold_split.
Every case asserts first that it took the path it names (eng.fold, the folded word of the SELECT section, the split).

Checks per case (phi, and dK where the case asks for it; TOL = 1e-5, the project's parity tolerance; bf16: 4e-3):
  poison        phi, dK and the workspace hold NaN before the call; everything that comes back is finite
  tiles         every 128 x 128 output tile on its own: relative Frobenius error <= 2 TOL (check_rows' column-block bound)
  elementwise   |diff| <= TOL (max|ref| + |ref|) over the whole matrix (check_rows' bound)
  columns       _check_columns of test_gpu_conditioning.py (bf16: the same per-column 2-norms at 4e-3)
  row sums      rowsum(K) per 128-row tile within TOL; unfolded and row blocks: PART_RS[z], PART_G[z], PART_T[z] of every
                j range on its own against the fp64 sums over that range's columns; folded: the whole sum
  consistency   a second call on the same engine is bit-identical; folded: phi with dK equals phi without it to the bit
The asserted bounds are the project's own, not the observed values; -s prints every figure as error / allowance and the
module's worst per check and operand form at the end (recorded in DESIGN.md section 4)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import contract_cases as cc  # noqa: E402
import test_gpu_conditioning as tc  # noqa: E402
import workspace_state as wsx  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import HipStages, SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = tc.TOL            # 1e-5
TOL_BF16 = 4e-3         # the project's bf16 bound (test_gpu_x3.py, test_gpu_baseline_sizes.py)
IDS = [cc.case_id(c) for c in cc.CASES]
_WORST = {}             # (form, check) -> (largest error / allowance, case id)
_PAIR_PHI = {}          # the two cases of cc.PERMUTE_PAIR: (phi, reference phi)


@pytest.fixture(scope="module", autouse=True)
def _print_the_worst_ratios():
    yield
    for (form, check), (ratio, where) in sorted(_WORST.items()):
        print("\nworst error / allowance: %-9s %-22s %.3f  (%s)" % (form, check, ratio, where), end="")
    print()


def _note(c, check, ratio):
    ratio = float(ratio)
    key = (c.form if c.n_local == c.n else c.form + "-rows", check)
    if ratio > _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (ratio, cc.case_id(c))
    return ratio


def _tol(c):
    return TOL_BF16 if c.form == "bf16" else TOL


_tiles, _assert_finite = cc.tiles, cc.assert_finite      # (shared with test_gpu_stream_matrix.py)


def _check_matrix(c, tag, what, got, ref, tol, elementwise=True):
    """checks 1-3 of one output matrix (or of one range's partial sums) against its fp64 reference"""
    _assert_finite(tag, what, got)
    diff = got.double() - ref
    den = _tiles(ref)
    assert bool((den > 0).all()), (tag, what, "an all-zero reference tile")
    ratio = _tiles(diff) / den / (2 * tol)
    worst = _note(c, what + " tile", ratio.max())
    at = divmod(int(ratio.argmax()), ratio.shape[1])
    line = "%s: %s worst tile %.3f of 2 TOL at tile %s" % (tag, what, worst, at)
    assert worst <= 1.0, (tag, what, "tile Frobenius error / (2 TOL)", worst, "row tile %d, column block %d" % at)
    if elementwise:
        e = _note(c, what + " elementwise", (diff.abs() / (tol * (ref.abs().max() + ref.abs()))).max())
        line += ", elementwise %.3f" % e
        assert e <= 1.0, (tag, what, "elementwise error / allowance", e)
    print(line)


def _check_rowsums(c, tag, what, got, ref, tol):
    """rowsum(K) per 128-row tile: relative 2-norm error within TOL"""
    _assert_finite(tag, what, got)
    ratio = _tiles((got.double() - ref)[:, None])[:, 0] / _tiles(ref[:, None])[:, 0] / tol
    worst = _note(c, what, ratio.max())
    print("%s: %s worst row tile %.3f of TOL (row tile %d)" % (tag, what, worst, int(ratio.argmax())))
    assert worst <= 1.0, (tag, what, worst, int(ratio.argmax()))


def _check_columns(c, tag, what, got, ref, T64):
    if c.form != "bf16":
        worst = tc._check_columns(tag, got.double().cpu().numpy(), ref.cpu().numpy(), T64, what)
        _note(c, what + " column", worst / TOL)
        return
    err, live = ci.column_errors(got.double().cpu().numpy(), ref.cpu().numpy())
    assert live.all(), (tag, what, "a zero reference column")      # normal inputs: nothing is excluded
    print("%s: %s worst column %.2e (column %d)" % (tag, what, err.max(), int(err.argmax())))
    assert _note(c, what + " column", err.max() / TOL_BF16) <= 1.0, (tag, what, float(err.max()), int(err.argmax()))


def _check_outputs(c, tag, phi, dK, rs, ref, T64):
    tol = _tol(c)
    for what, got in (("phi", phi), ("dK", dK)):
        if got is not None:
            _check_matrix(c, tag, what, got, ref[what], tol)
            _check_columns(c, tag, what, got, ref[what], T64)
    _check_rowsums(c, tag, "rowsum(K)", rs, ref["rs"], tol)


def _check_partials(c, tag, parts, ref, tol):
    """every j range on its own: the true-unit partial sums of the PART sections against the fp64 sums over its columns"""
    for z in range(parts[0].shape[0]):
        _check_matrix(c, tag, "PART_G[%d]" % z, parts[0][z], ref["part_g"][z], tol, elementwise=False)
        _check_matrix(c, tag, "PART_T[%d]" % z, parts[1][z], ref["part_t"][z], tol, elementwise=False)
        _check_rowsums(c, tag, "PART_RS[%d]" % z, parts[2][z], ref["part_rs"][z], tol)


def _inputs(c, cuda):
    """(theta, score as the call gets them, the same values in fp64 on the device, theta in fp64 on the host)"""
    T64, G64 = cc.inputs(c.n, c.d)
    dtype = torch.bfloat16 if c.form == "bf16" else torch.float32
    T, G = tc._dev(T64, cuda, dtype), tc._dev(G64, cuda, dtype)
    return T, G, T.double(), G.double(), T.double().cpu().numpy()


def _nan(*shape, device):
    return torch.full(shape, float("nan"), device=device)


def _folded_word(eng):
    return eng.select_state_bytes(_lib.FUSE_FOLDED_OFFSET, 4).view(torch.int32).item()


def _engine_call(tag, eng, T, G, dk):
    """one fused call on a workspace and outputs that hold NaN -> clones of phi, dK (None unless asked for), h2"""
    wsx.poison(eng, "ones", keep_select=False)
    wsx.scrub_outputs(eng)
    dK = _nan(eng.n, eng.d, device=eng.device) if dk else None
    eng.compute_phi(T, G, dK_out=dK)
    torch.cuda.synchronize()
    for what, got in (("phi", eng.phi), ("dK", dK), ("h2", eng.h2), ("|phi|^2", eng.sqnorm)):
        if got is not None:
            _assert_finite(tag, what, got)
    return eng.phi.clone(), dK, eng.h2.clone()


def _same(tag, a, b):
    for what, x, y in zip(("phi", "dK", "h2"), a, b):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), \
            (tag, what, "differs in %d entries" % int((x != y).sum()))


# ---------------------------------------------------------------------------------------------------------------
# the three drivers
# ---------------------------------------------------------------------------------------------------------------
def _run_upper(c, m, cuda, tag):
    T, G, Td, Gd, T64 = _inputs(c, cuda)
    eng = SvgdEngine(c.n, c.d, device=cuda, fold=False, small=False, dtype=T.dtype)
    assert not eng.fold and not eng._one_kernel and eng.split == m["split"], (tag, eng.fold, eng.split, m["split"])
    first = _engine_call(tag, eng, T, G, c.dk)
    assert _folded_word(eng) == 0, tag
    parts = tc._partials(eng.ws, eng._offs, eng.split, c.n, c.d)
    _same(tag + " second call", _engine_call(tag, eng, T, G, c.dk), first)
    phi, dK, h2 = first
    ref = cc.reference(Td, Gd, float(h2.item()), ranges=[(r["jbeg"], r["jend"]) for r in m["ranges"]])
    _check_outputs(c, tag, phi, dK, parts[2].double().sum(0), ref, T64)
    _check_partials(c, tag, parts, ref, _tol(c))


class _Shim:
    """a row block as workspace_state.poison wants it"""

    def __init__(self, blk):
        self.ws, self._offs = blk.ws, blk.offs


def _run_rows(c, m, cuda, tag):
    T, G, Td, Gd, T64 = _inputs(c, cuda)
    full = SvgdEngine(c.n, c.d, device=cuda, small=False, dtype=T.dtype)      # the bandwidth of the whole step
    full.compute_phi(T, G)
    h2 = full.h2.clone()
    blk = tc._RowBlock(HipStages(), c.n, c.d, c.row0, c.n_local, cuda)
    dt = _lib.BF16 if c.form == "bf16" else _lib.F32
    assert _lib.workspace_layout(c.n_local, c.n, c.d, dt, _lib.FLAG_X3)[:2] == (blk.ws.numel(), blk.offs), tag
    assert blk.split == m["split"], (tag, blk.split, m["split"])

    def call():
        wsx.poison(_Shim(blk), "ones", keep_select=False)
        blk.partial(T, G, h2)
        phi, sq = _nan(c.n_local, c.d, device=cuda), torch.full((1,), float("nan"), dtype=torch.float64, device=cuda)
        dK = _nan(c.n_local, c.d, device=cuda) if c.dk else None
        blk.st.contract_finish(T, c.n, c.d, c.row0, c.n_local, h2, phi, sq, dK, blk.ws, _lib.FLAG_X3)
        torch.cuda.synchronize()
        for what, got in (("phi", phi), ("dK", dK), ("|phi|^2", sq)):
            if got is not None:
                _assert_finite(tag, what, got)
        return phi, dK, sq

    first = call()
    parts = tc._partials(blk.ws, blk.offs, blk.split, c.n_local, c.d)
    _same(tag + " second call", call(), first)
    ref = cc.reference(Td, Gd, float(h2.item()), c.row0, c.n_local, [(r["jbeg"], r["jend"]) for r in m["ranges"]])
    _check_outputs(c, tag, first[0], first[1], parts[2].double().sum(0), ref, T64)
    _check_partials(c, tag, parts, ref, _tol(c))


def _run_fold(c, m, cuda, tag):
    T, G, Td, Gd, T64 = _inputs(c, cuda)
    try:
        _lib.debug_fold_split(c.k)                # the workspace is sized under the hook, and the calls run under it
        eng = SvgdEngine(c.n, c.d, device=cuda, fold=True, small=False)
        assert eng.fold and not eng._one_kernel, tag
        assert _lib.layout_fold_ranges(c.n, c.n, c.d, _lib.F32, eng.flags) == m["split"], tag
        _, _, at_rs = cc.fold_sections(c.n, c.d, m["split"], eng._offs, eng.ws_bytes)
        first = _engine_call(tag, eng, T, G, c.dk)
        assert _folded_word(eng) == 1, tag
        rs = eng.ws[at_rs:at_rs + m["split"] * c.n * 4].view(torch.float32).view(m["split"], c.n).double().sum(0)
        _same(tag + " second call", _engine_call(tag, eng, T, G, c.dk), first)
        other = _engine_call(tag, eng, T, G, not c.dk)       # with the theta workgroups and without: the W half does not know
        assert torch.equal(other[0], first[0]) and torch.equal(other[2], first[2]), (tag, "phi depends on dK_out")
    finally:
        _lib.debug_fold_split(0)
    phi, dK, h2 = first
    ref = cc.reference(Td, Gd, float(h2.item()))
    _check_outputs(c, tag, phi, dK, rs, ref, T64)
    if c in cc.PERMUTE_PAIR:
        _PAIR_PHI[c] = (phi, ref["phi"])
    return phi, ref["phi"]


@pytest.mark.parametrize("case", cc.CASES, ids=IDS)
def test_contraction_case(cuda, case):
    m = cc.classify_case(case)
    tag = cc.case_id(case)
    print("\n%s: classes %s" % (tag, " ".join(sorted(cc.classes(case)))))
    if case.form == "fold":
        _run_fold(case, m, cuda, tag)
    elif case.n_local < case.n:
        _run_rows(case, m, cuda, tag)
    else:
        _run_upper(case, m, cuda, tag)


def test_permuted_against_unpermuted_stages_on_the_same_planes(cuda):
    """2048 x 1024 folded: one range, its 16 stages permuted per row tile (k = 1), against the library's own four ranges in
    natural order (k = 0).  Same planes, another order of the fp32 sums: each is held to its own bounds against fp64 (the
    cases above, run here if they have not been), and to each other through the sum of the two tile bounds."""
    for c in cc.PERMUTE_PAIR:
        if c not in _PAIR_PHI:
            _run_fold(c, cc.classify_case(c), cuda, cc.case_id(c))
    (a, ra), (b, rb) = (_PAIR_PHI[c] for c in cc.PERMUTE_PAIR)
    ma, mb = (cc.classify_case(c) for c in cc.PERMUTE_PAIR)
    assert [r["permute"] for r in ma["ranges"]] == [True] and [r["permute"] for r in mb["ranges"]] == [False] * 4
    assert torch.equal(ra, rb), "the two cases did not see the same inputs and bandwidth"
    ratio = (_tiles(a.double() - b.double()) / _tiles(ra) / (4 * TOL)).max().item()
    print("permute true against false, 2048 x 1024: worst tile %.3f of 4 TOL; bit-identical: %s" % (ratio, torch.equal(a, b)))
    assert ratio <= 1.0, ratio
