"""GPU: the output tail of the contraction (k_phi_x3fs, stein_x3.hip).  The matrix waves hand their scaled partial sums over
through an LDS image of the workgroup's 128 x 256 tile and all twelve waves store it row-major in whole lines.  Every
store branch at the smallest shapes that reach it:

  folded (fold=True, small=False, as test_gpu_fold_prepare.py forces it)
    256 x 256     aligned, two column blocks: one workgroup per row tile, both halves store
    700 x 300     ragged rows and columns; three blocks: the last workgroup's second half stores nothing
    1088 x 192    two blocks, the second ragged at d (one block's columns past d are never written)
    192 x 130     with dK_out: the theta-half workgroups behind W's
    320 x 257     d % 4 != 0: the 4-byte form of the store loop
  unfolded (fold=False, small=False)   1536 x 257 (4-byte form, block pairs of [G | theta]) and 1000 x 130
  bf16 (one plane: the image holds 128 columns at a time, two passes)   512 x 48

Tolerances are the neighbours': phi per column at test_gpu_conditioning.TOL through its _check_columns and |phi|^2 at 2e-5
relative, as test_gpu_fold.py::test_parity_normal_inputs, on every shape.  phi of the bf16 case cannot be held per column at
1e-5 (K is rounded to bf16, 2^-9 per entry): it takes the project's bf16 bound, 4e-3 relative Frobenius error against the
fp64 oracle on the same bf16 inputs (derivation: test_gpu_x3.py).
The 4-byte-offset inputs are test_gpu_fold_prepare._offset_by_4_bytes's; the helper places fp32 tensors, so the bf16 case
does not take that part.  Run with -s to see the figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import test_gpu_conditioning as tc  # noqa: E402
import test_gpu_fold_prepare as tp  # noqa: E402
import test_gpu_x3 as tx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_BF16 = 4e-3
# (form, n, d, with dK_out)
CASES = [("fold", 256, 256, False), ("fold", 700, 300, False), ("fold", 1088, 192, False), ("fold", 192, 130, True),
         ("fold", 320, 257, False), ("unfolded", 1536, 257, False), ("unfolded", 1000, 130, False), ("bf16", 512, 48, False)]


def _engine(form, n, d, cuda):
    if form == "bf16":
        eng = SvgdEngine(n, d, device=cuda, small=False, dtype=torch.bfloat16)
        assert not eng.fold
    else:
        eng = SvgdEngine(n, d, device=cuda, fold=form == "fold", small=False)
        assert eng.fold == (form == "fold")
    return eng


def _call(eng, T, G, dk):
    dK = torch.full((eng.n, eng.d), float("nan"), device=T.device) if dk else None
    phi = eng.compute_phi(T, G, dK_out=dK).clone()
    torch.cuda.synchronize()
    out = dict(phi=phi, h2=eng.h2.clone(), sqnorm=eng.sqnorm.clone())
    if dk:
        out["dK"] = dK
    return out


def _same(tag, got, want):
    for key in want:
        assert torch.equal(got[key], want[key]), (tag, key, int((got[key] != want[key]).sum()))


@pytest.mark.parametrize("form,n,d,dk", CASES, ids=["%s-%dx%d%s" % (f, n, d, "-dK" if k else "") for f, n, d, k in CASES])
def test_output_tail(cuda, form, n, d, dk):
    tag = "tail %s %dx%d" % (form, n, d)
    T64, G64 = tx._inputs(n, d)
    dtype = torch.bfloat16 if form == "bf16" else torch.float32
    T, G = tc._dev(T64, cuda, dtype), tc._dev(G64, cuda, dtype)
    T64, G64 = T.double().cpu().numpy(), G.double().cpu().numpy()      # what the device holds, exactly
    ref = orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)

    # 1. three consecutive calls (radix select first, the window later): parity with the oracle, and the same bits
    eng = _engine(form, n, d, cuda)
    calls = [_call(eng, T, G, dk) for _ in range(3)]
    for k, got in enumerate(calls):
        phi, sq = tc._np(got["phi"]), float(got["sqnorm"].item())
        assert np.isfinite(phi).all(), tag
        if form == "bf16":
            err = np.linalg.norm(phi - ref["phi"]) / np.linalg.norm(ref["phi"])
            print("%s call %d: phi Frobenius %.2e, |phi|^2 %.2e" % (tag, k, err, abs(sq - ref["sqnorm"]) / ref["sqnorm"]))
            assert err <= TOL_BF16, (tag, err)
            assert abs(sq - ref["sqnorm"]) <= 2e-5 * ref["sqnorm"], tag
        else:
            tc._check_columns("%s call %d" % (tag, k), phi, ref["phi"], T64, "phi")
            print("%s call %d: |phi|^2 %.2e" % (tag, k, abs(sq - ref["sqnorm"]) / ref["sqnorm"]))
            assert abs(sq - ref["sqnorm"]) <= 2e-5 * ref["sqnorm"], tag
            if dk:
                tc._check_columns("%s call %d" % (tag, k), tc._np(got["dK"]), ref["dK"], T64, "dK",
                                  scale_terms=ref["K"].sum(1)[:, None] / ref["h2"])
        _same("%s call %d against call 0" % (tag, k), got, calls[0])

    # 2. nothing outside the valid region is written, nothing inside it is left over: 0xFF all over the workspace, then the
    #    bits of a fresh engine
    fresh = _call(_engine(form, n, d, cuda), T, G, dk)
    _same(tag + " fresh engine", fresh, calls[0])
    eng.ws.fill_(0xFF)
    _same(tag + " after 0xFF", _call(eng, T, G, dk), fresh)

    # 3. the same values 4 bytes into a larger buffer
    if form != "bf16":
        T4, G4 = tp._offset_by_4_bytes(T), tp._offset_by_4_bytes(G)
        _same(tag + " inputs offset by 4 bytes", _call(_engine(form, n, d, cuda), T4, G4, dk), fresh)
