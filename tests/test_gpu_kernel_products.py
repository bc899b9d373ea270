"""GPU: the Stein-kernel products (stein_ksd_matmul, include/steinhip.h; stein_amd.utilities.stein_kernel_products).

Every element of out = V U is checked against the fp64 product of tests/weights_ref.py within the allowance its docstring
derives from k_ksd_boot's arithmetic, on a NaN-filled workspace with guard bytes behind `out`; a repeat, another workspace
content and every forced j split bit for bit or within the allowance; a row of ones against the quadratic form of
ksd_quadratic_forms.  The shapes are the smallest at which the product tail can go wrong: n below, at and past one and two
row tiles (2, 127, 129, 257, 300: ragged 16-byte stores at the last rows), d in one and several k tiles (1, 31, 33, 130),
reps in one live 128-block, the second block and two column groups (1, 33, 129, 257), and j splits 1, 2, 3 and more than the
j tiles (ragged and dropped tails).  Measured on the MI355X (largest error over allowance, printed): DESIGN.md section 6i.
"""
import functools

import numpy as np
import pytest
import torch

import boot_ref as B
import weights_ref as R
from stein_amd import _lib
from stein_amd.engine import HipStages
from stein_amd.utilities import ksd_quadratic_forms, stein_kernel_products

pytestmark = pytest.mark.gpu
KERNEL_IDS = {"rbf": _lib.KERNEL_RBF, "imq": _lib.KERNEL_IMQ}
GUARD = 64
# every n, d and reps of the list above at least once, under both kernels
SHAPES = [(2, 1, 1), (127, 31, 33), (129, 33, 129), (257, 130, 257), (300, 33, 33), (300, 1, 129), (257, 31, 1), (129, 130, 33)]
SPLITS = (1, 2, 3, 1000)


@functools.lru_cache(maxsize=None)
def reference(n, d, reps, kernel):
    """(X, G, h2, V, out, allow), computed once and shared -- read-only.  V: row 0 all ones, row 1 (if any) mixed signs with a
    third of its entries zero, the rest general values of mixed sign and magnitude"""
    rng = np.random.default_rng(5000 + 7 * n + d)
    X = (rng.standard_normal((n, d)) + 0.2).astype(np.float32)
    G = (-X + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    V = (rng.standard_normal((reps, n)) * np.exp(rng.standard_normal((reps, 1)))).astype(np.float32)
    V[0] = 1.0
    if reps > 1:
        V[1] = rng.integers(-1, 2, n).astype(np.float32)
    h2 = B.median_h2(X)
    out, allow = R.Model(X, G, h2, kernel).products(V)
    return X, G, h2, V, out, allow


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _products(T, G, h2, kernel, V, jsplit=0, fill=float("nan")):
    """the C call on device tensors, on a workspace filled with `fill`, `out` NaN with a guard behind it -> out as NumPy"""
    n, d = T.shape
    reps = V.shape[0]
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=T.device)
    buf = torch.full((reps * n + GUARD,), float("nan"), dtype=torch.float32, device=T.device)
    buf[reps * n:] = -12345.0
    _lib.debug_boot_jsplit(jsplit)
    try:
        ws = torch.full((_lib.ksd_matmul_workspace_bytes(n, d, reps) // 4,), fill, dtype=torch.float32, device=T.device)
        HipStages().ksd_matmul(T, G, n, d, h2_t, KERNEL_IDS[kernel], V, reps, buf, ws.view(torch.uint8))
    finally:
        _lib.debug_boot_jsplit(0)
    torch.cuda.synchronize()
    assert (buf[reps * n:] == -12345.0).all(), "the guard behind out was written"
    return buf[:reps * n].view(reps, n).cpu().numpy()


def _check(tag, got, want, allow):
    ratio = np.abs(got - want) / allow
    print("products %s: largest |err| / allowance %.3g  (allowance / largest |out| %.3g)" %
          (tag, ratio.max(), allow.max() / np.abs(want).max()))
    assert np.isfinite(got).all(), tag
    assert (ratio <= 1.0).all(), (tag, np.argwhere(ratio > 1.0)[:8], ratio.max())


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("n,d,reps", SHAPES)
def test_every_element_within_its_allowance(cuda, n, d, reps, kernel):
    X, G, h2, V, want, allow = reference(n, d, reps, kernel)
    T, S, Vd = _dev(cuda, X, G, V)
    tag = "%dx%d r%d %s" % (n, d, reps, kernel)
    out = _products(T, S, h2, kernel, Vd)
    _check(tag, out, want, allow)
    assert np.array_equal(out, _products(T, S, h2, kernel, Vd))                  # on repeat: the same bits
    assert np.array_equal(out, _products(T, S, h2, kernel, Vd, fill=0.0))        # whatever the workspace held
    for k in SPLITS:                                                             # every j split, ragged and dropped tails
        ok = _products(T, S, h2, kernel, Vd, jsplit=k)
        _check("%s jsplit %d" % (tag, k), ok, want, allow)
        assert np.array_equal(ok, _products(T, S, h2, kernel, Vd, jsplit=k, fill=1e30)), k


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("n,d,reps", [(129, 33, 129), (300, 33, 33), (257, 130, 257)])
def test_a_row_of_ones_agrees_with_the_quadratic_form(cuda, n, d, reps, kernel):
    """sum_i out[0, i] = sum_ij u_p(x_i, x_j) = Q of the all-ones row, which ksd_quadratic_forms computes with the other
    tail of the same kernel: within the sum of the products' allowances plus that form's own (boot_ref)"""
    X, G, h2, V, want, allow = reference(n, d, reps, kernel)
    T, S, Vd = _dev(cuda, X, G, V)
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=cuda)
    out = stein_kernel_products(T, S, Vd, bandwidth=h2_t, kernel=kernel)
    assert out.dtype == torch.float32 and out.shape == (reps, n) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), _products(T, S, h2, kernel, Vd))    # the utility is the C call
    q, _ = ksd_quadratic_forms(T, S, Vd[:1].contiguous(), bandwidth=h2_t, kernel=kernel)
    f = B.quadratic_forms(X, G, h2, kernel, V[:1])
    err, tol = abs(float(out[0].double().sum()) - float(q[0])), float(allow[0].sum()) + float(f.allow[0])
    print("products %dx%d r%d %s: |sum_i out[0, i] - Q_0| / tolerance %.3g" % (n, d, reps, kernel, err / tol))
    assert err <= tol


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_misaligned_bases(cuda, kernel):
    """theta, score, V and out 4 bytes past a 16-byte boundary (d % 4 == 0: the split's 16-byte loads must not be taken)"""
    n, d, reps = 150, 8, 5
    X, G, h2, V, want, allow = reference(n, d, reps, kernel)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device=cuda)
        buf[1:] = torch.from_numpy(a.reshape(-1)).to(cuda)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4
        return v
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=cuda)
    ws = torch.full((_lib.ksd_matmul_workspace_bytes(n, d, reps) // 4,), float("nan"), dtype=torch.float32, device=cuda)
    buf = torch.full((reps * n + 1 + GUARD,), float("nan"), dtype=torch.float32, device=cuda)
    buf[reps * n + 1:] = -12345.0
    out = buf[1:reps * n + 1].view(reps, n)
    assert out.data_ptr() % 16 == 4
    HipStages().ksd_matmul(shifted(X), shifted(G), n, d, h2_t, KERNEL_IDS[kernel], shifted(V), reps, out, ws.view(torch.uint8))
    torch.cuda.synchronize()
    assert (buf[reps * n + 1:] == -12345.0).all() and bool(torch.isnan(buf[0]))
    _check("150x8 r5 misaligned %s" % kernel, out.cpu().numpy(), want, allow)
