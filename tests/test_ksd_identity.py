"""CPU: the per-element identity behind STEIN_FLAG_KSD (include/steinhip.h) and the flag's host-side ABI.

The library sums the kernelized Stein discrepancy over the n*d elements of quantities its finish pass already holds
(K.G, K.theta, rowsum(K)) instead of over the n^2 pairs; these tests pin that identity in fp64 (tests/ksd_ref.py)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksd_ref as R  # noqa: E402

from stein_amd import _lib  # noqa: E402


def _particles(n, d, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    X = torch.tensor(rng.normal(size=(n, d)) + shift)
    G = torch.tensor(rng.normal(size=(n, d)))
    return X, G


@pytest.mark.parametrize("n,d", [(2, 1), (7, 3), (40, 5), (64, 17)])
def test_elementwise_equals_pairwise(n, d):
    X, G = _particles(n, d, seed=n * 31 + d)
    h2 = R.median_h2(X)
    U = R.pairwise_u(X, G, h2)
    S, S_diag = R.elementwise_sums(X, G, h2)
    assert S == pytest.approx(float(U.sum()), rel=1e-10, abs=1e-10 * float(U.abs().sum()))
    assert S_diag == pytest.approx(float(U.diagonal().sum()), rel=1e-12)
    v = float(U.sum()) / n ** 2
    u = float(U.sum() - U.diagonal().sum()) / (n * (n - 1))
    scale = float(U.abs().sum())
    assert R.statistic(S, S_diag, n, "v") == pytest.approx(v, abs=1e-10 * scale / n ** 2)
    assert R.statistic(S, S_diag, n, "u") == pytest.approx(u, abs=1e-10 * scale / (n * (n - 1)))
    Sp, Sdp, _ = R.pairwise_sums(X, G, h2, block=5)       # the blocked pair sum the GPU tests use
    assert Sp == pytest.approx(float(U.sum()), abs=1e-10 * scale) and Sdp == pytest.approx(S_diag, rel=1e-12)


def test_u_is_the_stein_kernel_of_autograd():
    """u_ij = g_i.g_j k + g_i.grad_y k + g_j.grad_x k + tr(grad_x grad_y k) for k(x, y) = exp(-|x - y|^2 / 2 h2)."""
    n, d = 5, 3
    X, G = _particles(n, d, seed=11)
    h2 = R.median_h2(X)
    U = R.pairwise_u(X, G, h2)

    def k(x, y):
        return torch.exp(-((x - y) ** 2).sum() / (2.0 * h2))
    for i in range(n):
        for j in range(n):
            x = X[i].clone().requires_grad_(True)
            y = X[j].clone().requires_grad_(True)
            kv = k(x, y)
            gx, gy = torch.autograd.grad(kv, (x, y), create_graph=True)
            tr = sum(torch.autograd.grad(gx[c], y, retain_graph=True)[0][c] for c in range(d))
            ref = (G[i] @ G[j]) * kv + G[i] @ gy + G[j] @ gx + tr
            assert float(U[i, j]) == pytest.approx(float(ref), rel=1e-10, abs=1e-12)


@pytest.mark.parametrize("blocks", [2, 8])
def test_row_block_shares_sum_to_the_total(blocks):
    n, d = 64, 6
    X, G = _particles(n, d, seed=blocks)
    h2 = R.median_h2(X)
    S, S_diag = R.elementwise_sums(X, G, h2)
    step = n // blocks
    parts = [R.elementwise_sums(X, G, h2, rows=slice(b * step, (b + 1) * step)) for b in range(blocks)]
    assert sum(p[0] for p in parts) == pytest.approx(S, rel=1e-11)
    assert sum(p[1] for p in parts) == pytest.approx(S_diag, rel=1e-12)
    # a share is not the block's rows of the pair sum: only the total is the statistic
    U = R.pairwise_u(X, G, h2)
    assert abs(parts[0][0] - float(U[:step].sum())) > 1e-6 * float(U.abs().sum())


def test_statistic_is_translation_invariant():
    n, d = 50, 4
    X, G = _particles(n, d, seed=5)
    h2 = R.median_h2(X)
    S, S_diag = R.elementwise_sums(X, G, h2)
    for shift in (3.0, -20.0):
        S2, S_diag2 = R.elementwise_sums(X + shift, G, h2)
        assert S2 == pytest.approx(S, rel=1e-8) and S_diag2 == pytest.approx(S_diag, rel=1e-12)
        assert R.median_h2(X + shift) == pytest.approx(h2, rel=1e-9)


def test_unknown_statistic_is_refused():
    with pytest.raises(ValueError):
        R.statistic(1.0, 0.5, 10, "w")


def test_workspace_with_the_flag():
    """Without STEIN_FLAG_KSD the workspace is the parent's, byte for byte (sizes recorded from it); with the flag SQPART
    holds three partial sets and only the sections behind it move."""
    recorded = {(100, 100, 10, _lib.F32, 0): 173568, (1000, 1000, 37, _lib.F32, _lib.FLAG_X3): 24818176,
                (4096, 4096, 128, _lib.BF16, _lib.FLAG_X3): 127753984,
                (16384, 16384, 256, _lib.F32, _lib.FLAG_X3): 1200536320,
                (2048, 16384, 256, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_TILED): 261008128}
    for (nl, n, d, dt, fl), size in recorded.items():
        total, offs, extra = _lib.workspace_layout(nl, n, d, dt, fl)
        assert total == size
        tk, ok, ek = _lib.workspace_layout(nl, n, d, dt, fl | _lib.FLAG_KSD)
        assert tk >= total and ek == extra
        assert ok[:_lib.WS_SQPART + 1] == offs[:_lib.WS_SQPART + 1]
        small = math.ceil(d / 32)
        assert ok[_lib.WS_SPEC] - ok[_lib.WS_SQPART] >= 3 * 8 * max(extra[_lib.WSX_SQ_BLOCKS], small)


def test_finish_calls_without_a_score_refuse_the_flag():
    lib = _lib.load()
    fake = (ctypes.c_ubyte * 64)()
    f = ctypes.cast(fake, ctypes.c_void_p)
    tot, _, extra = _lib.workspace_layout(256, 256, 8, _lib.F32, _lib.FLAG_KSD)
    assert lib.stein_contract_finish(f, 256, 8, 0, 256, _lib.F32, f, f, f, None, f, tot, _lib.FLAG_KSD, None) == _lib.E_BADARG
    assert b"STEIN_FLAG_KSD" in lib.stein_last_error() and b"score" in lib.stein_last_error()
    assert lib.stein_kernel_contract(f, extra[_lib.WSX_LD_DIST], f, f, 256, 8, 0, 256, _lib.F32, f, f, f, None, None, f, tot,
                                     _lib.FLAG_KSD, None) == _lib.E_BADARG
    assert b"STEIN_FLAG_KSD" in lib.stein_last_error()
    # the rank segments accept it (argument checks only: a NULL score is refused before any launch)
    assert lib.stein_rank_finish(f, None, 256, 8, 0, 256, _lib.F32, f, f, f, None, f, tot, _lib.FLAG_KSD, None) == _lib.E_BADARG
    assert b"NULL" in lib.stein_last_error()


def test_standalone_call_checks_its_arguments_on_the_host():
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    with pytest.raises(ValueError, match="device"):
        ksd(torch.zeros(8, 3), torch.zeros(8, 3))
    with pytest.raises(ValueError, match="torch tensor"):
        ksd(np.zeros((8, 3)), np.zeros((8, 3)))
