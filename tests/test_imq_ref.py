"""CPU: the closed forms of tests/imq_ref.py -- what stein_svgd_phi_imq{,_ksd} evaluates (include/steinhip.h) -- against
torch.autograd on the kernel itself, the row-sum form against the pair sum, and the fp32 model of the library's arithmetic
(rowsum_sums(round32=True)) at the GPU tests' parity shapes, inside the bounds those tests use.

The model's figures, printed with -s: over the fifteen inputs x {0.25, 1, 4} median bandwidths it reaches at most 0.18 of
the phi allowance (graded 700 x 300, x 4) and 3.4e-8 of the statistic's scale (2 x 1)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import imq_ref as R  # noqa: E402

TOL, TOL_F32 = 1e-5, 1e-6     # test_gpu_conditioning.TOL and test_gpu_ksd.TOL_F32 (GPU modules: not imported here)
PARITY_SHAPES = [(2, 1), (20, 3), (128, 128), (129, 129), (150, 37), (257, 256), (300, 260), (384, 513), (1000, 40),
                 (1536, 130), (4096, 256)]
GRADED_SHAPES = [(150, 37), (700, 300), (1024, 256), (1536, 130)]     # test_gpu_conditioning.SHAPES


def ksd_inputs(n, d, seed):
    """test_gpu_ksd._inputs on the CPU"""
    rng = np.random.default_rng(seed)
    T = torch.tensor(rng.normal(size=(n, d)), dtype=torch.float32)
    G = torch.tensor(-rng.normal(size=(n, d)) * 0.5, dtype=torch.float32) - 0.5 * T
    return T, G


def _small(n, d, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=gen, dtype=torch.float64), torch.randn(n, d, generator=gen, dtype=torch.float64)


def _k(x, y, h2):
    return (1.0 + ((x - y) ** 2).sum() / (2.0 * h2)) ** -0.5


SMALL = [(2, 1, 0.7), (5, 3, 1.9), (7, 3, 0.4), (8, 4, 6.5)]


@pytest.mark.parametrize("n,d,h2", SMALL)
def test_closed_forms_against_autograd(n, d, h2):
    X, G = _small(n, d, 10 * n + d)
    c2 = 2.0 * h2
    D = R.sq_dists(X)
    k, k3, k5 = R.kernel(D, h2)
    phi = torch.zeros(n, d, dtype=torch.float64)
    U = torch.zeros(n, n, dtype=torch.float64)
    for i in range(n):
        for j in range(n):
            x = X[i].clone().requires_grad_(True)
            y = X[j].clone().requires_grad_(True)
            kij = _k(x, y, h2)
            gx, gy = torch.autograd.grad(kij, (x, y), create_graph=True)
            # the gradient: grad_{theta_j} k(theta_j, theta_i) = k3 (theta_i - theta_j) / c2
            assert torch.allclose(gy, k3[i, j] * (X[i] - X[j]) / c2, rtol=1e-13, atol=1e-15)
            # the trace term: sum_c d^2 k / dx_c dy_c = d k3 / c2 - 3 k5 D / c2^2
            tr = sum(torch.autograd.grad(gx[c], y, retain_graph=True)[0][c] for c in range(d))
            assert abs(float(tr) - float(d * k3[i, j] / c2 - 3.0 * k5[i, j] * D[i, j] / c2 ** 2)) <= 1e-13
            phi[i] += (kij.detach() * G[j] + gy.detach()) / n
            U[i, j] = kij.detach() * (G[i] @ G[j]) + G[i] @ gy.detach() + G[j] @ gx.detach() + tr.detach()
    assert torch.allclose(R.pair_phi(X, G, h2), phi, rtol=1e-13, atol=1e-15)
    assert torch.allclose(R.pairwise_u(X, G, h2), U, rtol=1e-12, atol=1e-14)
    S, S_diag, scale = R.pairwise_sums(X, G, h2)
    assert abs(S - float(U.sum())) <= 1e-12 * scale
    assert abs(S_diag - float(U.diagonal().sum())) <= 1e-12 * scale
    assert scale >= abs(S)


@pytest.mark.parametrize("n,d", [(7, 3), (150, 37), (300, 260), (700, 300)])
def test_row_sum_form_equals_the_pair_sum(n, d):
    X, G = ksd_inputs(n, d, n + d)
    for mult in (0.25, 1.0, 4.0):
        h2 = R.median_h2(X) * mult
        S, S_diag, scale = R.pairwise_sums(X, G, h2, block=128)
        S2, S_diag2, phi, rs3 = R.rowsum_sums(X, G, h2, block=100)
        assert abs(S2 - S) <= 1e-12 * scale and S_diag2 == S_diag
        assert abs(S_diag - float(((G.double() ** 2).sum(1) + d / (2.0 * h2)).sum())) <= 1e-12 * S_diag
        if n <= 300:
            ref = R.pair_phi(X, G, h2)
            assert float((phi - ref).norm() / ref.norm()) <= 1e-12
            assert abs(S - float(R.pairwise_u(X, G, h2).sum())) <= 1e-12 * scale
        assert torch.allclose(rs3, R.kernel(R.sq_dists(X), h2)[1].sum(1), rtol=1e-13)


def test_one_particle_and_coincident_particles():
    X, G = _small(1, 3, 5)
    S, S_diag, scale = R.pairwise_sums(X, G, 2.0)
    assert S == S_diag and abs(S - (float((G * G).sum()) + 3 / 4.0)) <= 1e-14 * S     # u_11 = |g|^2 + d / c2
    X2 = X.repeat(4, 1)
    G2 = G.repeat(4, 1)
    assert float(R.pair_phi(X2, G2, 2.0).sub(G).abs().max()) <= 1e-15                  # every k = 1, every difference 0


@functools.lru_cache(maxsize=None)
def _case(family, n, d):
    if family == "normal":
        return ksd_inputs(n, d, n + d)
    T64, G64 = ci.make("graded", n, d, 0)
    return torch.tensor(T64, dtype=torch.float32), torch.tensor(G64, dtype=torch.float32)


MODEL = [("normal", n, d) for n, d in PARITY_SHAPES] + [("graded", n, d) for n, d in GRADED_SHAPES]


@pytest.mark.parametrize("family,n,d", MODEL, ids=["%s-%dx%d" % c for c in MODEL])
def test_fp32_model_stays_inside_the_gpu_bounds(family, n, d):
    """What fp32 sums, an fp32 rsq and the two-term fp16 split at 2^14 cost by themselves: well inside TOL for phi and half
    of TOL_F32 for the statistic at every parity case, so the GPU tests use those bounds as they are."""
    T, G = _case(family, n, d)
    med = R.median_h2(T)
    for mult in (0.25, 1.0, 4.0):
        h2 = float(np.float32(med * mult))
        S, S_diag, scale = R.pairwise_sums(T, G, h2)
        _, _, phi, rs3 = R.rowsum_sums(T, G, h2)
        S32, S_diag32, phi32, _ = R.rowsum_sums(T, G, h2, round32=True)
        ratio = float(((phi32 - phi).norm(dim=0) / R.phi_allowance(phi, rs3, T, h2, TOL)).max())
        e = abs(S32 - S) / scale
        print("imq model %s %dx%d h2 x %g: phi error / allowance %.3f, S error / scale %.2e" % (family, n, d, mult, ratio, e))
        assert ratio <= 0.5, (mult, ratio)
        assert e <= 0.5 * TOL_F32, (mult, e)
        assert S_diag32 == S_diag
