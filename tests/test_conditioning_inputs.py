"""CPU: the inputs of tests/conditioning_inputs.py are what they claim to be, and the bounds test_gpu_conditioning.py holds
the kernels to are attainable by the reference arithmetic alone: the fp32-faithful oracle against the fp64 oracle, per
column, on every family at the shapes the GPU module uses.

Measured with these constructions (maximum over the columns of |phi32[:, c] - phi64[:, c]| / |phi64[:, c]|, shapes
150 x 37 / 700 x 300 / 1024 x 256): at most 1.0e-6 for graded, zero_const, spike and for far without the displaced row.
Asserted: 2e-6 -- twice that, so that another BLAS does not trip it; it is a property of the inputs, a factor of five
inside the 1e-5 the kernels are held to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402

SHAPES = [(150, 37), (700, 300), (1024, 256)]
ORACLE_BOUND = 2e-6


@pytest.mark.parametrize("n,d", SHAPES + [(1536, 130)])
def test_generators_are_seeded_fp32_exact_and_as_described(n, d):
    for family in ci.FAMILIES + ("offset",):
        T, G = ci.make(family, n, d, 3)
        T2, G2 = ci.make(family, n, d, 3)
        assert np.array_equal(T, T2) and np.array_equal(G, G2), family
        assert T.shape == (n, d) and T.dtype == np.float64 and np.isfinite(T).all() and np.isfinite(G).all()
        assert np.array_equal(ci.f32(T), T) and np.array_equal(ci.f32(G), G), family
        assert not np.array_equal(ci.make(family, n, d, 4)[0], T)
    T, G, e, f = ci.graded(n, d, 3, with_exponents=True)
    assert ci.neighbours_differ(e) and ci.neighbours_differ(f) and ci.blocks_differ(e) and ci.blocks_differ(f)
    assert sorted(e) == sorted(np.arange(d) % 41 - 20) and sorted(f) == sorted(np.arange(d) % 9 - 4)
    for c in range(16, d, 16):                  # either side of every column-block edge
        assert e[c - 1] != e[c] and f[c - 1] != f[c]
    # the scale exponent the split path derives from a column maximum really varies from column to column
    eg = np.floor(np.log2(np.abs(G).max(0))).astype(int)
    et = np.floor(np.log2(np.abs(T).max(0))).astype(int)
    assert len(set(eg)) >= min(d, 41) // 2 and len(set(et)) >= 5
    T, G = ci.zero_const(n, d, 3)
    assert not G[:, ci.zero_score_cols(d)].any() and not T[:, 1].any() and (T[:, 2] == 3.0).all()
    assert list(ci.constant_theta_cols(T)) == [1, 2]
    T, G = ci.spike(n, d, 3)
    assert G[7, 3] == 1e6 and G[11, d - 2] == 1.0 and np.abs(np.delete(G[:, d - 2], 11)).max() < 1e-5
    T0, G0 = ci.make("graded", n, d, 3)
    T2, G2, b = ci.pow2(T0, G0, -7, 3)
    assert np.array_equal(T2, T0 * 2.0 ** -7) and np.array_equal(G2, G0 * 2.0 ** b)
    assert b.min() >= -40 and b.max() <= 40 and ci.neighbours_differ(b)
    assert np.array_equal(np.frexp(T2)[0], np.frexp(T0)[0]) and np.array_equal(np.frexp(G2)[0], np.frexp(G0)[0])


def test_round_bf16_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415926, 0.0, 1e-30])
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 0.0, 0.0])
    got = ci.round_bf16(x)
    assert np.array_equal(got[:6], want[:6])
    assert abs(got[6] - 1e-30) <= 2.0 ** -9 * 1e-30
    import torch
    r = np.random.default_rng(0).normal(size=4096) * 10.0 ** np.random.default_rng(1).integers(-20, 20, size=4096)
    assert np.array_equal(ci.round_bf16(r), torch.tensor(r, dtype=torch.float32).bfloat16().double().numpy())


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("family", ci.FAMILIES)
def test_fp32_oracle_meets_the_per_column_bound(family, n, d):
    T, G = ci.make(family, n, d, 0)
    ref = orc.svgd_step(T, G, orc.AdagradState(), np.float64)
    o32 = orc.svgd_step(T, G, orc.AdagradState(), np.float32)
    skip = (ci.FAR_ROW,) if family.startswith("far") else ()
    e_phi, live = ci.column_errors(o32["phi"], ref["phi"], skip)
    const = ci.constant_theta_cols(T)
    e_dk, live_dk = ci.column_errors(np.delete(o32["dK"], const, axis=1), np.delete(ref["dK"], const, axis=1), skip)
    print("%s %dx%d: fp32 oracle vs fp64, worst column: phi %.2e  dK %.2e" % (family, n, d, e_phi.max(), e_dk.max()))
    assert live.all() and live_dk.all()
    assert e_phi.max() <= ORACLE_BOUND, (family, e_phi.max(), int(e_phi.argmax()))
    assert e_dk.max() <= ORACLE_BOUND, (family, e_dk.max(), int(e_dk.argmax()))
    assert abs(float(o32["h2"]) - ref["h2"]) <= 4e-6 * ref["h2"]
    if skip:    # the displaced particle sees nobody: its kernel row is its own diagonal entry
        K = ref["K"][ci.FAR_ROW]
        assert np.delete(K, ci.FAR_ROW).max() < 2.0 ** -149 and abs(K[ci.FAR_ROW] - 1.0) < 1e-9
        row = o32["phi"][ci.FAR_ROW]
        d55 = float(o32["D"][ci.FAR_ROW, ci.FAR_ROW])
        own = np.exp(-d55 / (2.0 * float(o32["h2"]))) * G[ci.FAR_ROW] / n
        print("   row %d: D_55 = %g (fp32 oracle), row error vs fp64 %.2e, vs its own diagonal %.2e" %
              (ci.FAR_ROW, d55, ci.frobenius_error(row, ref["phi"][ci.FAR_ROW]), ci.frobenius_error(row, own)))
        assert ci.frobenius_error(row, own) <= 1e-5


@pytest.mark.parametrize("n,d", SHAPES)
def test_offset_cluster_is_the_cancellation_case(n, d):
    """the fp32 oracle itself is two orders of magnitude outside 1e-5 here: why the GPU test of this family compares
    with 5 x this error and not with 1e-5"""
    T, G = ci.offset(n, d, 0)
    ref = orc.svgd_step(T, G, orc.AdagradState(), np.float64)
    o32 = orc.svgd_step(T, G, orc.AdagradState(), np.float32)
    e = ci.frobenius_error(o32["phi"], ref["phi"])
    print("offset %dx%d: fp32 oracle vs fp64, Frobenius %.2e" % (n, d, e))
    assert 1e-5 < e < 1e-2
