"""GPU: the streaming SVGD step at a caller-given bandwidth (stein_svgd_phi_stream; SvgdEngine(h2=), SteinSampler(bandwidth=)).

No distance image and no median: W = G - theta / h2 is built first, every distance tile is exponentiated and contracted the
moment it is complete (stein_amd/csrc/stein_stream.hip).  The inputs and yardsticks are the other modules' (imported, not
restated); the fp64 reference for a given h2 is formed here, on the fp32 input values:

    K = exp(-D / (2 h2)),   phi = (K.G + (rowsum(K) theta - K.theta) / h2) / n

Bounds that are not imported:
  other bandwidths   per column TOL * (|ref_c| + |rowsum(K) * theta_c| / (h2 n)) (2-norms): the folded form carries two
                     terms of size rowsum(K) |theta| / h2 that cancel in phi, each rounded at the project's relative
                     tolerance; derived from the form, not measured.  The worst observed ratio is recorded in DESIGN.md.
  against the fold   the streaming error against fp64 is held to twice the stored-D folded path's own on the same rows and
                     in any case to 1e-5: test_gpu_fold.py's rule for folded against unfolded.
Run with -s to see every figure."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402
import test_gpu_conditioning as tc  # noqa: E402
import test_gpu_fold as tf  # noqa: E402
import test_gpu_x3 as tx  # noqa: E402
from oracle import svgd_oracle as orc  # noqa: E402
from stein_amd import _lib  # noqa: E402
from stein_amd.engine import SvgdEngine  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = tc.TOL
_check_columns, _dev, _np = tc._check_columns, tc._dev, tc._np


# ---------------------------------------------------------------------------------------------------------------
# references (computed once per input, shared)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _normal_case(n, d):
    T64, G64 = tx._inputs(n, d)
    T64, G64 = ci.f32(T64), ci.f32(G64)
    return T64, G64, orc.svgd_step(T64, G64, orc.AdagradState(), np.float64)


def _inputs_of(family, n, d):
    """(theta, score, the fp64 oracle's step) -- `normal`: test_gpu_x3's inputs, else a family of conditioning_inputs"""
    return _normal_case(n, d) if family == "normal" else tc._case(family, n, d)


def _h2_f32(x):
    """the value a float32 tensor holds, as a Python float"""
    return float(np.float32(x))


def _phi_at(T64, G64, D, h2):
    """(phi, rowsum(K)) in fp64 at the given h2, from the oracle's fp64 distances of the fp32 inputs"""
    n = T64.shape[0]
    K = np.exp(-D / (2.0 * h2))
    rs = K.sum(axis=1)
    return (K @ G64 + (rs[:, None] * T64 - K @ T64) / h2) / n, rs


@functools.lru_cache(maxsize=None)
def _reference(family, n, d, mult=1.0):
    T64, G64, ref = _inputs_of(family, n, d)
    h2 = _h2_f32(ref["h2"]) * mult          # (multipliers are powers of two: still an fp32 value)
    phi, rs = _phi_at(T64, G64, ref["D"], h2)
    return T64, G64, h2, phi, rs


def _stream_engine(n, d, cuda, h2):
    eng = SvgdEngine(n, d, device=cuda, h2=h2)
    assert eng.streaming and (eng.row_tiles, eng.col_groups) == ((n + 127) // 128, (d + 255) // 256)
    return eng


def _check_parity(tag, eng, T64, G64, phi_ref, cuda, skip=(), sqnorm=True):
    phi = eng.compute_phi(_dev(T64, cuda), _dev(G64, cuda))
    torch.cuda.synchronize()
    worst = _check_columns(tag, _np(phi), phi_ref, T64, "phi", skip)
    sq, sq_ref = eng.sqnorm.item(), float(np.sum(phi_ref * phi_ref))
    assert np.isfinite(sq), tag
    if sqnorm:
        print("%s: |phi|^2 %.9e (fp64 %.9e)" % (tag, sq, sq_ref))
        assert abs(sq - sq_ref) <= 2e-5 * sq_ref, (tag, sq, sq_ref)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# 1. parity at the heuristic's own bandwidth
# ---------------------------------------------------------------------------------------------------------------
NORMAL_SHAPES = sorted(set(tx.SHAPES) | set(tc.SHAPES) | {(129, 257), (20, 1)})


@pytest.mark.parametrize("n,d", NORMAL_SHAPES)
def test_parity_normal_inputs(cuda, n, d):
    T64, G64, h2, phi_ref, _ = _reference("normal", n, d)
    eng = _stream_engine(n, d, cuda, h2)
    tag = "stream normal %dx%d (plan %s)" % (n, d, (eng.row_tiles, eng.col_groups, eng.jsplit))
    for call in range(2):
        _check_parity(tag, eng, T64, G64, phi_ref, cuda)
    assert eng.h2.item() == h2


PARITY = [(f, n, d) for f in ci.FAMILIES for (n, d) in tc.SHAPES]


@pytest.mark.parametrize("family,n,d", PARITY, ids=["%s-%dx%d" % c for c in PARITY])
def test_parity_per_column(cuda, family, n, d):
    T64, G64, h2, phi_ref, _ = _reference(family, n, d)
    is_far = family.startswith("far")
    eng = _stream_engine(n, d, cuda, h2)
    # (with the displaced row |phi|^2 carries that row's K_55 = exp(-D_55 / 2 h2) of a D_55 that is rounding: skipped with
    # the row, as test_gpu_fold.py does)
    _check_parity("stream %s %dx%d" % (family, n, d), eng, T64, G64, phi_ref, cuda, (ci.FAR_ROW,) if is_far else (),
                  sqnorm=not is_far)


# ---------------------------------------------------------------------------------------------------------------
# 2. against the stored-D folded path, fed that path's own bandwidth tensor
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1024, 256), (1536, 130)])
def test_against_the_stored_folded_path(cuda, n, d):
    T64, G64, ref = _inputs_of("graded", n, d)
    T, G = _dev(T64, cuda), _dev(G64, cuda)
    stored = SvgdEngine(n, d, device=cuda, fold=True, small=False)
    assert stored.fold
    p_stored = _np(stored.compute_phi(T, G))
    eng = _stream_engine(n, d, cuda, stored.h2)
    assert eng.h2 is stored.h2
    p_stream = _np(eng.compute_phi(T, G))
    phi_ref, _ = _phi_at(T64, G64, ref["D"], float(stored.h2.item()))
    e_stream, e_stored = ci.frobenius_error(p_stream, phi_ref), ci.frobenius_error(p_stored, phi_ref)
    print("stream %dx%d against fp64 on all rows: streaming %.3e, stored-D folded %.3e" % (n, d, e_stream, e_stored))
    assert e_stream <= min(2.0 * e_stored, 1e-5), (e_stream, e_stored)
    assert abs(eng.sqnorm.item() - stored.sqnorm.item()) <= 2e-5 * stored.sqnorm.item()


# ---------------------------------------------------------------------------------------------------------------
# 3. other bandwidths
# ---------------------------------------------------------------------------------------------------------------
OTHER = [(f, n, d, m) for f in ("normal", "graded") for (n, d) in tc.SHAPES for m in (0.25, 4.0)]


@pytest.mark.parametrize("family,n,d,mult", OTHER, ids=["%s-%dx%d-x%g" % c for c in OTHER])
def test_other_bandwidths(cuda, family, n, d, mult):
    T64, G64, h2, phi_ref, rs = _reference(family, n, d, mult)
    eng = _stream_engine(n, d, cuda, h2)
    phi = _np(eng.compute_phi(_dev(T64, cuda), _dev(G64, cuda)))
    assert np.isfinite(phi).all()
    err = np.linalg.norm(phi - phi_ref, axis=0)
    allowed = TOL * (np.linalg.norm(phi_ref, axis=0) + np.linalg.norm(rs[:, None] * T64, axis=0) / (h2 * n))
    ratio = err / allowed
    print("stream %s %dx%d h2 x %g: worst column error / allowance %.3f (column %d); plain relative error %.2e" %
          (family, n, d, mult, ratio.max(), int(ratio.argmax()), ci.column_errors(phi, phi_ref)[0].max()))
    assert (err <= allowed).all(), (float(ratio.max()), int(ratio.argmax()))


# ---------------------------------------------------------------------------------------------------------------
# 4. the j split: every split passes parity and repeats itself to the bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(700, 300), (1536, 256)])
def test_every_j_split_is_right_and_deterministic(cuda, n, d):
    family = "normal" if (n, d) in tx.SHAPES else "graded"
    T64, G64, h2, phi_ref, _ = _reference(family, n, d)
    T, G = _dev(T64, cuda), _dev(G64, cuda)
    seen = {}
    try:
        for want in (1, 2, 3, 0):      # 0: the plan's own rule
            _lib.debug_stream_jsplit(want)
            eng = _stream_engine(n, d, cuda, h2)
            if want:
                assert eng.jsplit == want == _lib.stream_plan(n, d)[2]
            tag = "stream %dx%d jsplit %d" % (n, d, eng.jsplit)
            _check_parity(tag, eng, T64, G64, phi_ref, cuda)
            first, sq = eng.phi.clone(), eng.sqnorm.clone()
            for call in range(5):
                assert torch.equal(eng.compute_phi(T, G), first) and torch.equal(eng.sqnorm, sq), (tag, "repeat", call)
            seen[eng.jsplit] = first
    finally:
        _lib.debug_stream_jsplit(0)
    assert {1, 2, 3} <= set(seen)


# ---------------------------------------------------------------------------------------------------------------
# 5. the workspace carries nothing
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(150, 37), (1024, 256)])
def test_result_does_not_depend_on_what_the_workspace_held(cuda, n, d):
    T64, G64, h2, _, _ = _reference("graded", n, d)
    T, G = _dev(T64, cuda), _dev(G64, cuda)
    eng = _stream_engine(n, d, cuda, h2)
    eng.ws.zero_()
    want, sq = eng.compute_phi(T, G).clone(), eng.sqnorm.clone()
    assert torch.isfinite(want).all()
    gen = torch.Generator(device="cpu").manual_seed(n + d)
    for name in ("0xFF", "random"):
        if name == "0xFF":
            eng.ws.fill_(0xFF)
        else:
            eng.ws.copy_(torch.randint(0, 256, (eng.ws_bytes,), dtype=torch.uint8, generator=gen))
        eng.phi.fill_(float("nan"))
        eng.sqnorm.fill_(float("nan"))
        got = eng.compute_phi(T, G)
        assert torch.equal(got, want) and torch.equal(eng.sqnorm, sq), (n, d, name)


# ---------------------------------------------------------------------------------------------------------------
# 6. the bandwidth lives on the device
# ---------------------------------------------------------------------------------------------------------------
def test_bandwidth_tensor_is_read_on_the_device_every_call(cuda):
    n, d = 700, 300
    T64, G64, ref = _inputs_of("graded", n, d)
    T, G = _dev(T64, cuda), _dev(G64, cuda)
    base = _h2_f32(ref["h2"])
    values = [base, _h2_f32(base * 0.5), _h2_f32(base * 1.75)]
    on_device = torch.tensor(values, dtype=torch.float32, device=cuda)
    h2 = torch.empty(1, dtype=torch.float32, device=cuda)
    eng = _stream_engine(n, d, cuda, h2)
    got = []
    for k in range(3):                 # rewritten in place by device copies: nothing here waits for the GPU
        h2.copy_(on_device[k:k + 1])
        got.append(eng.compute_phi(T, G).clone())
    torch.cuda.synchronize()
    assert eng.h2 is h2
    for k, v in enumerate(values):
        phi_ref, _ = _phi_at(T64, G64, ref["D"], v)
        _check_columns("stream 700x300 call %d at h2 = %.6g" % (k, v), _np(got[k]), phi_ref, T64, "phi")
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


# ---------------------------------------------------------------------------------------------------------------
# 7. beyond what the stored-D path can hold comfortably
# ---------------------------------------------------------------------------------------------------------------
def test_large_n_on_a_small_workspace(cuda):
    n, d = 32768, 64
    gen = torch.Generator(device="cpu").manual_seed(5)
    T = torch.randn(n, d, generator=gen).to(cuda)
    G = torch.randn(n, d, generator=gen).to(cuda)
    h2 = _h2_f32(2.0 * d / math.log(n))        # about the heuristic's value for standard normal particles
    eng = _stream_engine(n, d, cuda, h2)
    stored_bytes = _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3)[0]
    print("stream %dx%d: workspace %.1f MiB, stored-D %.1f MiB" % (n, d, eng.ws_bytes / 2.0 ** 20, stored_bytes / 2.0 ** 20))
    assert eng.ws_bytes < stored_bytes / 16
    phi = eng.compute_phi(T, G)
    rows = torch.arange(0, n, n // 48, device=cuda)[:48]
    ref = tf._sampled_fp64(T, G, h2, rows)
    e = ((phi[rows].double() - ref).norm() / ref.norm()).item()
    print("stream %dx%d against fp64 on 48 rows: %.3e" % (n, d, e))
    assert e <= 1e-5, e
    assert np.isfinite(eng.sqnorm.item())


# ---------------------------------------------------------------------------------------------------------------
# 8. the sampler, and everything the streaming engine refuses
# ---------------------------------------------------------------------------------------------------------------
def test_sampler_with_a_fixed_bandwidth(cuda):
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    n, d, h, lr = 100, 10, 1.3, 1e-2
    rng = np.random.default_rng(77)
    mu, T0 = rng.normal(size=d), rng.normal(size=(n, d))

    def score(theta, feed):            # N(mu, 0.5^2 I): d log p / d theta = -(theta - mu) / 0.25
        return -(theta - torch.as_tensor(mu, device=theta.device, dtype=theta.dtype)) / 0.25

    s = SteinSampler(n, None, AdagradGradientDescent(learning_rate=lr), theta=T0.copy(), score=score, device=cuda,
                     dtype=torch.float64, bandwidth=h)
    assert s.engine.streaming and s.engine.h2.item() == _h2_f32(h * h)
    theta, gd, h2 = T0.copy(), orc.AdagradState(learning_rate=lr), _h2_f32(h * h)
    for it in range(3):
        s.train_on_batch(None)
        T32, G32 = ci.f32(theta), ci.f32(-(theta - mu) / 0.25)      # what the kernel path is fed
        phi, _ = _phi_at(T32, G32, orc.pairwise_sq_dists(T32, np.float64), h2)
        theta = theta + gd.update(phi * orc.clip_scale(float(np.sum(phi * phi))))
        e = ci.frobenius_error(s.samples, theta)
        print("sampler, fixed bandwidth %.2f, iteration %d: theta against the fp64 loop %.2e" % (h, it, e))
        assert e <= 1e-5, (it, e)
    assert not np.array_equal(s.samples, T0)
    # the device form, forwarded as it is
    h2t = torch.full((1,), 2.0, dtype=torch.float32, device=cuda)
    s2 = SteinSampler(n, None, AdagradGradientDescent(learning_rate=lr), theta=T0.copy(), score=score, device=cuda, h2=h2t)
    assert s2.engine.h2 is h2t
    s2.train_on_batch(None)
    assert np.isfinite(s2.samples).all()
    for bad in (0.0, -1.0, float("inf"), float("nan"), "wide"):
        with pytest.raises(ValueError):
            SteinSampler(n, None, AdagradGradientDescent(learning_rate=lr), theta=T0.copy(), device=cuda, bandwidth=bad)
    with pytest.raises(ValueError):
        SteinSampler(n, None, AdagradGradientDescent(learning_rate=lr), theta=T0.copy(), device=cuda, bandwidth=h, h2=h2t)


def test_what_the_streaming_engine_refuses(cuda):
    n, d = 100, 10
    T, G = torch.randn(n, d, device=cuda), torch.randn(n, d, device=cuda)
    eng = _stream_engine(n, d, cuda, 1.5)
    eng.compute_phi(T, G)
    with pytest.raises(ValueError, match="dist_matrix"):
        eng.dist_matrix()
    for view in ("rownorm", "dist", "hist", "select_state", "spec_section", "spec_table", "planes"):
        with pytest.raises(ValueError, match="streaming"):
            getattr(eng, view)
    with pytest.raises(ValueError, match="streaming"):
        eng.window_stats()
    with pytest.raises(ValueError, match="K_out"):
        eng.compute_phi(T, G, K_out=torch.empty(n, n, device=cuda))
    with pytest.raises(ValueError, match="dK_out"):
        eng.compute_phi(T, G, dK_out=torch.empty(n, d, device=cuda))
    with pytest.raises(ValueError, match="mark"):
        eng.compute_phi(T, G, mark=lambda label: None)
    with pytest.raises(ValueError, match="ksd"):
        SvgdEngine(n, d, device=cuda, h2=1.5, ksd=True)
    with pytest.raises(ValueError, match="group"):
        SvgdEngine(n, d, device=cuda, h2=1.5, group=object())
    with pytest.raises(ValueError, match="x3=False"):
        SvgdEngine(n, d, device=cuda, h2=1.5, x3=False)
    with pytest.raises(ValueError, match="bf16"):
        SvgdEngine(n, d, device=cuda, h2=1.5, dtype=torch.bfloat16)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="positive and finite"):
            SvgdEngine(n, d, device=cuda, h2=bad)
    for bad in (torch.ones(2, device=cuda), torch.ones(1, dtype=torch.float64, device=cuda), torch.ones(1)):
        with pytest.raises(ValueError, match="1-element float32"):
            SvgdEngine(n, d, device=cuda, h2=bad)
    # h2 = None changes nothing: the default engine is the median heuristic's
    plain = SvgdEngine(n, d, device=cuda)
    assert not plain.streaming and plain.ws_bytes == _lib.workspace_layout(n, n, d, _lib.F32, plain.flags)[0]
