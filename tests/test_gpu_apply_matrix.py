"""GPU: the optimizer apply kernels and the casts of csrc/stein_apply.hip through the C ABI, against the fp64 optimizer
maps of oracle/svgd_oracle.py (AdagradState / AdamState / clip_scale, pinned by the goldens).

The matrix pairs its factors instead of taking their product: every count with every dtype pairing, every count above
524 288 elements (where the scalar loops stride the grid; the float4 Adagrad loop strides above 2 097 152) with both
optimizers, and theta / step_out present or NULL with the five clip modes in every combination.  Each case runs three
consecutive steps (Adam: and one at t = 10000 resumed from a supplied state); before every step the reference takes
over the state the device holds, so each bound is the bound of ONE step, relative to the reference's own entry:
  fp64 state (phi fp32-representable)  rtol 1e-13 on step and state, |d theta| <= 1e-13 |step| + 2^-52 |theta|
  fp32 state                           rtol 2e-6 on step and state,  |d theta| <= 2e-6 |step| + 2^-23 |theta|
A bound relative to the result of Adam's mu = b1 mu + (1 - b1) p presumes that its two terms do not cancel, so in the
matrix every phi of a case and the resumed mu carry the sign pattern of the first phi.  Momentum that does cancel is
the business of test_adam_momentum_that_cancels_is_held_to_its_operands, whose bound is relative to the operands
|b1 mu| + |(1 - b1) p|: no arithmetic of the state's precision can hold a cancelled sum to a bound relative to it.
The clip modes "exact" (*sq = 100.0 = threshold^2, |phi| = 10) and "zero" (*sq = 0) must give scale 1 EXACTLY: each
of their steps is repeated from the same state with no device sqnorm and a host scale of 1.0, bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import svgd_oracle as orc
from stein_amd import _lib

COUNTS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 524287, 524288, 524289, 2097152 + 4, 2097152 + 7, 4194304]
PAIRINGS = {"f32_f32": (torch.float32, torch.float32), "f64_f32": (torch.float64, torch.float32),
            "f64_f64": (torch.float64, torch.float64)}
CLIPS = ("below", "exact", "above", "zero", "host")
THR = 10.0
LR, ALPHA, B1, B2 = 1e-2, 0.9, 0.9, 0.999


def _matrix():
    cases, k = [], 0
    for i, count in enumerate(COUNTS):
        for j, pair in enumerate(PAIRINGS):
            for opt in (("adagrad", "adam") if count > 524288 else (("adagrad", "adam")[(i + j) % 2],)):
                cases.append((opt, count, pair, k % 2 == 0, (k // 2) % 2 == 0, CLIPS[k % 5]))
                k += 1
    return cases


MATRIX = _matrix()


def test_the_matrix_pairs_every_factor():
    assert {(c[1], c[2]) for c in MATRIX} == {(n, p) for n in COUNTS for p in PAIRINGS}
    for n in COUNTS:
        if n > 524288:
            assert {(c[0], c[2]) for c in MATRIX if c[1] == n} == {(o, p) for o in ("adagrad", "adam") for p in PAIRINGS}
    assert {c[3:] for c in MATRIX} == {(t, s, cl) for t in (True, False) for s in (True, False) for cl in CLIPS}
    for opt in ("adagrad", "adam"):
        mine = [c for c in MATRIX if c[0] == opt]
        assert {c[5] for c in mine} == set(CLIPS) and {c[3] for c in mine} == {True, False} == {c[4] for c in mine}
        assert {c[2] for c in mine if c[1] % 4 and c[1] > 4} == set(PAIRINGS)          # every pairing at a tail count
        assert any(c[5] != "host" and not c[3] and c[4] for c in mine)                 # theta NULL + step_out with a device sqnorm
    assert max(COUNTS) == 16384 * 256 and {524287, 524288, 524289, 2097152 + 4} <= set(COUNTS)


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=2)
def _base(count):
    rng = np.random.default_rng(count)
    return _r32(rng.normal(size=count)), _r32(rng.normal(size=count))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _code(dtype):
    return _lib.F32 if dtype == torch.float32 else _lib.F64


def _adagrad(cuda, theta, phi, hist, sq, host_scale, first, step_out, count=None):
    _lib.call("stein_apply_adagrad", _p(theta), _p(phi), _code(phi.dtype), _p(hist), phi.numel() if count is None else count,
              _code(hist.dtype), _p(sq), host_scale, THR, LR, ALPHA, orc.ADAGRAD_EPS, first, _p(step_out), _stream(cuda))


def _adam(cuda, theta, phi, mu, nu, sq, host_scale, t, step_out):
    _lib.call("stein_apply_adam", _p(theta), _p(phi), _code(phi.dtype), _p(mu), _p(nu), phi.numel(), _code(mu.dtype), _p(sq),
              host_scale, THR, LR, B1, B2, orc.ADAM_EPS, t, _p(step_out), _stream(cuda))


def _np(t):
    return t.double().cpu().numpy()


def _ibits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _within(what, got, ref, tol):
    err = np.abs(_np(got) - ref)
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, "%s: %d of %d outside the bound, first at %d: got %r ref %r tol %.3g" % (
        what, bad.size, err.size, bad[0], float(_np(got)[bad[0]]), float(ref[bad[0]]), float(np.broadcast_to(tol, err.shape)[bad[0]]))


@pytest.mark.gpu
@pytest.mark.parametrize("opt,count,pair,theta_on,step_on,clip", MATRIX,
                         ids=["%s-%d-%s-%s%s-%s" % (c[0], c[1], c[2], "T" if c[3] else "t", "S" if c[4] else "s", c[5]) for c in MATRIX])
def test_apply_matches_the_fp64_optimizer(cuda, opt, count, pair, theta_on, step_on, clip):
    sdt, pdt = PAIRINGS[pair]
    rt, ulp = (2e-6, 2.0 ** -23) if sdt == torch.float32 else (1e-13, 2.0 ** -52)
    base, theta0 = _base(count)
    rng = np.random.default_rng([count, 1])
    norm = {"below": 3.0, "exact": THR, "above": 40.0, "zero": 40.0, "host": 40.0}[clip]
    phi0 = _r32(base * (norm / max(np.linalg.norm(base), 1e-30)))
    sq_true = float(np.sum(phi0 * phi0))
    assert abs(np.sqrt(sq_true) - norm) <= 1e-6 * norm        # (rounding phi to fp32 moves |phi| off 10 by some 1e-8)
    sq_val = {"below": sq_true, "above": sq_true, "exact": THR * THR, "zero": 0.0, "host": None}[clip]
    sq = None if sq_val is None else torch.tensor([sq_val], dtype=torch.float64, device=cuda)
    host_scale = orc.clip_scale(sq_true) if clip == "host" else 123.0       # ignored whenever a device sqnorm is given
    scale = orc.clip_scale(sq_true if clip == "host" else sq_val)
    if clip in ("exact", "zero", "below"):
        assert scale == 1.0
    else:
        assert scale < 0.5
    sign = np.sign(phi0)
    assert (sign != 0).all()
    phis = [phi0, sign * np.abs(np.roll(phi0, 1)), sign * np.abs(np.roll(phi0, 2))]     # one sign pattern: mu never cancels
    theta = torch.tensor(theta0, dtype=sdt, device=cuda) if theta_on else None
    step_out = torch.full((count,), float("nan"), dtype=sdt, device=cuda) if step_on else None
    state = [torch.full((count,), float("nan"), dtype=sdt, device=cuda) for _ in range(1 if opt == "adagrad" else 2)]
    steps = [(k + 1, phis[k]) for k in range(3)]
    if opt == "adam":
        steps.append((10000, phis[0]))
    for t, phi_np in steps:
        phi = torch.tensor(phi_np, dtype=pdt, device=cuda)
        if t == 10000:                                       # resume from a supplied state
            state[0].copy_(torch.tensor(_r32(sign * np.abs(rng.normal(size=count))), dtype=sdt))
            state[1].copy_(torch.tensor(_r32(rng.normal(size=count) ** 2), dtype=sdt))
        before = [_np(s) for s in state]
        th_before = _np(theta) if theta_on else None
        twin = None
        if clip in ("exact", "zero"):                        # the same step from the same state, unclipped by the host
            twin = dict(state=[s.clone() for s in state], theta=theta.clone() if theta_on else None,
                        step=torch.full_like(step_out, float("nan")) if step_on else None)
        p = phi_np * scale
        if opt == "adagrad":
            gd = orc.AdagradState(learning_rate=LR, alpha=ALPHA)
            gd.n_iters, gd.hist = t - 1, before[0]
            step_ref = gd.update(p)
            state_ref = [gd.hist]
            _adagrad(cuda, theta, phi, state[0], sq, host_scale, 1 if t == 1 else 0, step_out)
            if twin:
                _adagrad(cuda, twin["theta"], phi, twin["state"][0], None, 1.0, 1 if t == 1 else 0, twin["step"])
        else:
            gd = orc.AdamState(learning_rate=LR, beta_1=B1, beta_2=B2)
            gd.n_iters, gd.mu, gd.nu = t - 1, before[0], before[1]
            step_ref = gd.update(p)
            assert t == 1 or (before[0] * p > 0).all()        # precondition: the two terms of mu do not cancel
            state_ref = [gd.mu, gd.nu]
            _adam(cuda, theta, phi, state[0], state[1], sq, host_scale, t, step_out)
            if twin:
                _adam(cuda, twin["theta"], phi, twin["state"][0], twin["state"][1], None, 1.0, t, twin["step"])
        torch.cuda.synchronize()
        step_tol = rt * np.abs(step_ref)
        for name, s, r in zip(("state0", "state1"), state, state_ref):
            _within("%s at t=%d" % (name, t), s, r, rt * np.abs(r))
        if step_on:
            _within("step at t=%d" % t, step_out, step_ref, step_tol)
        if theta_on:
            ref = th_before + step_ref
            _within("theta at t=%d" % t, theta, ref, step_tol + ulp * np.abs(ref))
        if twin:
            pairs = list(zip(state, twin["state"])) + ([(theta, twin["theta"])] if theta_on else []) + ([(step_out, twin["step"])] if step_on else [])
            for got, want in pairs:
                assert torch.equal(_ibits(got), _ibits(want)), "clip %r is not scale 1 exactly at t=%d" % (clip, t)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["f32_f32", "f64_f32", "f64_f64"])
@pytest.mark.parametrize("count", [1023, 524289])
def test_adam_momentum_that_cancels_is_held_to_its_operands(cuda, count, pair):
    """mu = b1 mu + (1 - b1) p with the two terms of opposite sign on half the elements and nearly equal size on some of
    them (every eighth element has (1 - b1) p = -b1 mu to within 2^-10).  The bound on mu cannot be relative to the
    result there: the terms are each rounded once in the state's precision before they are added, so the error is
    proportional to |b1 mu| + |(1 - b1) p| whatever is left of the sum.  The bound is therefore the matrix's rtol applied
    to that operand sum (the same bound wherever the terms do not cancel), the step's bound follows from mu's through
    step = lr (mu / corr1) / (eps + sqrt(nu / corr2)), and nu (a sum of positive terms) keeps the bound relative to itself."""
    sdt, pdt = PAIRINGS[pair]
    rt, ulp = (2e-6, 2.0 ** -23) if sdt == torch.float32 else (1e-13, 2.0 ** -52)
    rng = np.random.default_rng([count, 2])
    phi_np = _r32(rng.normal(size=count))
    mu0 = _r32(rng.normal(size=count))
    near = np.arange(count) % 8 == 0
    mu0[near] = _r32(-(1.0 - B1) / B1 * phi_np[near] * (1.0 + 2.0 ** -10 * rng.uniform(-1, 1, size=int(near.sum()))))
    nu0, theta0 = _r32(rng.normal(size=count) ** 2), _r32(rng.normal(size=count))
    assert 0.3 < np.mean(mu0 * phi_np < 0) < 0.8
    for t in (2, 10000):
        mu, nu, theta = (torch.tensor(a, dtype=sdt, device=cuda) for a in (mu0, nu0, theta0))
        phi = torch.tensor(phi_np, dtype=pdt, device=cuda)
        step_out = torch.full((count,), float("nan"), dtype=sdt, device=cuda)
        gd = orc.AdamState(learning_rate=LR, beta_1=B1, beta_2=B2)
        gd.n_iters, gd.mu, gd.nu = t - 1, mu0.copy(), nu0.copy()
        step_ref = gd.update(phi_np)
        mu_mag = np.abs(B1 * mu0) + np.abs((1.0 - B1) * phi_np)
        assert (mu_mag[near] >= 1000.0 * np.abs(gd.mu[near])).all()            # the cancellation is there
        step_tol = rt * (mu_mag / (1.0 - B1 ** t)) / (orc.ADAM_EPS + np.sqrt(gd.nu / (1.0 - B2 ** t))) * LR
        assert (step_tol >= rt * np.abs(step_ref) * (1 - 1e-9)).all()
        _adam(cuda, theta, phi, mu, nu, None, 1.0, t, step_out)
        torch.cuda.synchronize()
        _within("mu at t=%d" % t, mu, gd.mu, rt * mu_mag)
        _within("nu at t=%d" % t, nu, gd.nu, rt * np.abs(gd.nu))
        _within("step at t=%d" % t, step_out, step_ref, step_tol)
        ref = theta0 + step_ref
        _within("theta at t=%d" % t, theta, ref, step_tol + ulp * np.abs(ref))


def _off16(t, cuda):
    """a copy of `t` whose storage starts one element (4 or 8 bytes) past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=cuda)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size()
    return v


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [4194304, 2097152 + 4, 1028])
def test_adagrad_float4_and_scalar_paths_are_bit_equal(cuda, count):
    """The float4 path (every pointer 16-byte aligned, count % 4 == 0, no step_out) against the scalar path forced one
    way at a time: theta, phi or hist four bytes off a 16-byte boundary, a step_out, a count that is no multiple of 4."""
    g = torch.Generator(device="cpu").manual_seed(count)
    phi, theta0 = torch.randn(count, generator=g).to(cuda), torch.randn(count, generator=g).to(cuda)
    hist0 = (torch.randn(count, generator=g) ** 2).to(cuda)
    sq = torch.tensor([float((phi.double() ** 2).sum()) * 4.0], dtype=torch.float64, device=cuda)   # clipped: scale = THR / (2 |phi|)
    for first in (1, 0):
        th_v, hi_v = theta0.clone(), hist0.clone()
        assert all(t.data_ptr() % 16 == 0 for t in (th_v, hi_v, phi)) and count % 4 == 0
        _adagrad(cuda, th_v, phi, hi_v, sq, 1.0, first, None)
        variants = {"theta": (_off16(theta0, cuda), phi, hist0.clone(), None), "phi": (theta0.clone(), _off16(phi, cuda), hist0.clone(), None),
                    "hist": (theta0.clone(), phi, _off16(hist0, cuda), None),
                    "step_out": (theta0.clone(), phi, hist0.clone(), torch.empty_like(phi))}
        for name, (th, ph, hi, so) in variants.items():
            _adagrad(cuda, th, ph, hi, sq, 1.0, first, so)
            torch.cuda.synchronize()
            assert torch.equal(_bits(th), _bits(th_v)) and torch.equal(_bits(hi), _bits(hi_v)), "%s (first=%d)" % (name, first)
            if so is not None:       # theta + step in fp32 is what the kernel stores
                assert torch.equal(_bits(theta0 + so), _bits(th_v))
        th, hi = theta0.clone(), hist0.clone()
        _adagrad(cuda, th, phi, hi, sq, 1.0, first, None, count=count - 1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(th[:-1]), _bits(th_v[:-1])) and torch.equal(_bits(hi[:-1]), _bits(hi_v[:-1])), "count %% 4 != 0 (first=%d)" % first
        assert torch.equal(_bits(th[-1:]), _bits(theta0[-1:])) and torch.equal(_bits(hi[-1:]), _bits(hist0[-1:]))   # not touched


@pytest.mark.gpu
@pytest.mark.parametrize("count", [4194304, 1023])
def test_adam_does_not_depend_on_alignment(cuda, count):
    g = torch.Generator(device="cpu").manual_seed(count)
    phi, theta0, mu0 = (torch.randn(count, generator=g).to(cuda) for _ in range(3))
    nu0 = (torch.randn(count, generator=g) ** 2).to(cuda)
    sq = torch.tensor([float((phi.double() ** 2).sum()) * 4.0], dtype=torch.float64, device=cuda)   # clipped: scale = THR / (2 |phi|)
    for t in (1, 7):
        ref = [theta0.clone(), mu0.clone(), nu0.clone(), torch.empty_like(phi)]
        _adam(cuda, ref[0], phi, ref[1], ref[2], sq, 1.0, t, ref[3])
        for which in ("theta", "phi", "mu", "nu", "step_out"):
            th, ph, mu, nu, so = theta0.clone(), phi, mu0.clone(), nu0.clone(), torch.empty_like(phi)
            if which == "theta":
                th = _off16(theta0, cuda)
            elif which == "phi":
                ph = _off16(phi, cuda)
            elif which == "mu":
                mu = _off16(mu0, cuda)
            elif which == "nu":
                nu = _off16(nu0, cuda)
            else:
                so = _off16(so, cuda)
            _adam(cuda, th, ph, mu, nu, sq, 1.0, t, so)
            torch.cuda.synchronize()
            for a, b in zip((th, mu, nu, so), ref):
                assert torch.equal(_bits(a), _bits(b)), "%s off a 16-byte boundary (t=%d)" % (which, t)


CAST_COUNTS = [1, 257, 524288 + 3]


def _tile(special, count, rng_values):
    out = np.concatenate([special, rng_values])
    return np.resize(out, count) if count >= out.size else out[:count]


@pytest.mark.gpu
@pytest.mark.parametrize("count", CAST_COUNTS)
def test_cast_f64_to_f32_rounds_like_numpy(cuda, count):
    rng = np.random.default_rng(count)
    fmax, tiny = float(np.finfo(np.float32).max), 2.0 ** -149
    special = np.array([1.0 + 2.0 ** -24, 0.0, -0.0, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -50,   # ties, +-0
                        fmax, fmax + 2.0 ** 102, fmax + 2.0 ** 103, np.nextafter(fmax + 2.0 ** 103, 0), -fmax - 2.0 ** 103, 1e39, -1e39, 1e308,
                        np.inf, -np.inf,                                                                                      # overflow
                        tiny, 0.5 * tiny, np.nextafter(0.5 * tiny, 1), 1.5 * tiny, 2.5 * tiny, -0.5 * tiny, 2.0 ** -126, 2.0 ** -126 - 2.0 ** -150,
                        2.0 ** -127 + 2.0 ** -150, 1e-45, 1e-46, 5e-324, -5e-324, 1e-300])                                    # subnormals
    vals = _tile(special, count, rng.normal(size=1000) * 10.0 ** rng.uniform(-44, 38, size=1000))
    with np.errstate(over="ignore", under="ignore"):
        want = vals.astype(np.float32)
    src = torch.tensor(vals, dtype=torch.float64, device=cuda)
    dst = torch.full((count + 1,), 7.0, dtype=torch.float32, device=cuda)
    _lib.call("stein_cast_f64_to_f32", _p(src), _p(dst), count, _stream(cuda))
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert got[count] == 7.0
    assert np.array_equal(got[:count].view(np.int32), want.view(np.int32))
    nan = torch.tensor([np.nan, 1.0, -np.nan][:min(count, 3)], dtype=torch.float64, device=cuda)
    out = torch.zeros(nan.numel(), dtype=torch.float32, device=cuda)
    _lib.call("stein_cast_f64_to_f32", _p(nan), _p(out), nan.numel(), _stream(cuda))
    assert torch.equal(torch.isnan(out), torch.isnan(nan))


@pytest.mark.gpu
@pytest.mark.parametrize("count", CAST_COUNTS)
def test_cast_f32_to_bf16_rounds_like_torch(cuda, count):
    rng = np.random.default_rng(count)

    def f32(bits):
        return np.array(bits, dtype=np.uint32).view(np.float32)
    special = f32([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,         # ties to even, either side, near ties
                   0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF,   # +-0, +-inf, overflow by rounding
                   0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000, 0x807F8000])  # subnormals
    rand = (rng.normal(size=1000) * 10.0 ** rng.uniform(-44, 38, size=1000)).astype(np.float32)
    vals = _tile(special, count, rand)
    want = torch.tensor(vals).to(torch.bfloat16)                       # CPU torch: round to nearest even
    src = torch.tensor(vals, device=cuda)
    dst = torch.full((count + 1,), 7.0, dtype=torch.bfloat16, device=cuda)
    _lib.call("stein_cast_f32_to_bf16", _p(src), _p(dst), count, _stream(cuda))
    torch.cuda.synchronize()
    assert float(dst[count]) == 7.0
    assert torch.equal(dst[:count].cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(dst[:count], src.to(torch.bfloat16))             # and the device's own conversion
    nan = torch.tensor(f32([0x7FC00000, 0x3F800000, 0x7F800001, 0xFFFFFFFF])[:min(count, 4)], device=cuda)
    out = torch.zeros(nan.numel(), dtype=torch.bfloat16, device=cuda)
    _lib.call("stein_cast_f32_to_bf16", _p(nan), _p(out), nan.numel(), _stream(cuda))
    assert torch.equal(torch.isnan(out), torch.isnan(nan))
