"""GPU: the kernelized Stein discrepancy of the step (STEIN_FLAG_KSD, SvgdEngine(ksd=True), SteinSampler.stein_discrepancy,
utilities.kernelized_stein_discrepancy) against an fp64 pair sum on the device (tests/ksd_ref.py) evaluated with the
engine's own bandwidth.

Errors are measured against the scale  sum_ij |terms of u_ij|  (the sums cancel).  Measured on an MI355X (printed by every
parity case with -s): at most 5.5e-8 with fp32 inputs (160 x 303, one-kernel path; C3 1.7e-8) and 7.4e-7 with bf16
inputs (4096 x 128).  Bounds: 1e-6 and 2e-5.  Comparisons between the sharded and the single-rank step (whose distance
passes round entries differently) keep the wider 1e-5."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ksd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F32, TOL_BF16 = 1e-6, 2e-5
TOL_SHARDED = 1e-5


def _inputs(n, d, seed, dev, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    T = torch.tensor(rng.normal(size=(n, d)), dtype=torch.float32, device=dev)
    G = torch.tensor(-rng.normal(size=(n, d)) * 0.5, dtype=torch.float32, device=dev) - 0.5 * T
    return T.to(dtype), G.to(dtype)


def _errors(eng, T, G):
    """(S error, S_diag error, U error, V error), each over the scale, and the reference statistics"""
    torch.cuda.synchronize()
    n = T.shape[0]
    h2 = float(eng.h2.item())
    S, Sd, scale = R.pairwise_sums(T.to(torch.float64), G.to(torch.float64), h2)
    sums = eng._sums.cpu().tolist()
    u, v = float(eng.stein_discrepancy("u").item()), float(eng.stein_discrepancy("v").item())
    ref_u, ref_v = R.statistic(S, Sd, n, "u"), R.statistic(S, Sd, n, "v")
    return (abs(sums[1] - S) / scale, abs(sums[2] - Sd) / scale, abs(u - ref_u) * n * (n - 1) / scale,
            abs(v - ref_v) * n * n / scale), (ref_u, ref_v, scale)


CASES = [  # (n, d, engine arguments, input dtype, bound)
    (20, 3, {}, torch.float32, TOL_F32),                   # one-kernel path (stein_small.hip), one workgroup
    (100, 10, {}, torch.float32, TOL_F32),
    (160, 303, {}, torch.float32, TOL_F32),                # one-kernel path, ten workgroups: the summed partials
    (1000, 37, {}, torch.float32, TOL_F32),                # tiled split path, ragged shape (scalar finish: d % 4 != 0)
    (1000, 37, {"x3": False}, torch.float32, TOL_F32),     # fp32-MFMA contraction
    (1000, 40, {"small": False}, torch.float32, TOL_F32),  # 16-byte finish
    (4096, 128, {}, torch.float32, TOL_F32),               # panel-resident distance pass
    (4096, 128, {}, torch.bfloat16, TOL_BF16),             # bf16 inputs
    (16384, 256, {}, torch.float32, TOL_F32),              # C3
]


@pytest.mark.parametrize("n,d,kw,dtype,tol", CASES, ids=["%dx%d%s%s" % (c[0], c[1], "".join("-%s=%s" % i for i in c[2].items()),
                                                                       "-bf16" if c[3] == torch.bfloat16 else "") for c in CASES])
def test_parity_with_fp64_pair_sum(cuda, n, d, kw, dtype, tol):
    from stein_amd.engine import SvgdEngine
    T, G = _inputs(n, d, n + d, cuda, dtype)
    eng = SvgdEngine(n, d, device=cuda, dtype=dtype, ksd=True, **kw)
    for _ in range(3):                  # the third call takes the speculative window where the path has one
        eng.compute_phi(T, G)
    errs, _ = _errors(eng, T, G)
    print("ksd %dx%d %s %s: err/scale S %.2e S_diag %.2e U %.2e V %.2e" % ((n, d, kw, dtype) + errs))
    assert max(errs) <= tol, errs


BIT_CASES = [(100, 10, {}, torch.float32), (160, 303, {}, torch.float32), (1000, 37, {}, torch.float32),
             (1000, 40, {"x3": False}, torch.float32), (4096, 128, {}, torch.bfloat16)]


@pytest.mark.parametrize("n,d,kw,dtype", BIT_CASES)
def test_flag_leaves_the_step_bit_identical(cuda, n, d, kw, dtype):
    from stein_amd.engine import SvgdEngine
    T, G = _inputs(n, d, 7, cuda, dtype)
    plain = SvgdEngine(n, d, device=cuda, dtype=dtype, **kw)
    withk = SvgdEngine(n, d, device=cuda, dtype=dtype, ksd=True, **kw)
    dK0, dK1 = torch.empty(n, d, device=cuda), torch.empty(n, d, device=cuda)
    for step in range(4):
        Ts = (T.float() * (1.0 + 0.05 * step)).to(dtype)
        p0 = plain.compute_phi(Ts, G, dK_out=dK0).clone()
        p1 = withk.compute_phi(Ts, G, dK_out=dK1)
        torch.cuda.synchronize()
        assert torch.equal(p0, p1) and torch.equal(dK0, dK1), step
        assert torch.equal(plain.h2, withk.h2) and torch.equal(plain.sqnorm, withk.sqnorm), step
        assert withk.sqnorm.data_ptr() == withk._sums.data_ptr()


def test_statistic_separates_a_good_sample_from_a_shifted_one(cuda):
    from stein_amd.engine import SvgdEngine
    n, d = 1000, 10
    X = torch.tensor(np.random.default_rng(3).normal(size=(n, d)), dtype=torch.float32, device=cuda)
    out = {}
    for shift in (0.0, 2.0):
        Xs = X + shift
        eng = SvgdEngine(n, d, device=cuda, ksd=True)
        eng.compute_phi(Xs, -Xs)            # the score of N(0, I)
        errs, (ref_u, _, _) = _errors(eng, Xs, -Xs)
        assert max(errs) <= TOL_F32, errs
        out[shift] = (float(eng.stein_discrepancy("u").item()), ref_u)
    # fp64 reference: 1.1e-3 vs 2.54, a ratio of 4.4e-4
    assert out[0.0][1] < 1e-3 * out[2.0][1]
    assert out[0.0][0] < 1e-2 * out[2.0][0], out


def test_sampler_discrepancy_falls_over_the_linear_regression_example(cuda):
    """examples/linear_regression: GlmScore, 50 particles, Adam(0.1).  The NumPy oracle's run (oracle.svgd_oracle, same
    start, 500 iterations) goes from KSD_U = 1.0e7 after the first step to |KSD_U| < 80 (ratio < 8e-6): bound 1e-4."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "linear_regression"))
    from main import make_data
    from stein_amd.optimizers import AdamGradientDescent
    from stein_amd.samplers import SteinSampler
    from stein_amd.scores import GlmScore
    X, y, _ = make_data()
    feed = {"X": torch.tensor(X, dtype=torch.float32, device=cuda), "y": torch.tensor(y, dtype=torch.float32, device=cuda)}
    theta = {"model/w:0": np.random.default_rng(5).normal(size=(50, 1, 1)) * 0.01}
    s = SteinSampler(50, None, AdamGradientDescent(learning_rate=1e-1), theta=theta, score=GlmScore("linear", 1),
                     device=cuda, ksd=True)
    with pytest.raises(RuntimeError, match="no step"):
        s.stein_discrepancy()
    s.train_on_batch(feed)
    first = s.stein_discrepancy()
    for _ in range(499):
        s.train_on_batch(feed)
    last = s.stein_discrepancy()
    print("linear regression KSD_U: first %.4e last %.4e" % (first, last))
    assert first > 1e6 and abs(last) < 1e-4 * first
    assert s.stein_discrepancy("v") > 0.0


def test_sampler_and_engine_refuse_what_has_no_statistic(cuda):
    from stein_amd.engine import SvgdEngine
    from stein_amd.optimizers import AdagradGradientDescent
    from stein_amd.samplers import SteinSampler
    T, G = _inputs(64, 4, 1, cuda)
    s = SteinSampler(64, None, AdagradGradientDescent(), theta=T.cpu().numpy(), device=cuda)
    s.update_particles(G)
    with pytest.raises(RuntimeError, match="ksd=True"):
        s.stein_discrepancy()
    s = SteinSampler(64, None, AdagradGradientDescent(), theta=T.cpu().numpy(), device=cuda, ksd=True)
    s.update_particles(G)
    assert np.isfinite(s.stein_discrepancy())

    class Foreign:
        def kernel_and_grad(self, th):
            return np.eye(th.shape[0]), np.zeros_like(th)
    s.kernel = Foreign()
    with pytest.raises(RuntimeError, match="user-supplied kernel"):
        s.stein_discrepancy()
    eng = SvgdEngine(300, 5, device=cuda, ksd=True)
    T, G = _inputs(300, 5, 2, cuda)
    with pytest.raises(ValueError, match="mark="):
        eng.compute_phi(T, G, mark=lambda label: None)
    with pytest.raises(ValueError, match="'u' or 'v'"):
        eng.compute_phi(T, G)
        eng.stein_discrepancy("w")


def test_standalone_call(cuda):
    from stein_amd.engine import SvgdEngine
    from stein_amd.utilities import kernelized_stein_discrepancy as ksd
    for n, d, dtype, tol in ((300, 7, torch.float32, TOL_F32), (90, 33, torch.float32, TOL_F32),
                             (600, 64, torch.bfloat16, TOL_BF16)):
        T, G = _inputs(n, d, 9, cuda, dtype)
        eng = SvgdEngine(n, d, device=cuda, dtype=dtype)        # the same bandwidth, for the reference
        eng.compute_phi(T, G)
        S, Sd, scale = R.pairwise_sums(T.double(), G.double(), float(eng.h2.item()))
        for stat, norm in (("u", n * (n - 1)), ("v", n * n)):
            got = ksd(T, G, statistic=stat)
            assert isinstance(got, float)
            assert abs(got - R.statistic(S, Sd, n, stat)) * norm <= tol * scale, (n, d, stat)
    T, G = _inputs(50, 4, 3, cuda)
    with pytest.raises(ValueError, match="device"):
        ksd(T.cpu(), G.cpu())
    with pytest.raises(ValueError, match="same shape"):
        ksd(T, G[:40])
    with pytest.raises(ValueError, match="at least two"):
        ksd(T[:1], G[:1])
    with pytest.raises(ValueError, match=r"\[n, d\]"):
        ksd(T[0], G[0])
    with pytest.raises(ValueError, match="same shape"):
        ksd(T, G.bfloat16())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_gloo(rank, world, port, n, d, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from stein_amd.engine import SvgdEngine
        T, G = _inputs(n, d, 13, "cuda:0")
        nl = n // world
        sl = slice(rank * nl, (rank + 1) * nl)
        res = []
        for window in (False, True):
            eng = SvgdEngine(n, d, device="cuda:0", group=dist.group.WORLD, ksd=True, dist_window=window)
            eng.compute_phi(T[sl].contiguous(), G[sl].contiguous())
            res.append(eng._sums.cpu().numpy())
        np.save(os.path.join(out_dir, "k%d.npy" % rank), np.array(res))
    finally:
        dist.destroy_process_group()


def test_two_ranks_give_the_single_rank_statistic(cuda, tmp_path):
    from stein_amd.engine import SvgdEngine
    n, d, world = 1280, 130, 2
    mp.spawn(_worker_gloo, args=(world, _free_port(), n, d, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "k%d.npy" % r)) for r in range(world)]
    assert np.array_equal(parts[0], parts[1])            # all-reduced: the same three doubles on every rank
    T, G = _inputs(n, d, 13, cuda)
    one = SvgdEngine(n, d, device=cuda, ksd=True)
    one.compute_phi(T, G)
    _, (_, _, scale) = _errors(one, T, G)
    ref = one._sums.cpu().numpy()
    for sums in parts[0]:
        assert abs(sums[0] - ref[0]) <= 1e-6 * ref[0]
        assert abs(sums[1] - ref[1]) <= TOL_SHARDED * scale and abs(sums[2] - ref[2]) <= TOL_SHARDED * scale, (sums, ref)


def _worker_rccl(rank, port, n, d, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from stein_amd.engine import SvgdEngine
        T, G = _inputs(n, d, 17, dev)
        out = {}
        for comm in ("native", "torch"):
            for x3 in (False, True):
                eng = SvgdEngine(n, d, device=dev, group=dist.group.WORLD, force_collectives=True, comm=comm, x3=x3,
                                 ksd=True, dist_window=True)
                for _ in range(3):
                    eng.compute_phi(T, G)
                out["%s_%d" % (comm, int(x3))] = eng._sums.cpu().numpy()
                eng.close()
        np.save(os.path.join(out_dir, "rccl_ksd.npy"), out, allow_pickle=True)
    finally:
        dist.destroy_process_group()


def test_native_rank_step_reduces_all_three_sums(cuda, tmp_path):
    from stein_amd.engine import SvgdEngine
    n, d = 1280, 130
    mp.spawn(_worker_rccl, args=(_free_port(), n, d, str(tmp_path)), nprocs=1, join=True)
    out = np.load(os.path.join(str(tmp_path), "rccl_ksd.npy"), allow_pickle=True).item()
    T, G = _inputs(n, d, 17, cuda)
    for x3 in (0, 1):
        assert np.array_equal(out["native_%d" % x3], out["torch_%d" % x3])   # the same kernels and reductions
        one = SvgdEngine(n, d, device=cuda, ksd=True, x3=bool(x3))
        one.compute_phi(T, G)
        _, (_, _, scale) = _errors(one, T, G)
        ref = one._sums.cpu().numpy()
        got = out["native_%d" % x3]
        assert abs(got[1] - ref[1]) <= TOL_SHARDED * scale and abs(got[2] - ref[2]) <= TOL_SHARDED * scale, (got, ref)
