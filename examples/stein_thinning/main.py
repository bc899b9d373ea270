"""Stein thinning of an SVGD run: the m particles that best represent all n.

    python examples/stein_thinning/main.py [--particles 1024] [--iters 300] [--m 64]

runs the sampler of examples/logistic_regression (synthetic data of Covertype's shape, HIP score producer), then picks m
of its particles with SteinSampler.thin (stein_amd.utilities.stein_thinning: greedy minimisation of the kernelized Stein
discrepancy under the IMQ kernel at the median bandwidth of all n) and prints KSD^2 (V-statistic, same kernel, same
bandwidth, full-data score) of the m chosen against the first m particles and a random m.

    python examples/stein_thinning/main.py --time [--shapes 4096x256x256,...] [--reps 5] [--no-torch] [--grid P]

measures the thinning call alone on synthetic particles: milliseconds per pick (device events around the m + 1 launches,
median of --reps after a warm-up) and the effective rate over the 8 n d bytes a pick reads, beside the same greedy loop
written in torch on the device (per pick two [n, d] x [d, 2] products, the elementwise Stein kernel, an add and an
argmin; no n x n matrix).  --grid forces the number of workgroups (stein_debug_thin_grid), --no-torch skips the torch
loop (a profiler run of the kernel alone).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from stein_amd import _lib  # noqa: E402
from stein_amd.optimizers import AdamGradientDescent  # noqa: E402
from stein_amd.samplers import SteinSampler  # noqa: E402
from stein_amd.scores import GlmScore  # noqa: E402
from stein_amd.stream_engine import StreamEngine  # noqa: E402
from stein_amd.utilities import kernelized_stein_discrepancy, stein_thinning  # noqa: E402

DEFAULT_SHAPES = "4096x256x256,16384x256x1024,8192x2001x256,262144x16x1024"


def logistic_example():
    spec = importlib.util.spec_from_file_location("logistic_main", os.path.join(HERE, "..", "logistic_regression", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_sampler(args):
    (Xtr, ytr), _ = logistic_example().make_data()
    dev = "cuda"
    Xtr_t, ytr_t = torch.tensor(Xtr, dtype=torch.float32, device=dev), torch.tensor(ytr, dtype=torch.float32, device=dev)
    score = GlmScore("logistic", Xtr.shape[1], w_col=1, alpha_col=0, n_train=len(Xtr))
    sampler = SteinSampler(args.particles, None, AdamGradientDescent(learning_rate=1e-1), score=score,
                           model_vars={"model/w:0": [Xtr.shape[1], 1], "model/log_alpha:0": []})
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(args.iters):
        idx = torch.randint(0, len(Xtr), (args.batch,), device=dev, generator=gen)
        sampler.train_on_batch({"X": Xtr_t[idx], "y": ytr_t[idx]})
    return sampler, {"X": Xtr_t, "y": ytr_t}


def thin_example(args):
    sampler, full = run_sampler(args)
    n, m = args.particles, args.m
    theta, score = sampler.theta_matrix.float().contiguous(), sampler.score_matrix(full)
    h2 = StreamEngine(n, theta.shape[1], device=theta.device, h2="median").refresh_bandwidth(theta).clone()
    idx, ksd2 = sampler.thin(m, full, bandwidth=h2, return_ksd=True)
    h = float(h2.sqrt().item())
    gen = torch.Generator(device=theta.device).manual_seed(1)
    sets = {"thinned": idx, "first m": torch.arange(m, device=theta.device),
            "random m": torch.randperm(n, device=theta.device, generator=gen)[:m]}
    print("%d particles after %d steps, median bandwidth h = %.4f; KSD^2_V (IMQ) of all of them: %.4e" %
          (n, args.iters, h, kernelized_stein_discrepancy(theta, score, "v", bandwidth=h, kernel="imq")))
    for name, sel in sets.items():
        v = kernelized_stein_discrepancy(theta[sel].contiguous(), score[sel].contiguous(), "v", bandwidth=h, kernel="imq")
        print("  %-9s m = %d: KSD^2_V = %.4e (%d distinct particles)" % (name, m, v, len(set(sel.tolist()))))
    print("  the thinning call's own running statistic after pick 1, m/2, m: %.4e  %.4e  %.4e" %
          (float(ksd2[0]), float(ksd2[m // 2 - 1] if m > 1 else ksd2[0]), float(ksd2[-1])))


def torch_greedy(X, G, h2, m, kernel="imq"):
    """the same greedy loop in torch on the device, no n x n matrix and no host read -> picks [m]"""
    n, d = X.shape
    c2 = 2.0 * h2
    r, a = (X * X).sum(1), (G * X).sum(1)
    obj = 0.5 * ((G * G).sum(1).double() + d / (c2 if kernel == "imq" else h2))
    picks = torch.empty(m, dtype=torch.int64, device=X.device)
    for t in range(m):
        s = obj.argmin().view(1)
        picks[t:t + 1] = s
        B = torch.cat([X.index_select(0, s), G.index_select(0, s)], 0).T           # [d, 2] = [x_s | g_s]
        XB, GB = X @ B, G @ B
        D = (r + r.index_select(0, s) - 2.0 * XB[:, 0]).clamp_min(0.0)
        cross = a + a.index_select(0, s) - XB[:, 1] - GB[:, 0]
        gg = GB[:, 1]
        if kernel == "imq":
            k = torch.rsqrt(1.0 + D / c2)
            k3 = k * k * k
            u = k * gg + k3 * cross / c2 + d * k3 / c2 - 3.0 * k3 * k * k * D / (c2 * c2)
        else:
            u = torch.exp(-D / c2) * (gg + cross / h2 + d / h2 - D / (h2 * h2))
        obj += u.double()
    return picks


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def time_shapes(args):
    dev = torch.device("cuda")
    _lib.debug_thin_grid(args.grid)
    print("thinning call alone, IMQ kernel, fixed bandwidth h2 = d / 2; %d timed repeats after one warm-up; grid %s" %
          (args.reps, args.grid or "default"))
    for spec in args.shapes.split(","):
        n, d, m = (int(x) for x in spec.split("x"))
        gen = torch.Generator(device=dev).manual_seed(n + d)
        X = (1.5 * torch.randn(n, d, device=dev, generator=gen) + 0.3).contiguous()
        G = -X
        h2 = 0.5 * d
        h2_t = torch.full((1,), h2, dtype=torch.float32, device=dev)
        got = []

        def ours():
            got[:] = [stein_thinning(X, G, m, bandwidth=h2_t, kernel="imq")]
        med, lo, hi = _ms(ours, args.reps)
        bytes_per_pick = 8.0 * n * d
        line = "%7d x %4d, m = %4d: %8.4f ms per pick (min %.4f max %.4f), %7.1f GB/s over 8 n d bytes" % (
            n, d, m, med / m, lo / m, hi / m, bytes_per_pick / (med / m * 1e-3) / 1e9)
        if not args.no_torch:
            ref = []

            def theirs():
                ref[:] = [torch_greedy(X, G, h2, m)]
            tmed, tlo, thi = _ms(theirs, max(2, args.reps // 2))
            same = float((ref[0] == got[0]).double().mean())
            line += " | torch loop %8.4f ms per pick (min %.4f max %.4f): %.2fx; picks equal %.3f" % (
                tmed / m, tlo / m, thi / m, tmed / med, same)
        print(line, flush=True)
    _lib.debug_thin_grid(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--time", action="store_true", help="measure the thinning call on synthetic particles instead")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated n x d x m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--grid", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    if args.time:
        time_shapes(args)
    else:
        thin_example(args)


if __name__ == "__main__":
    main()
