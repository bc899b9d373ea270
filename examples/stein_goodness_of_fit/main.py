"""KSD goodness-of-fit test of an SVGD run's particles: is the statistic large for this n, target and bandwidth?

    python examples/stein_goodness_of_fit/main.py [--particles 1024] [--early 10] [--iters 300] [--boot 511]

runs the sampler of examples/logistic_regression (synthetic data of Covertype's shape, HIP score producer) and prints
KSD^2 (V-statistic, IMQ kernel, median bandwidth, full-data score) with its wild-bootstrap p-value
(SteinSampler.goodness_of_fit -> stein_amd.utilities.stein_goodness_of_fit) after --early steps and after --iters.
SVGD particles interact: the p-value is a calibrated scale for the statistic, not a proof of convergence.

    python examples/stein_goodness_of_fit/main.py --time [--shapes 4096x256x255,...] [--reps 5] [--no-torch]

measures the quadratic forms alone on synthetic particles (device events around the call, median of --reps after a warm-up,
the engines alternated in one process): stein_ksd_boot with B + 1 rows of weights, the same forms written in torch on the
device (U from matmuls, then U @ W.T: n x n images) where its memory fits, and the plain streaming step with the statistic
at the same shape as the unit of cost; peak device memory of each.
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
from stein_amd.engine import SvgdEngine  # noqa: E402
from stein_amd.utilities import ksd_quadratic_forms  # noqa: E402
from stein_amd.utilities.stein_test import sign_processes  # noqa: E402

DEFAULT_SHAPES = "4096x256x255,16384x256x255,8192x2001x255,65536x256x255,16384x256x1023"


def thinning_example():
    spec = importlib.util.spec_from_file_location("thinning_main", os.path.join(HERE, "..", "stein_thinning", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_example(args):
    ex = thinning_example()
    gen = torch.Generator(device="cuda").manual_seed(1)
    for iters in (args.early, args.iters):
        sampler, full = ex.run_sampler(argparse.Namespace(particles=args.particles, iters=iters, batch=args.batch))
        stat, p, reps = sampler.goodness_of_fit(full, n_boot=args.boot, generator=gen, return_samples=True)
        q = torch.quantile(reps, torch.tensor([0.5, 0.95], dtype=reps.dtype, device=reps.device)).tolist()
        print("%d particles after %4d steps: KSD^2_V (IMQ, median bandwidth) = %.4e; bootstrap median %.4e, 95 %% %.4e; "
              "p = %.4f (%d replicates)" % (args.particles, iters, stat, q[0], q[1], p, args.boot))


def torch_forms(X, G, W, h2, kernel="imq"):
    """the same quadratic forms in torch on the device: the n x n Stein-kernel matrix from matmuls, then U @ W.T"""
    d = X.shape[1]
    c2 = 2.0 * h2
    r, a = (X * X).sum(1), (G * X).sum(1)
    XX = X @ X.T
    D = (r[:, None] + r[None, :] - 2.0 * XX).clamp_min_(0.0)
    del XX
    cross = a[:, None] + a[None, :] - G @ X.T - X @ G.T
    gg = G @ G.T
    if kernel == "imq":
        k = torch.rsqrt(1.0 + D / c2)
        k3 = k * k * k
        U = k * gg + k3 * (cross / c2 + d / c2 - 3.0 * k * k * D / (c2 * c2))
    else:
        U = torch.exp(-D / c2) * (gg + cross / h2 + d / h2 - D / (h2 * h2))
    del D, cross, gg
    return ((U @ W.T).double() * W.T.double()).sum(0)


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
    return out


def time_shapes(args):
    dev = torch.device("cuda")
    print("quadratic forms alone, IMQ kernel, fixed bandwidth h2 = d; %d timed repeats after one warm-up, engines alternated"
          % args.reps)
    for spec in args.shapes.split(","):
        n, d, boot = (int(x) for x in spec.split("x"))
        gen = torch.Generator(device=dev).manual_seed(n + d)
        X = torch.randn(n, d, device=dev, generator=gen).contiguous()
        G = -X
        h2 = float(d)
        h2_t = torch.full((1,), h2, dtype=torch.float32, device=dev)
        W = torch.cat([torch.ones(1, n, device=dev), sign_processes(boot, n, 0.5, dev, gen)]).contiguous()
        eng = SvgdEngine(n, d, device=dev, h2=h2, kernel="imq")
        got, ref = [], []

        def ours():
            got[:] = [ksd_quadratic_forms(X, G, W, bandwidth=h2_t, kernel="imq")[0]]

        def step():
            eng.stream_discrepancy_sums(X, G)

        def theirs():
            ref[:] = [torch_forms(X, G, W, h2)]
        engines = [("boot", ours), ("step", step)]
        fits = not args.no_torch
        if fits:
            try:
                theirs()
                torch.cuda.synchronize()
                engines.append(("torch", theirs))
            except torch.OutOfMemoryError as e:
                fits = False
                ref[:] = []
                torch.cuda.empty_cache()
                oom = str(e).split(".")[0]
        times = {name: [] for name, _ in engines}
        peak = {}
        for name, fn in engines:      # warm-up and peak memory, one engine at a time
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        for _ in range(args.reps):    # alternated
            for name, fn in engines:
                times[name] += _ms(fn, 1)
        med = {k: float(np.median(v)) for k, v in times.items()}
        line = "%6d x %4d, %4d replicates: boot %8.3f ms (min %.3f max %.3f), workspace %.1f MiB, peak %.1f MiB; " \
               "streaming KSD step %.3f ms: %.2f steps" % (
                   n, d, boot, med["boot"], min(times["boot"]), max(times["boot"]),
                   _lib.ksd_boot_workspace_bytes(n, d, boot + 1) / 2 ** 20, peak["boot"] / 2 ** 20, med["step"],
                   med["boot"] / med["step"])
        if fits:
            rel = float(((ref[0] - got[0]).abs() / got[0].abs().clamp_min(1e-300)).max())
            line += " | torch %8.3f ms (min %.3f max %.3f), peak %.1f MiB: %.2fx; largest relative difference %.2e" % (
                med["torch"], min(times["torch"]), max(times["torch"]), peak["torch"] / 2 ** 20, med["torch"] / med["boot"], rel)
        elif not args.no_torch:
            line += " | torch: does not fit (%s)" % oom
        print(line, flush=True)
        del eng, X, G, W
        got[:], ref[:] = [], []
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--early", type=int, default=10)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--boot", type=int, default=511)
    ap.add_argument("--time", action="store_true", help="measure the quadratic forms on synthetic particles instead")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated n x d x replicates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU")
    if args.time:
        time_shapes(args)
    else:
        run_example(args)


if __name__ == "__main__":
    main()
