"""A/B of the predictive producers (stein_amd/predict.py) against the torch route they replace: the example's torch callable
on the device followed by mean, var and logsumexp in torch on the device (profiles/predict_ab.txt).  Device events around
blocks of calls, variants alternated block by block.  The host copy of [n, batch] that function_posterior adds to the torch
route is timed on its own line.

    python scratch/predict_ab.py [--out FILE]
    python scratch/predict_ab.py --trace logistic|network      60 summary-only calls at the large shape and nothing else,
                                                               for a profiler run of its own
"""
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stein_amd.predict import BnnPredict, GlmPredict  # noqa: E402

OUT_FILE = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def ab(variants, warm, blocks, steps):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            res[k].append(timed(fn, steps))
    return res


def report(tag, res):
    say(tag)
    for k, v in res.items():
        say("  %-38s median %.4f ms   per block %s" % (k, statistics.median(v), ["%.4f" % x for x in v]))


def host_copy_ms(t, reps=3):
    """wall time of the device -> host copy of the [n, batch] matrix, as function_posterior makes it (.cpu().numpy())"""
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        t.cpu().numpy()
        best.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(best)


def logistic_inputs(n, feats, B):
    gen = torch.Generator(device="cpu").manual_seed(0)
    theta = (torch.randn(n, feats + 1, generator=gen) * 0.3).to(dev)          # log_alpha, then the weights
    X = torch.randn(B, feats, generator=gen).to(dev)
    y = (torch.rand(B, generator=gen) < 0.5).float().to(dev)
    return theta, {"X": X, "y": y}


def logistic_case(n, feats, B, blocks=5, steps=20, note=""):
    theta, feed = logistic_inputs(n, feats, B)
    prod = GlmPredict("logistic", feats, w_col=1)
    keep = {}

    def torch_route():
        w = theta[:, 1:]
        logits = (feed["X"] @ w.T).T                                           # the example's callable: [n, B]
        ll = -F.binary_cross_entropy_with_logits(logits, feed["y"][None, :].expand_as(logits), reduction="none")
        keep["t"] = (logits, logits.mean(0), logits.var(0, unbiased=False), torch.logsumexp(ll, 0) - math.log(n))

    def torch_pred_only():
        keep["tp"] = (feed["X"] @ theta[:, 1:].T).T              # as the example writes it: a transposed view, no copy
    out = torch.empty(n, B, device=dev)

    def both():
        prod(theta, feed, out=out)
        keep["s2"] = prod.summary(theta, feed)
    variants = {"torch: callable + mean/var/logsumexp": torch_route, "torch: callable only": torch_pred_only,
                "this: summary only": lambda: keep.__setitem__("s", prod.summary(theta, feed)),
                "this: pred only": lambda: prod(theta, feed, out=out), "this: pred, then summary": both}
    res = ab(variants, 5, blocks, steps)
    torch.cuda.synchronize()
    t, s = keep["t"], keep["s"]
    errs = [float((a - b).abs().max()) for a, b in ((out, t[0]), (s[0], t[1]), (s[1], t[2]), (s[2], t[3]))]
    report("logistic %d particles x %d features x %d rows%s, %d x %d calls; max |this - torch| pred %.2e mean %.2e var %.2e lpd %.2e"
           % (n, feats, B, note, blocks, steps, *errs), res)
    say("  host copy of [n, batch] (%.0f MB), which function_posterior adds to the torch route: %.2f ms"
        % (n * B * 4 / 1e6, host_copy_ms(t[0])))
    return res


def network_inputs(n, H, B):
    gen = torch.Generator(device="cpu").manual_seed(0)
    d = 3 * H + 3
    theta = torch.randn(n, d, generator=gen).to(dev)
    # packed by sorted name: b_1 [H], b_2, log_gamma, log_lambda, w_1 [1][H], w_2 [H]
    cols = (H + 3, 0, 2 * H + 3, H, H + 2, H + 1)
    X = torch.rand(B, 1, generator=gen).to(dev)
    y = torch.randn(B, generator=gen).to(dev)
    return theta, cols, {"X": X, "y": y}


def network_case(n, H, B, blocks=5, steps=20):
    theta, cols, feed = network_inputs(n, H, B)
    prod = BnnPredict(1, H, cols)
    keep = {}
    b1, b2, lg, w1, w2 = theta[:, :H], theta[:, H], theta[:, H + 1], theta[:, H + 3:2 * H + 3].reshape(n, 1, H), theta[:, 2 * H + 3:]

    def callable_():
        hidden = torch.relu(torch.einsum("pf,nfh->nph", feed["X"], w1) + b1[:, None, :])   # the example's predict()
        return torch.einsum("nph,nh->np", hidden, w2) + b2[:, None]

    def torch_route():
        pred = callable_()
        ll = 0.5 * lg[:, None] - 0.5 * lg.exp()[:, None] * (pred - feed["y"][None, :]) ** 2 - 0.5 * math.log(2 * math.pi)
        keep["t"] = (pred, pred.mean(0), pred.var(0, unbiased=False), torch.logsumexp(ll, 0) - math.log(n))
    out = torch.empty(n, B, device=dev)

    def both():
        prod(theta, feed, out=out)
        keep["s2"] = prod.summary(theta, feed)
    variants = {"torch: callable + mean/var/logsumexp": torch_route, "torch: callable only": lambda: keep.__setitem__("tp", callable_()),
                "this: summary only": lambda: keep.__setitem__("s", prod.summary(theta, feed)),
                "this: pred only": lambda: prod(theta, feed, out=out), "this: pred, then summary": both}
    res = ab(variants, 5, blocks, steps)
    torch.cuda.synchronize()
    t, s = keep["t"], keep["s"]
    errs = [float((a - b).abs().max()) for a, b in ((out, t[0]), (s[0], t[1]), (s[1], t[2]), (s[2], t[3]))]
    report("network %d particles x %d hidden x %d rows, %d x %d calls; max |this - torch| pred %.2e mean %.2e var %.2e lpd %.2e"
           % (n, H, B, blocks, steps, *errs), res)
    say("  host copy of [n, batch] (%.1f MB), which function_posterior adds to the torch route: %.2f ms"
        % (n * B * 4 / 1e6, host_copy_ms(t[0])))
    return res


if __name__ == "__main__":
    if "--trace" in sys.argv:
        which = sys.argv[sys.argv.index("--trace") + 1]
        if which == "logistic":
            theta, feed = logistic_inputs(16384, 54, 4000)
            prod = GlmPredict("logistic", 54, w_col=1)
        else:
            theta, cols, feed = network_inputs(8192, 666, 200)
            prod = BnnPredict(1, 666, cols)
        for _ in range(60):
            prod.summary(theta, feed)
        torch.cuda.synchronize()
        sys.exit(0)
    logistic_case(16384, 54, 4000)
    network_case(8192, 666, 200)
    logistic_case(100, 54, 4000, steps=50)
    network_case(20, 100, 20, steps=50)
    # not one of the examples' shapes: the GLM kernel's chunked arm (more than 58 features: the X tile is staged again from
    # global memory in every pass of 16 particles)
    logistic_case(16384, 200, 4000, note=" (chunked arm)")
    if OUT_FILE:
        with open(OUT_FILE, "w") as f:
            f.write("\n".join(lines) + "\n")
