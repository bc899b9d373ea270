"""A/B of the softmax-regression calls (stein_score_softmax, stein_predict_softmax: SoftmaxScore / SoftmaxPredict) against the
torch routes on the same device and against their FMA floors.  Prints, and writes softmax_ab.txt into --out (default: the
working directory).

    python scratch/softmax_ab.py [--out DIR]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stein_amd import _lib  # noqa: E402
from stein_amd.predict import SoftmaxPredict  # noqa: E402
from stein_amd.scores import SoftmaxScore  # noqa: E402

OUT = []
PEAK = 157.3e12      # fp32 vector peak, flops


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def blocks(fns, calls, nblocks=5, warm=5):
    """the routes `fns` alternated block by block (the first one first in every round) -> one list of ms per call each"""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = [[] for _ in fns]
    for _ in range(nblocks):
        for fn, r in zip(fns, res):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            r.append(e0.elapsed_time(e1) / calls)
    return res


def line(name, res, extra=""):
    say("  %-52s median %8.4f ms   per block %s%s" % (name, float(np.median(res)), ["%.4f" % r for r in res], extra))
    return float(np.median(res))


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def inputs(F, C, B, n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    theta = torch.randn(n, F * C + 1, device=dev, generator=g) * (1.0 / F ** 0.5)
    X = torch.rand(B, F, device=dev, generator=g)
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    return theta.contiguous(), X.contiguous(), y


def score_shape(F, C, B, n, dev, calls):
    theta, X, y = inputs(F, C, B, n, dev)
    scale = 10.0
    prod = SoftmaxScore(F, C, w_col=0, alpha_col=F * C, n_train=scale * B)
    feed = {"X": X, "y": y.to(torch.int32)}
    out = torch.empty_like(theta)
    rows = torch.arange(B, device=dev)
    onehot = torch.nn.functional.one_hot(y, C).float()

    def log_p(t):
        W, la = t[:, :F * C].reshape(n, F, C), t[:, F * C]
        lp = torch.log_softmax(torch.einsum("bf,nfc->nbc", X, W), -1)[:, rows, y].sum(-1)
        a = la.exp()
        return scale * lp + (0.5 * la[:, None] - 0.5 * a[:, None] * t[:, :F * C] ** 2).sum(-1) - 0.01 * a

    def autograd():
        t = theta.detach().clone().requires_grad_(True)
        (g,) = torch.autograd.grad(log_p(t).sum(), t)
        return g

    def closed():
        W = theta[:, :F * C].reshape(n, F, C)
        r = onehot - torch.softmax(torch.einsum("bf,nfc->nbc", X, W), -1)
        a = theta[:, F * C].exp()
        g = torch.empty_like(theta)
        g[:, :F * C] = scale * torch.einsum("bf,nbc->nfc", X, r).reshape(n, F * C) - a[:, None] * theta[:, :F * C]
        g[:, F * C] = 0.5 * F * C - a * (0.5 * (theta[:, :F * C] ** 2).sum(-1) + 0.01)
        return g
    t64, X64 = theta.double(), X.double()
    W64 = t64[:, :F * C].reshape(n, F, C)
    r64 = onehot.double() - torch.softmax(torch.einsum("bf,nfc->nbc", X64, W64), -1)
    ref = scale * torch.einsum("bf,nbc->nfc", X64, r64).reshape(n, F * C) - t64[:, F * C].exp()[:, None] * t64[:, :F * C]
    del r64
    errs = ["%s %.2e" % (k, float((f()[:, :F * C].double() - ref).abs().max() / ref.abs().max()))
            for k, f in (("this", lambda: prod(theta, feed, out=out)), ("autograd", autograd), ("einsum fp32", closed))]
    floor = 4.0 * n * B * F * C / PEAK * 1e3
    say("%d x %d, batch %d, n %d (d %d)   max |. - fp64| / max|fp64|: %s" % (F, C, B, n, F * C + 1, ", ".join(errs)))
    ra, rb, rc = blocks([lambda: prod(theta, feed, out=out), autograd, closed], calls)
    a = line("this: SoftmaxScore (stein_score_softmax)", ra, "   peak %.1f MB" % peak(lambda: prod(theta, feed, out=out)))
    b = line("torch: autograd of the batched log posterior", rb, "   peak %.1f MB" % peak(autograd))
    c = line("torch: closed form, einsum", rc, "   peak %.1f MB" % peak(closed))
    say("  this / autograd x %.3f   this / einsum x %.3f   FMA floor %.4f ms: this x %.1f" % (a / b, a / c, floor, a / floor))
    return a, b, c, floor


def lanes_shape(F, C, B, n, dev, calls):
    """the forward phase's feature split: the rule's lanes per row against one lane per row (the starting design), same call"""
    theta, X, y = inputs(F, C, B, n, dev)
    prod = SoftmaxScore(F, C, w_col=0, alpha_col=F * C, n_train=10.0 * B)
    feed = {"X": X, "y": y.to(torch.int32)}
    out = torch.empty_like(theta)

    def with_lanes(g):
        def run():
            _lib.debug_score_softmax_lanes(g)
            prod(theta, feed, out=out)
            _lib.debug_score_softmax_lanes(0)
        return run
    ref = with_lanes(0)
    ref()
    base = out.clone()
    with_lanes(1)()
    diff = float((out - base).abs().max() / base.abs().max())
    rule, one = blocks([with_lanes(0), with_lanes(1)], calls)
    say("%d x %d, batch %d, n %d   max |one lane - rule| / max %.2e" % (F, C, B, n, diff))
    a = line("the rule's lanes per row", rule)
    b = line("one lane per row (G = 1)", one)
    say("  rule / one lane x %.3f" % (a / b))


def predict_shape(F, C, B, n, dev, calls):
    theta, X, y = inputs(F, C, B, n, dev)
    prod = SoftmaxPredict(F, C)
    feed = {"X": X, "y": y}
    rows = torch.arange(B, device=dev)

    def torch_route():
        W = theta[:, :F * C].reshape(n, F, C)
        z = torch.matmul(X, W)                                  # [n, B, C]: the bmm forward pass
        p = torch.softmax(z, -1)
        prob = p.mean(0)
        lpd = p[:, rows, y].mean(0).log()
        ent = (torch.logsumexp(z, -1) - (p * z).sum(-1)).mean(0)
        return prob, prob.argmax(-1), ent, lpd

    def torch_mean_only():
        return torch.softmax(torch.matmul(X, theta[:, :F * C].reshape(n, F, C)), -1).mean(0)
    s = prod.summary(theta, feed)
    t = torch_route()
    say("%d x %d, %d rows, n %d   max |this - torch|: prob %.2e  ent %.2e  lpd %.2e  labels differing %d"
        % (F, C, B, n, float((s["prob"] - t[0]).abs().max()), float((s["ent"] - t[2]).abs().max()),
           float((s["lpd"] - t[3]).abs().max()), int((s["label"].long() != t[1]).sum())))
    floor = 2.0 * n * B * F * C / PEAK * 1e3
    out = torch.empty(n, B, C, device=dev)
    ra, rp, rb, rc = blocks([lambda: prod.summary(theta, feed), lambda: prod(theta, feed, out=out), torch_route, torch_mean_only], calls)
    del out
    a = line("this: SoftmaxPredict.summary (prob, label, ent, lpd)", ra,
             "   peak %.1f MB (+ workspace %.1f MB, held by the producer)" % (peak(lambda: prod.summary(theta, feed)), prod._ws.numel() / 1e6))
    p = line("this: SoftmaxPredict.__call__ ([n, rows, C])", rp)
    b = line("torch: bmm + softmax + mean, entropy, lpd", rb, "   peak %.1f MB" % peak(torch_route))
    c = line("torch: bmm + softmax + mean alone", rc, "   peak %.1f MB" % peak(torch_mean_only))
    say("  this / torch x %.3f   this / torch mean alone x %.3f   FMA floor %.4f ms: this x %.1f" % (a / b, a / c, floor, a / floor))
    return a, p, b, c, floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say("device: %s" % torch.cuda.get_device_name(0))
    say("== score: stein_score_softmax against the torch routes and the FMA floor (4 n batch F C flops at 157.3 TFLOPS)")
    for F, C, B, n, calls in ((54, 7, 100, 100, 50), (54, 7, 100, 1024, 50), (54, 7, 100, 16384, 10), (784, 10, 100, 1024, 10),
                              (16, 3, 1000, 16384, 10)):
        score_shape(F, C, B, n, dev, calls)
    say("== score: lanes per row of the forward phase, the rule against G = 1, alternated block by block")
    for F, C, B, n, calls in ((784, 10, 100, 1024, 10), (512, 32, 100, 1024, 10), (54, 7, 100, 16384, 10), (54, 7, 16, 16384, 10),
                              (54, 7, 4, 16384, 10), (16, 3, 8, 16384, 10), (784, 10, 8, 1024, 10)):
        lanes_shape(F, C, B, n, dev, calls)
    say("== summaries: stein_predict_softmax against the torch route and the FMA floor (2 n rows F C flops)")
    for F, C, B, n, calls in ((54, 7, 4000, 1024, 20), (54, 7, 4000, 16384, 5), (784, 10, 1000, 1024, 10)):
        predict_shape(F, C, B, n, dev, calls)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "softmax_ab.txt"), "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
