"""A/B of the network-classifier calls (stein_score_bnn_class, stein_predict_bnn_class: BnnClassScore / BnnClassPredict) against
the torch routes on the same device and against their FMA floors, by the protocol of scratch/softmax_ab.py: the routes of a
shape alternated block by block, every block's time printed.  Prints, and writes netclass_ab.txt into --out (default: the
working directory).

    python scratch/netclass_ab.py [--out DIR]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stein_amd.predict import BnnClassPredict  # noqa: E402
from stein_amd.scores import BnnClassScore  # noqa: E402

OUT = []
PEAK = 157.3e12      # fp32 vector peak, flops


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def blocks(fns, calls, nblocks=5, warm=3):
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
    say("  %-52s median %9.4f ms   per block %s%s" % (name, float(np.median(res)), ["%.4f" % r for r in res], extra))
    return float(np.median(res))


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def inputs(F, H, C, B, n, dev):
    """-> theta [n, d] with the blocks in the order w1, b1, w2, b2, log_lambda; X; y; cols"""
    g = torch.Generator(device=dev).manual_seed(0)
    sizes = (F * H, H, H * C, C, 1)
    cols = [int(c) for c in np.cumsum((0,) + sizes[:-1])]
    theta = torch.randn(n, sum(sizes), device=dev, generator=g)
    theta[:, cols[0]:cols[1]] /= F ** 0.5
    theta[:, cols[2]:cols[3]] /= H ** 0.5
    theta[:, cols[4]] *= 0.3
    X = torch.randn(B, F, device=dev, generator=g)
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    return theta.contiguous(), X.contiguous(), y, cols


def parts(t, F, H, C, cols):
    n = t.shape[0]
    return (t[:, cols[0]:cols[1]].reshape(n, F, H), t[:, cols[1]:cols[2]], t[:, cols[2]:cols[3]].reshape(n, H, C), t[:, cols[3]:cols[4]],
            t[:, cols[4]])


def score_shape(F, H, C, B, n, dev, calls):
    theta, X, y, cols = inputs(F, H, C, B, n, dev)
    scale = 10.0
    prod = BnnClassScore(F, H, C, cols, n_train=scale * B)
    feed = {"X": X, "y": y.to(torch.int32)}
    out = torch.empty_like(theta)
    rows = torch.arange(B, device=dev)
    onehot = torch.nn.functional.one_hot(y, C).to(theta.dtype)
    P = cols[4]

    def log_p(t):
        w1, b1, w2, b2, ll = parts(t, F, H, C, cols)
        hid = torch.relu(torch.matmul(X, w1) + b1[:, None, :])
        lp = torch.log_softmax(torch.baddbmm(b2[:, None, :], hid, w2), -1)[:, rows, y].sum(-1)
        lam = ll.exp()
        return scale * lp + (0.5 * ll[:, None] - 0.5 * lam[:, None] * t[:, :P] ** 2).sum(-1) - 0.01 * lam

    def autograd():
        t = theta.detach().clone().requires_grad_(True)
        (g,) = torch.autograd.grad(log_p(t).sum(), t)
        return g

    def closed(t=theta, oh=onehot, Xr=X):
        w1, b1, w2, b2, ll = parts(t, F, H, C, cols)
        m = t.shape[0]
        pre = torch.matmul(Xr, w1) + b1[:, None, :]
        a = torch.relu(pre)
        r = oh - torch.softmax(torch.baddbmm(b2[:, None, :], a, w2), -1)          # [n, B, C]
        dl = torch.bmm(r, w2.transpose(1, 2)) * (pre > 0)                          # [n, B, H]
        lam = ll.exp()
        g = torch.empty_like(t)
        g[:, cols[0]:cols[1]] = torch.matmul(Xr.T, dl).reshape(m, F * H)
        g[:, cols[1]:cols[2]] = dl.sum(1)
        g[:, cols[2]:cols[3]] = torch.bmm(a.transpose(1, 2), r).reshape(m, H * C)
        g[:, cols[3]:cols[4]] = r.sum(1)
        g[:, :P] = scale * g[:, :P] - lam[:, None] * t[:, :P]
        g[:, P] = 0.5 * P - lam * (0.5 * (t[:, :P] ** 2).sum(-1) + 0.01)
        return g
    m = min(n, 256)     # the fp64 yardstick on the first particles
    ref = closed(theta[:m].double(), onehot.double(), X.double())
    errs = ["%s %.2e" % (k, float((f()[:m].double() - ref).abs().max() / ref.abs().max()))
            for k, f in (("this", lambda: prod(theta, feed, out=out)), ("autograd", autograd), ("closed fp32", closed))]
    del ref
    floor = 2.0 * n * B * (2 * F * H + 3 * H * C) / PEAK * 1e3
    say("%d x %d x %d, batch %d, n %d (d %d)   max |. - fp64| / max|fp64|: %s" % (F, H, C, B, n, P + 1, ", ".join(errs)))
    ra, rb, rc = blocks([lambda: prod(theta, feed, out=out), autograd, closed], calls)
    a = line("this: BnnClassScore (stein_score_bnn_class)", ra, "   peak %.1f MB" % peak(lambda: prod(theta, feed, out=out)))
    b = line("torch: autograd of the batched log posterior", rb, "   peak %.1f MB" % peak(autograd))
    c = line("torch: closed form, matmul / bmm", rc, "   peak %.1f MB" % peak(closed))
    say("  this / autograd x %.3f   this / closed form x %.3f   FMA floor %.4f ms: this x %.1f" % (a / b, a / c, floor, a / floor))


def predict_shape(F, H, C, B, n, dev, calls):
    theta, X, y, cols = inputs(F, H, C, B, n, dev)
    prod = BnnClassPredict(F, H, C, cols)
    feed = {"X": X, "y": y}
    rows = torch.arange(B, device=dev)

    def logits():
        w1, b1, w2, b2, _ = parts(theta, F, H, C, cols)
        return torch.baddbmm(b2[:, None, :], torch.relu(torch.matmul(X, w1) + b1[:, None, :]), w2)    # [n, B, C]

    def torch_route():
        z = logits()
        p = torch.softmax(z, -1)
        prob = p.mean(0)
        lpd = p[:, rows, y].mean(0).log()
        ent = (torch.logsumexp(z, -1) - (p * z).sum(-1)).mean(0)
        return prob, prob.argmax(-1), ent, lpd

    def torch_mean_only():
        return torch.softmax(logits(), -1).mean(0)
    s = prod.summary(theta, feed)
    t = torch_route()
    say("%d x %d x %d, %d rows, n %d   max |this - torch|: prob %.2e  ent %.2e  lpd %.2e  labels differing %d"
        % (F, H, C, B, n, float((s["prob"] - t[0]).abs().max()), float((s["ent"] - t[2]).abs().max()),
           float((s["lpd"] - t[3]).abs().max()), int((s["label"].long() != t[1]).sum())))
    del t
    floor = 2.0 * n * B * (F * H + H * C) / PEAK * 1e3
    out = torch.empty(n, B, C, device=dev)
    ra, rp, rb, rc = blocks([lambda: prod.summary(theta, feed), lambda: prod(theta, feed, out=out), torch_route, torch_mean_only], calls)
    del out
    a = line("this: BnnClassPredict.summary (prob, label, ent, lpd)", ra,
             "   peak %.1f MB (+ workspace %.1f MB, held by the producer)" % (peak(lambda: prod.summary(theta, feed)), prod._ws.numel() / 1e6))
    line("this: BnnClassPredict.__call__ ([n, rows, C])", rp)
    b = line("torch: forward + softmax + mean, entropy, lpd", rb, "   peak %.1f MB" % peak(torch_route))
    c = line("torch: forward + softmax + mean alone", rc, "   peak %.1f MB" % peak(torch_mean_only))
    say("  this / torch x %.3f   this / torch mean alone x %.3f   FMA floor %.4f ms: this x %.1f" % (a / b, a / c, floor, a / floor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say("device: %s" % torch.cuda.get_device_name(0))
    say("== score: stein_score_bnn_class against the torch routes and the FMA floor (2 n batch (2 F H + 3 H C) flops at 157.3 TFLOPS)")
    for F, H, C, B, n, calls in ((54, 100, 7, 100, 100, 30), (54, 100, 7, 100, 1024, 20), (54, 100, 7, 100, 16384, 3),
                                 (13, 50, 3, 100, 16384, 5), (128, 64, 32, 1000, 1024, 3), (3, 20, 3, 100, 100, 30)):
        score_shape(F, H, C, B, n, dev, calls)
        torch.cuda.empty_cache()
    say("== summaries: stein_predict_bnn_class against the torch route and the FMA floor (2 n rows (F H + H C) flops)")
    for F, H, C, B, n, calls in ((54, 100, 7, 4000, 1024, 5), (54, 100, 7, 4000, 16384, 2), (13, 50, 3, 200, 16384, 5),
                                 (3, 20, 3, 500, 100, 30)):
        predict_shape(F, H, C, B, n, dev, calls)
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "netclass_ab.txt"), "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
