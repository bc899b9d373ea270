"""A/B of the weighted class summaries (stein_predict_softmax_weighted, stein_predict_bnn_class_weighted:
SoftmaxPredict / BnnClassPredict.weighted_summary) by the protocol of scratch/netclass_ab.py: the routes of a shape alternated
block by block, five blocks, every block's time printed.  Per shape:
  1. the unweighted call of this tree against the parent commit's library (--parent PATH to its libsteinhip.so, loaded side by
     side): bit identity of prob, lpd, ent and label, and time;
  2. weighted with positive weights against unweighted, both from this tree (the weight pass is two more launches);
  3. weighted with thinning counts (n / 16 picks with replacement, no pred) against positive weights, beside the share of dead
     particles and staging units;
  4. the torch route: forward, softmax, einsum('p,pbc->bc'), weighted entropy, logsumexp with log w; time and peak memory.
Prints, and writes class_weighted_ab.txt into --out (default: the working directory).

    python scratch/class_weighted_ab.py [--parent PATH/libsteinhip.so] [--out DIR]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stein_amd import _lib  # noqa: E402
from stein_amd.predict import BnnClassPredict, SoftmaxPredict  # noqa: E402
import class_weighted_cases as cwc  # noqa: E402  (the Python mirror of the staging units)

OUT = []


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
    say("  %-58s median %9.4f ms   per block %s%s" % (name, float(np.median(res)), ["%.4f" % r for r in res], extra))
    return float(np.median(res))


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def load_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("stein_predict_softmax", "stein_predict_bnn_class"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib._SIGNATURES[name], ctypes.c_int
    return lib


class Shape:
    """one model shape: inputs, the producer, a raw unweighted call for either library, and the torch route"""

    def __init__(self, model, F, H, C, B, n, dev):
        self.model, self.F, self.H, self.C, self.B, self.n = model, F, H, C, B, n
        g = torch.Generator(device=dev).manual_seed(0)
        if model == "softmax":
            self.cols, d = None, F * C
            theta = torch.randn(n, d, device=dev, generator=g) * (2.0 / F ** 0.5)
            self.prod = SoftmaxPredict(F, C)
        else:
            sizes = (F * H, H, H * C, C)
            self.cols = [int(c) for c in np.cumsum((0,) + sizes[:-1])]
            d = sum(sizes)
            theta = torch.randn(n, d, device=dev, generator=g)
            theta[:, :self.cols[1]] /= F ** 0.5
            theta[:, self.cols[2]:self.cols[3]] /= H ** 0.5
            self.prod = BnnClassPredict(F, H, C, self.cols)
        self.theta, self.d = theta.contiguous(), d
        self.X = torch.randn(B, F, device=dev, generator=g).contiguous()
        self.y = torch.randint(0, C, (B,), device=dev, generator=g)
        self.y32 = self.y.to(torch.int32)
        self.feed = {"X": self.X, "y": self.y}
        self.rows = torch.arange(B, device=dev)
        self.name = ("softmax %d x %d" % (F, C)) if model == "softmax" else ("network %d x %d x %d" % (F, H, C))

    def raw(self, lib):
        """-> (call, outputs) of the unweighted C entry point of `lib` on preallocated outputs and workspace"""
        dev, n, B, C = self.theta.device, self.n, self.B, self.C
        out = {"prob": torch.empty(B, C, device=dev), "lpd": torch.empty(B, device=dev), "ent": torch.empty(B, device=dev),
               "label": torch.empty(B, dtype=torch.int32, device=dev)}
        stem = "softmax" if self.model == "softmax" else "bnn_class"
        ws = torch.empty(getattr(_lib, "predict_%s_workspace_bytes" % stem)(n, B, C), dtype=torch.uint8, device=dev)
        margs = (0, self.F, C) if self.model == "softmax" else (self.F, self.H, C, (ctypes.c_int64 * 5)(*(self.cols + [-1])))
        fn = getattr(lib, "stein_predict_" + stem)
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (self.theta.data_ptr(), n, self.d, _lib.PRED_MEAN) + margs + (self.X.data_ptr(), self.y32.data_ptr(), B, None,
                out["prob"].data_ptr(), out["lpd"].data_ptr(), out["ent"].data_ptr(), out["label"].data_ptr(), ws.data_ptr(),
                ws.numel(), stream)

        def call():
            rc = fn(*args)
            assert rc == 0, rc
        return call, out, ws

    def logits(self):
        if self.model == "softmax":
            return torch.matmul(self.X, self.theta.reshape(self.n, self.F, self.C))
        c, t, n = self.cols, self.theta, self.n
        w1, b1 = t[:, :c[1]].reshape(n, self.F, self.H), t[:, c[1]:c[2]]
        w2, b2 = t[:, c[2]:c[3]].reshape(n, self.H, self.C), t[:, c[3]:]
        return torch.baddbmm(b2[:, None, :], torch.relu(torch.matmul(self.X, w1) + b1[:, None, :]), w2)    # [n, B, C]

    def torch_route(self, w):
        v = (w / w.sum()).float()
        z = self.logits()
        p = torch.softmax(z, -1)
        prob = torch.einsum("p,pbc->bc", v, p)
        ent = torch.einsum("p,pb->b", v, torch.logsumexp(z, -1) - (p * z).sum(-1))
        logp_y = torch.log_softmax(z, -1)[:, self.rows, self.y]
        lpd = torch.logsumexp(logp_y + v.log()[:, None], 0)
        return prob, prob.argmax(-1), ent, lpd


def dead_share(sh, w):
    """-> (share of particles with lane weight zero, share of dead staging units) of a call without pred"""
    case = {"F": sh.F, "H": sh.H, "C": sh.C, "B": sh.B, "n": sh.n}
    w = w.cpu().numpy()
    rows = cwc.units(sh.model, case, w)
    total = sum(len(r) for r in rows)
    dead = sum(1 for r in rows for u in r if not u[2])
    return float((cwc.cwr.lane_weights(w) == 0).mean()), dead / total


def shape(model, F, H, C, B, n, dev, calls, parent):
    sh = Shape(model, F, H, C, B, n, dev)
    prod, th, feed = sh.prod, sh.theta, sh.feed
    g = torch.Generator(device=dev).manual_seed(1)
    positive = torch.rand(n, device=dev, generator=g, dtype=torch.float64) + 0.05
    picks = torch.randint(0, n, (max(n // 16, 1),), device=dev, generator=g)
    counts = torch.bincount(picks, minlength=n).double()
    say("%s, %d rows, n %d" % (sh.name, B, n))
    # 1. against the parent library
    this_call, this_out, _ = sh.raw(_lib.load())
    if parent is not None:
        par_call, par_out, par_ws = sh.raw(parent)
        par_ws.fill_(255)
        this_call()
        par_call()
        torch.cuda.synchronize()
        same = all(torch.equal(this_out[k].view(torch.int32), par_out[k].view(torch.int32)) for k in this_out)
        rp, rt = blocks([par_call, this_call], calls)
        a = line("1. parent library: stein_predict_* (raw call)", rp)
        b = line("   this tree:      stein_predict_* (raw call)", rt)
        inside = min(rp) <= b <= max(rp)
        say("   bit-identical outputs: %s   this / parent x %.3f   parent's blocks span [%.4f, %.4f] ms: this tree's median %s"
            % (same, b / a, min(rp), max(rp), "inside" if inside else "OUTSIDE by %.4f ms" % (b - max(rp) if b > max(rp) else b - min(rp))))
    # 2. the weights' cost, 3. the dead-unit skip, 4. torch
    s = prod.weighted_summary(th, feed, positive)
    t = sh.torch_route(positive)
    say("   max |this - torch| under positive weights: prob %.2e  ent %.2e  lpd %.2e  labels differing %d"
        % (float((s["prob"] - t[0]).abs().max()), float((s["ent"] - t[2]).abs().max()), float((s["lpd"] - t[3]).abs().max()),
           int((s["label"].long() != t[1]).sum())))
    del t
    ru, rw, rc, rtor = blocks([lambda: prod.summary(th, feed), lambda: prod.weighted_summary(th, feed, positive),
                               lambda: prod.weighted_summary(th, feed, counts), lambda: sh.torch_route(positive)], calls)
    u = line("2. this: summary (unweighted)", ru)
    w = line("   this: weighted_summary, positive weights", rw,
             "   peak %.1f MB (+ workspace %.1f MB, held by the producer)" % (peak(lambda: prod.weighted_summary(th, feed, positive)),
                                                                              prod._wws.numel() / 1e6))
    say("   weighted / unweighted x %.3f (+ %.4f ms)" % (w / u, w - u))
    c = line("3. this: weighted_summary, thinning counts (n / 16 picks)", rc)
    dp, du = dead_share(sh, counts)
    say("   counts / positive x %.3f   dead particles %.1f %%, dead staging units %.1f %%: live share %.3f (particles) %.3f (units)"
        % (c / w, 100 * dp, 100 * du, 1 - dp, 1 - du))
    tr = line("4. torch: forward, softmax, einsum, entropy, logsumexp", rtor, "   peak %.1f MB" % peak(lambda: sh.torch_route(positive)))
    say("   this (positive) / torch x %.3f   this (counts) / torch x %.3f%s" % (w / tr, c / tr, "   **the call loses**" if w > tr else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--parent", default=None, help="the parent commit's libsteinhip.so")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say("device: %s" % torch.cuda.get_device_name(0))
    parent = load_parent(args.parent) if args.parent else None
    if parent is None:
        say("(no --parent: part 1 is left out)")
    for model, F, H, C, B, n, calls in (("softmax", 54, 0, 7, 4000, 1024, 10), ("softmax", 54, 0, 7, 4000, 16384, 3),
                                        ("softmax", 784, 0, 10, 1000, 1024, 5), ("netclass", 54, 100, 7, 4000, 1024, 5),
                                        ("netclass", 13, 50, 3, 200, 16384, 5), ("netclass", 3, 20, 3, 500, 100, 30)):
        shape(model, F, H, C, B, n, dev, calls, parent)
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "class_weighted_ab.txt"), "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
