"""A/B of the weighted predictive summaries (stein_amd/predict.py, weighted_summary), by the protocol of
profiles/predict_ab.txt section 1: one process, variants alternated block by block, 5 warm-up calls, 5 blocks, device events.

    python scratch/predict_weighted_ab.py [--out FILE] [--parent PATH_OF_THE_PARENT_COMMITS_libsteinhip.so]

Per shape (the four example shapes and the GLM kernel's chunked arm) three comparisons:
  1. weighted summaries against this commit's unweighted summaries;
  2. weighted summaries against the torch route: the example's callable, then w @ f, a weighted variance and
     logsumexp(l + log w), all on the device;
  3. with --parent: the unweighted C calls of this commit against the same calls into the parent commit's library, loaded
     beside this one, alternated in the same session -- and bit-identity of pred / mean / var / lpd between the two.
"""
import ctypes
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ab as base  # noqa: E402  (inputs, timed, ab, report)
from stein_amd import _lib  # noqa: E402
from stein_amd.predict import BnnPredict, GlmPredict  # noqa: E402

OUT_FILE = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
PARENT = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
dev = base.dev
say = base.say


def load_parent():
    lib = ctypes.CDLL(PARENT)
    for name in ("stein_predict_glm", "stein_predict_bnn"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib._SIGNATURES[name], ctypes.c_int
    return lib


def raw_unweighted(lib, prod, theta, feed, n, B):
    """-> (call(), buffers): the unweighted C entry point of `lib` for all four outputs, on buffers of its own"""
    bufs = dict(pred=torch.empty(n, B, device=dev), mean=torch.empty(B, device=dev), var=torch.empty(B, device=dev),
                lpd=torch.empty(B, device=dev))
    ws = torch.empty(_lib.predict_workspace_bytes(n, B), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    d = theta.shape[1]
    out = [bufs[k].data_ptr() for k in ("pred", "mean", "var", "lpd")] + [ws.data_ptr(), ws.numel(), stream]
    if isinstance(prod, BnnPredict):
        args = [theta.data_ptr(), n, d, prod.n_in, prod.n_hidden, prod._cols, prod.output, feed["X"].data_ptr(), feed["y"].data_ptr(), B] + out
        fn = lib.stein_predict_bnn
    else:
        args = [theta.data_ptr(), n, d, prod.kind, prod.output, prod.w_col, prod.n_feats, feed["X"].data_ptr(), feed["y"].data_ptr(), B,
                prod.noise_precision] + out
        fn = lib.stein_predict_glm

    def call():
        rc = fn(*args)
        assert rc == 0, rc
    return call, bufs


def spread(v):
    return max(v) - min(v)


def case(tag, n, B, prod, theta, feed, outputs, loglik, parent, blocks=5, steps=20):
    gen = torch.Generator(device="cpu").manual_seed(1)
    w = torch.empty(n, dtype=torch.float64).exponential_(generator=gen).to(dev)
    logw = (w / w.sum()).log()
    keep = {}

    def torch_route():
        f = outputs()                                                          # [n, B], the example's callable
        wn = (w / w.sum()).float()
        mean = wn @ f
        var = wn @ (f - mean) ** 2
        keep["t"] = (mean, var, torch.logsumexp(loglik(f) + logw.float()[:, None], 0))
    variants = {"this: unweighted summary": lambda: keep.__setitem__("u", prod.summary(theta, feed)),
                "this: weighted summary": lambda: keep.__setitem__("w", prod.weighted_summary(theta, feed, w)),
                "torch: callable + weighted mean/var/logsumexp": torch_route}
    res = base.ab(variants, 5, blocks, steps)
    torch.cuda.synchronize()
    errs = [float((a - b).abs().max()) for a, b in zip(keep["w"][:3], keep["t"])]
    base.report("%s, %d x %d calls; max |weighted - torch| mean %.2e var %.2e lpd %.2e; ess %.1f of %d"
                % (tag, blocks, steps, *errs, float(keep["w"][3]), n), res)
    med = {k: statistics.median(v) for k, v in res.items()}
    say("  1. weighted / unweighted summary: %.3f" % (med["this: weighted summary"] / med["this: unweighted summary"]))
    say("  2. weighted summary / torch route: %.3f" % (med["this: weighted summary"] / med["torch: callable + weighted mean/var/logsumexp"]))
    if parent is not None:
        this_call, this_bufs = raw_unweighted(_lib.load(), prod, theta, feed, n, B)
        par_call, par_bufs = raw_unweighted(parent, prod, theta, feed, n, B)
        r3 = base.ab({"this commit: pred + mean + var + lpd (C call)": this_call, "parent commit: the same call": par_call}, 5, blocks, steps)
        torch.cuda.synchronize()
        same = all(torch.equal(this_bufs[k].view(torch.int32), par_bufs[k].view(torch.int32)) for k in this_bufs)
        base.report("  3. unweighted call, this commit against the parent commit's library", r3)
        a, b = (r3[k] for k in r3)
        diff, allowed = statistics.median(a) - statistics.median(b), max(spread(a), spread(b))
        say("     this - parent %+.4f ms; larger block-to-block spread %.4f ms: %s; pred / mean / var / lpd bit-identical: %s"
            % (diff, allowed, "not slower" if diff <= allowed else "SLOWER", same))


def logistic(n, feats, B, parent, note="", steps=20):
    theta, feed = base.logistic_inputs(n, feats, B)
    prod = GlmPredict("logistic", feats, w_col=1)
    case("logistic %d particles x %d features x %d rows%s" % (n, feats, B, note), n, B, prod, theta, feed,
         lambda: (feed["X"] @ theta[:, 1:].T).T,
         lambda f: -F.binary_cross_entropy_with_logits(f, feed["y"][None, :].expand_as(f), reduction="none"), parent, steps=steps)


def network(n, H, B, parent, steps=20):
    theta, cols, feed = base.network_inputs(n, H, B)
    prod = BnnPredict(1, H, cols)
    b1, b2, lg, w1, w2 = theta[:, :H], theta[:, H], theta[:, H + 1], theta[:, H + 3:2 * H + 3].reshape(n, 1, H), theta[:, 2 * H + 3:]

    def outputs():
        hidden = torch.relu(torch.einsum("pf,nfh->nph", feed["X"], w1) + b1[:, None, :])
        return torch.einsum("nph,nh->np", hidden, w2) + b2[:, None]
    case("network %d particles x %d hidden x %d rows" % (n, H, B), n, B, prod, theta, feed, outputs,
         lambda f: 0.5 * lg[:, None] - 0.5 * lg.exp()[:, None] * (f - feed["y"][None, :]) ** 2 - 0.5 * math.log(2 * math.pi),
         parent, steps=steps)


if __name__ == "__main__":
    parent = load_parent() if PARENT else None
    if parent is None:
        say("(no --parent library: comparison 3 not run)")
    logistic(16384, 54, 4000, parent)
    network(8192, 666, 200, parent)
    logistic(100, 54, 4000, parent, steps=50)
    network(20, 100, 20, parent, steps=50)
    logistic(16384, 200, 4000, parent, note=" (chunked arm)")
    if OUT_FILE:
        with open(OUT_FILE, "w") as f:
            f.write("\n".join(base.lines) + "\n")
