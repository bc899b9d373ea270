"""A/B of the predictive order statistics (stein_amd/predict.py, order_statistics) by the protocol of profiles/predict_ab.txt
section 1: one process, variants alternated block by block, 5 warm-up calls, 5 blocks, device events.

    python scratch/predict_quantile_ab.py [--out FILE] [--parent PATH_OF_THE_PARENT_COMMITS_libsteinhip.so]
    python scratch/predict_quantile_ab.py --trace logistic|network|chunked|small   30 six-rank and 30 summary calls at that shape
                                                                               (small: logistic, 100 particles) and
                                                                               nothing else, for a profiler run of its own

Per shape (the four example shapes and the GLM kernel's chunked arm):
  1. the two-rank and the six-rank call against the torch route on the device: the example's callable materialising
     [n, batch], then torch.sort(dim=0) and a gather of the ranks (and torch.quantile where it takes the size), with the peak
     of torch.cuda.max_memory_allocated over one call of each;
  2. the cost model: 8 levels x this commit's mean / var summary call at the same shape;
  3. with --parent: the unweighted C calls of this commit against the same calls into the parent commit's library, loaded
     beside this one and alternated in the same session, and bit-identity of pred / mean / var / lpd between the two.
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ab as base  # noqa: E402  (inputs, timed, ab, report)
import predict_weighted_ab as wab  # noqa: E402  (load_parent, raw_unweighted, spread)
from stein_amd import _lib  # noqa: E402
from stein_amd.predict import BnnPredict, GlmPredict  # noqa: E402

OUT_FILE = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = base.dev
say = base.say
LEVELS = 8


def peak_bytes(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    del keep
    return peak


def case(tag, n, B, prod, theta, feed, outputs, parent, blocks=5, steps=20):
    two = [int(0.05 * (n - 1)), int(0.95 * (n - 1))]
    six = [int(q * (n - 1)) for q in (0.025, 0.05, 0.25, 0.5, 0.75, 0.95)]
    idx2, idx6 = torch.tensor(two, device=dev), torch.tensor(six, device=dev)
    qs = torch.tensor([0.05, 0.95], device=dev)
    keep = {}

    def sort_route(idx):
        return torch.sort(outputs(), dim=0).values[idx]

    def quantile_route():
        return torch.quantile(outputs(), qs, dim=0, interpolation="lower")
    variants = {"this: 2 ranks": lambda: keep.__setitem__("r2", prod.order_statistics(theta, feed, two)),
                "this: 6 ranks": lambda: keep.__setitem__("r6", prod.order_statistics(theta, feed, six)),
                "this: mean / var summary": lambda: keep.__setitem__("s", prod.summary(theta, feed, lpd=False)),
                "torch: callable + sort + 2 ranks": lambda: keep.__setitem__("t2", sort_route(idx2)),
                "torch: callable + sort + 6 ranks": lambda: keep.__setitem__("t6", sort_route(idx6))}
    try:
        quantile_route()
        variants["torch: callable + quantile (2, lower)"] = lambda: keep.__setitem__("tq", quantile_route())
    except RuntimeError as e:
        say("  (torch.quantile refuses this size: %s)" % str(e).splitlines()[0])
    res = base.ab(variants, 5, blocks, steps)
    torch.cuda.synchronize()
    own = torch.sort(prod(theta, feed), dim=0).values
    exact = bool(torch.equal(keep["r2"], own[idx2])) and bool(torch.equal(keep["r6"], own[idx6]))
    errs = [float((keep["r%d" % k] - keep["t%d" % k]).abs().max()) for k in (2, 6)]
    base.report("%s, %d x %d calls; ranks equal torch.sort of the library's own pred: %s; max |this - torch route| %.2e / %.2e"
                % (tag, blocks, steps, exact, *errs), res)
    med = {k: statistics.median(v) for k, v in res.items()}
    mem = {"this: 6 ranks": peak_bytes(lambda: prod.order_statistics(theta, feed, six)),
           "torch: callable + sort + 6 ranks": peak_bytes(lambda: sort_route(idx6))}
    for k, v in mem.items():
        say("  peak device memory of one call, %-34s %.2f MB" % (k + ":", v / 1e6))
    for k in (2, 6):
        r = med["this: %d ranks" % k] / med["torch: callable + sort + %d ranks" % k]
        say("  1. %d ranks / torch sort route: %.3f  (%s)" % (k, r, "this call wins" if r < 1 else "THIS CALL LOSES TO TORCH"))
    if "torch: callable + quantile (2, lower)" in med:
        say("     2 ranks / torch.quantile route: %.3f" % (med["this: 2 ranks"] / med["torch: callable + quantile (2, lower)"]))
    model = LEVELS * med["this: mean / var summary"]
    say("  2. cost model %d x summary = %.4f ms; 2 ranks / model %.2f, 6 ranks / model %.2f"
        % (LEVELS, model, med["this: 2 ranks"] / model, med["this: 6 ranks"] / model))
    if parent is not None:
        this_call, this_bufs = wab.raw_unweighted(_lib.load(), prod, theta, feed, n, B)
        par_call, par_bufs = wab.raw_unweighted(parent, prod, theta, feed, n, B)
        r3 = base.ab({"this commit: pred + mean + var + lpd (C call)": this_call, "parent commit: the same call": par_call}, 5, blocks, steps)
        torch.cuda.synchronize()
        same = all(torch.equal(this_bufs[k].view(torch.int32), par_bufs[k].view(torch.int32)) for k in this_bufs)
        base.report("  3. unweighted call, this commit against the parent commit's library", r3)
        a, b = (r3[k] for k in r3)
        diff, allowed = statistics.median(a) - statistics.median(b), max(wab.spread(a), wab.spread(b))
        say("     this - parent %+.4f ms; larger block-to-block spread %.4f ms: %s; pred / mean / var / lpd bit-identical: %s"
            % (diff, allowed, "not slower" if diff <= allowed else "SLOWER", same))


def logistic(n, feats, B, parent, note="", steps=20):
    theta, feed = base.logistic_inputs(n, feats, B)
    prod = GlmPredict("logistic", feats, w_col=1)
    case("logistic %d particles x %d features x %d rows%s" % (n, feats, B, note), n, B, prod, theta, feed,
         lambda: (feed["X"] @ theta[:, 1:].T).T, parent, steps=steps)


def network(n, H, B, parent, steps=20):
    theta, cols, feed = base.network_inputs(n, H, B)
    prod = BnnPredict(1, H, cols)
    b1, b2, w1, w2 = theta[:, :H], theta[:, H], theta[:, H + 3:2 * H + 3].reshape(n, 1, H), theta[:, 2 * H + 3:]

    def outputs():
        hidden = torch.relu(torch.einsum("pf,nfh->nph", feed["X"], w1) + b1[:, None, :])
        return torch.einsum("nph,nh->np", hidden, w2) + b2[:, None]
    case("network %d particles x %d hidden x %d rows" % (n, H, B), n, B, prod, theta, feed, outputs, parent, steps=steps)


if __name__ == "__main__":
    if "--trace" in sys.argv:
        which = sys.argv[sys.argv.index("--trace") + 1]
        if which == "network":
            theta, cols, feed = base.network_inputs(8192, 666, 200)
            prod = BnnPredict(1, 666, cols)
        else:
            feats = 200 if which == "chunked" else 54
            theta, feed = base.logistic_inputs(100 if which == "small" else 16384, feats, 4000)
            prod = GlmPredict("logistic", feats, w_col=1)
        n = theta.shape[0]
        for _ in range(30):
            prod.order_statistics(theta, feed, [int(q * (n - 1)) for q in (0.025, 0.05, 0.25, 0.5, 0.75, 0.95)])
        for _ in range(30):
            prod.summary(theta, feed, lpd=False)
        torch.cuda.synchronize()
        sys.exit(0)
    parent = wab.load_parent() if wab.PARENT else None
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
