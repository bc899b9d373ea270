"""A/B of the weighted predictive quantiles (stein_amd/predict.py, weighted_quantiles) by the protocol of
profiles/predict_quantile_ab.txt: one process, variants alternated block by block, 5 warm-up calls, 5 blocks, device events.

    python scratch/predict_wquantile_ab.py --parent PATH_OF_THE_PARENT_COMMITS_libsteinhip.so [--out FILE] [--sections 3]

Per shape (the four example shapes and the GLM kernel's chunked arm):
  1. the weighted C call at three and at six levels (masses made once, outside the timing) against the parent commit's
     unweighted ranks call with as many ranks, against the torch route on the device -- the example's callable materialising
     [n, batch], torch.sort(dim=0), a gather of the weights, cumsum, searchsorted -- and the masses pass alone; peak of
     torch.cuda.max_memory_allocated over one call of each route;
  2. the same weighted calls under every digit width the hook can force (the rule's own width is marked);
  3. the existing calls, this commit against the parent commit's library loaded beside it: pred + mean + var + lpd, the
     six-rank call and the weighted call at three and at six levels, timed alternately and compared bit for bit.
--sections 3 runs section 3 alone (a change that must leave every call as it is needs nothing else).
"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ab as base  # noqa: E402  (inputs, timed, ab, report)
import predict_weighted_ab as wab  # noqa: E402  (load_parent, raw_unweighted, spread)
from predict_quantile_ab import peak_bytes  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wquantile_cases as wq  # noqa: E402  (the width rule restated)
from stein_amd import _lib  # noqa: E402
from stein_amd.predict import BnnPredict, GlmPredict  # noqa: E402

OUT_FILE = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
SECTIONS = sys.argv[sys.argv.index("--sections") + 1] if "--sections" in sys.argv else "all"
if SECTIONS not in ("all", "3"):
    sys.exit("--sections takes 'all' or '3', not %r" % SECTIONS)
ONLY_3 = SECTIONS == "3"
dev = base.dev
say = base.say
Q3 = (0.05, 0.5, 0.95)
Q6 = (0.025, 0.05, 0.25, 0.5, 0.75, 0.95)


def model_head(prod, theta, feed, n, B):
    d = theta.shape[1]
    if isinstance(prod, BnnPredict):
        return "bnn", [theta.data_ptr(), n, d, prod.n_in, prod.n_hidden, prod._cols, prod.output, feed["X"].data_ptr(), B]
    return "glm", [theta.data_ptr(), n, d, prod.kind, prod.output, prod.w_col, prod.n_feats, feed["X"].data_ptr(), B]


def raw_ranks(lib, prod, theta, feed, n, B, ranks):
    which, head = model_head(prod, theta, feed, n, B)
    fn = getattr(lib, "stein_predict_%s_ranks" % which)
    fn.argtypes, fn.restype = _lib._SIGNATURES["stein_predict_%s_ranks" % which], ctypes.c_int
    out = torch.empty(len(ranks), B, device=dev)
    ws = torch.empty(_lib.predict_ranks_workspace_bytes(n, B, len(ranks)), dtype=torch.uint8, device=dev)
    arr = (ctypes.c_int64 * len(ranks))(*ranks)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        assert fn(*head, arr, len(ranks), out.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    return call, out


def raw_wranks(lib, prod, theta, feed, n, B, masses, levels):
    which, head = model_head(prod, theta, feed, n, B)
    fn = getattr(lib, "stein_predict_%s_ranks_weighted" % which)
    fn.argtypes, fn.restype = _lib._SIGNATURES["stein_predict_%s_ranks_weighted" % which], ctypes.c_int
    out = torch.empty(len(levels), B, device=dev)
    ws = torch.empty(_lib.predict_ranks_weighted_workspace_bytes(n, B, len(levels)), dtype=torch.uint8, device=dev)
    arr = (ctypes.c_double * len(levels))(*levels)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        assert fn(*head, masses.data_ptr(), arr, len(levels), out.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    return call, out


def default_bits(prod, R, n, B):
    """the width the library's rule takes (restated in tests/wquantile_cases.py)"""
    rt, slices, _ = wq.pc.plan(n, B)
    other = wq.glm_other_bytes(prod.n_feats) if isinstance(prod, GlmPredict) else wq.bnn_other_bytes(prod.n_in)
    return wq.default_bits(R, other, rt * slices)


def case(tag, n, B, prod, theta, feed, outputs, parent, blocks=5, steps=20):
    gen = torch.Generator(device="cpu").manual_seed(1)
    w = torch.empty(n, dtype=torch.float64).exponential_(generator=gen).to(dev)
    masses = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.float64, device=dev)
    mws = torch.empty(_lib.predict_rank_masses_workspace_bytes(n), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def masses_pass():
        _lib.call("stein_predict_rank_masses", w.data_ptr(), n, _lib.MASS_NORMALISED, masses.data_ptr(), info.data_ptr(),
                  mws.data_ptr(), mws.numel(), stream)
    masses_pass()
    if not ONLY_3:
        sections_1_2(tag, n, B, prod, theta, feed, outputs, parent, blocks, steps, w, masses, masses_pass)
    else:
        say("%s, %d x %d calls" % (tag, blocks, steps))
    if parent is not None:
        section_3(n, B, prod, theta, feed, parent, blocks, steps, masses)


def sections_1_2(tag, n, B, prod, theta, feed, outputs, parent, blocks, steps, w, masses, masses_pass):
    keep = {}

    def torch_route(qs):
        f = outputs()                                                          # [n, B], the example's callable
        srt, order = torch.sort(f, dim=0)
        cum = torch.cumsum((w / w.sum())[order], dim=0)                        # [n, B] in fp64
        at = torch.searchsorted(cum.T.contiguous(), torch.tensor(qs, dtype=torch.float64, device=dev).expand(B, -1).contiguous())
        return torch.gather(srt, 0, at.clamp_(max=n - 1).T)
    variants = {"masses pass alone": masses_pass}
    outs = {}
    for qs in (Q3, Q6):
        k = len(qs)
        call, outs["w%d" % k] = raw_wranks(_lib.load(), prod, theta, feed, n, B, masses, qs)
        variants["this: weighted, %d levels (%d bits)" % (k, default_bits(prod, k, n, B))] = call
        if parent is not None:
            call, outs["p%d" % k] = raw_ranks(parent, prod, theta, feed, n, B, [int(q * (n - 1)) for q in qs])
            variants["parent: unweighted, %d ranks" % k] = call
        variants["torch: callable + sort + cumsum + searchsorted, %d levels" % k] = \
            (lambda qs=qs, k=k: keep.__setitem__("t%d" % k, torch_route(qs)))
    res = base.ab(variants, 5, blocks, steps)
    torch.cuda.synchronize()
    base.report("%s, %d x %d calls; max |this - torch route| %.2e / %.2e" % (
        tag, blocks, steps, *[float((outs["w%d" % k] - keep["t%d" % k]).abs().max()) for k in (3, 6)]), res)
    med = {k: statistics.median(v) for k, v in res.items()}
    name = {k: [v for v in med if v.startswith("this: weighted, %d" % k)][0] for k in (3, 6)}
    mem = {"this: weighted, 6 levels": peak_bytes(lambda: prod.weighted_quantiles(theta, feed, w, Q6)),
           "torch route, 6 levels": peak_bytes(lambda: torch_route(Q6))}
    for k, v in mem.items():
        say("  peak device memory of one call, %-26s %.2f MB" % (k + ":", v / 1e6))
    for k in (3, 6):
        r = med[name[k]] / med["torch: callable + sort + cumsum + searchsorted, %d levels" % k]
        say("  1. %d levels / torch route: %.3f  (%s)" % (k, r, "this call wins" if r < 1 else "THIS CALL LOSES TO TORCH"))
        if parent is not None:
            say("     %d levels / parent's unweighted call with %d ranks: %.3f" % (k, k, med[name[k]] / med["parent: unweighted, %d ranks" % k]))
    # 2. every width the hook can force
    widths = {}
    calls = {}
    for k, qs in ((3, Q3), (6, Q6)):
        calls[k], _ = raw_wranks(_lib.load(), prod, theta, feed, n, B, masses, qs)

    def forced(k, bits):
        def run():
            _lib.debug_predict_ranks_weighted_bits(bits)
            try:
                calls[k]()
            finally:
                _lib.debug_predict_ranks_weighted_bits(0)
        return run
    for k in (3, 6):
        for bits in (1, 2, 3, 4):
            try:
                forced(k, bits)()
            except AssertionError:
                continue
            widths["%d levels, %d bits%s" % (k, bits, " (the rule)" if bits == default_bits(prod, k, n, B) else "")] = forced(k, bits)
    base.report("  2. forced digit widths", base.ab(widths, 3, 3, max(steps // 2, 5)))


def section_3(n, B, prod, theta, feed, parent, blocks, steps, masses):
    this_call, this_bufs = wab.raw_unweighted(_lib.load(), prod, theta, feed, n, B)
    par_call, par_bufs = wab.raw_unweighted(parent, prod, theta, feed, n, B)
    six = [int(q * (n - 1)) for q in Q6]
    this_r, this_out = raw_ranks(_lib.load(), prod, theta, feed, n, B, six)
    par_r, par_out = raw_ranks(parent, prod, theta, feed, n, B, six)
    variants = {"this commit: pred + mean + var + lpd (C call)": this_call, "parent commit: the same call": par_call,
                "this commit: 6 ranks (C call)": this_r, "parent commit: 6 ranks": par_r}
    pairs = [("summary", lambda: all(torch.equal(this_bufs[k].view(torch.int32), par_bufs[k].view(torch.int32)) for k in this_bufs)),
             ("6 ranks", lambda: torch.equal(this_out.view(torch.int32), par_out.view(torch.int32)))]
    for qs in (Q3, Q6):
        this_w, this_wout = raw_wranks(_lib.load(), prod, theta, feed, n, B, masses, qs)
        par_w, par_wout = raw_wranks(parent, prod, theta, feed, n, B, masses, qs)
        variants["this commit: weighted, %d levels (C call)" % len(qs)] = this_w
        variants["parent commit: weighted, %d levels" % len(qs)] = par_w
        pairs.append(("weighted, %d levels" % len(qs),
                      lambda a=this_wout, b=par_wout: torch.equal(a.view(torch.int32), b.view(torch.int32))))
    r3 = base.ab(variants, 5, blocks, steps)
    torch.cuda.synchronize()
    base.report("  3. existing calls, this commit against the parent commit's library", r3)
    v = list(r3.values())
    for i, (what, same) in enumerate(pairs):
        a, b = v[2 * i], v[2 * i + 1]
        diff, allowed = statistics.median(a) - statistics.median(b), max(wab.spread(a), wab.spread(b))
        say("     %s: this - parent %+.4f ms; larger block-to-block spread %.4f ms: %s; bit-identical: %s"
            % (what, diff, allowed, "not slower" if diff <= allowed else "SLOWER", same()))


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
    parent = wab.load_parent() if wab.PARENT else None
    if parent is None:
        say("(no --parent library: the comparisons with the parent commit are not run)")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else "all"
    if only in ("all", "first"):
        logistic(16384, 54, 4000, parent, steps=10)
        network(8192, 666, 200, parent, steps=10)
        logistic(100, 54, 4000, parent, steps=30)
        network(20, 100, 20, parent, steps=30)
    if only in ("all", "chunked"):
        logistic(16384, 200, 4000, parent, note=" (chunked arm)", steps=5)
    if OUT_FILE:
        with open(OUT_FILE, "w") as f:
            f.write("\n".join(base.lines) + "\n")
