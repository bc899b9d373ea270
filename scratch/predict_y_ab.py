"""A/B of the predictive distribution of y: this commit's calls against the summary call (cost model), against the torch
route, and the existing predictive calls against the parent commit's library.  Prints, and writes predict_y_ab.txt into --out (default: the working directory).

    python scratch/predict_y_ab.py --parent <libsteinhip.so built from the parent commit>
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stein_amd import _lib  # noqa: E402
from stein_amd.predict import BnnPredict, GlmPredict  # noqa: E402

OUT = []


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def blocks(fn, calls, nblocks=5, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(nblocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / calls)
    return res


def line(name, res):
    say("  %-46s median %8.4f ms   per block %s" % (name, float(np.median(res)), ["%.4f" % r for r in res]))
    return float(np.median(res))


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def parent_lib(path):
    lib = ctypes.CDLL(path)
    for name, args in _lib._SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, ctypes.c_int
    return lib


def shape_run(tag, model, n, width, B, parent, calls):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if model == "linear":
        d = width
        theta = torch.randn(n, d, device=dev, generator=g) * 0.3
        X = torch.randn(B, width, device=dev, generator=g)
        prod = GlmPredict("linear", width, w_col=0, noise_precision=4.0)
        s_vec = torch.full((n,), 2.0, device=dev)
        cols = None
    else:
        H = width
        d = 3 * H + 3
        cols = (0, H, 2 * H, 3 * H, 3 * H + 1, 3 * H + 2)
        theta = torch.randn(n, d, device=dev, generator=g) * 0.3
        X = torch.rand(B, 1, device=dev, generator=g)
        prod = BnnPredict(1, H, cols)
        s_vec = torch.exp(0.5 * theta[:, 3 * H + 2])
    y = torch.randn(B, device=dev, generator=g)
    feed = {"X": X, "y": y}
    w = torch.rand(n, device=dev, generator=g, dtype=torch.float64)
    t1 = y.reshape(1, B).contiguous()
    t8 = (y[None, :] + torch.linspace(-2, 2, 8, device=dev)[:, None]).contiguous()
    q2, q6 = (0.05, 0.95), (0.025, 0.05, 0.25, 0.5, 0.75, 0.95)
    say("%s %d particles x %d %s x %d rows, 5 x %d calls" % (model, n, width, "features" if model == "linear" else "hidden", B, calls))

    # --- correctness of what is timed: the call against the torch route on the library's own pred, in fp64
    pred = prod(theta, feed).double()
    def F64(t):   # noqa: E306
        return torch.stack([torch.special.ndtr((t[i][None, :].double() - pred) * s_vec.double()[:, None]).mean(0) for i in range(t.shape[0])])
    got8 = prod.y_cdf(theta, feed, t8)
    lo6, hi6 = prod.y_quantiles(theta, feed, q6, return_bracket=True)
    Fhi, Flo = F64(hi6), F64(lo6)
    qv = torch.tensor(q6, device=dev, dtype=torch.float64)[:, None]
    say("  max |y_cdf - fp64 of own pred| %.2e; quantiles: max |F64(hi) - q| %.2e, F64(lo) <= q + 1e-5: %s, F64(hi) >= q - 1e-5: %s, "
        "largest hi - lo %.3g (%.1f ulp of the scale |hi| + 1 / sqrt(tau))"
        % (float((got8.double() - F64(t8)).abs().max()), float((Fhi - qv).abs().max()), bool((Flo <= qv + 1e-5).all()),
           bool((Fhi >= qv - 1e-5).all()), float((hi6 - lo6).max()),
           float(((hi6 - lo6).double() / torch.tensor(np.spacing((np.abs(hi6.cpu().numpy()) + float(1.0 / s_vec.min())).astype(np.float32)),
                                                      device=dev)).max())))
    del pred, Fhi, Flo

    # --- the calls
    heavy = max(1, calls // 4)
    m_sum = line("this: mean / var / lpd summary", blocks(lambda: prod.summary(theta, feed), calls))
    m_wsum = line("this: weighted summary", blocks(lambda: prod.weighted_summary(theta, feed, w), calls))
    m_c1 = line("this: y_cdf 1 point", blocks(lambda: prod.y_cdf(theta, feed, t1), calls))
    m_c8 = line("this: y_cdf 8 points", blocks(lambda: prod.y_cdf(theta, feed, t8), calls))
    m_c1w = line("this: y_cdf 1 point, weighted", blocks(lambda: prod.y_cdf(theta, feed, t1, weights=w), calls))
    m_c8w = line("this: y_cdf 8 points, weighted", blocks(lambda: prod.y_cdf(theta, feed, t8, weights=w), calls))
    m_q2 = line("this: y_quantiles 2 levels, 8 passes", blocks(lambda: prod.y_quantiles(theta, feed, q2), heavy))
    m_q6 = line("this: y_quantiles 6 levels, 8 passes", blocks(lambda: prod.y_quantiles(theta, feed, q6), heavy))
    m_q6w = line("this: y_quantiles 6 levels, 8 passes, weighted", blocks(lambda: prod.y_quantiles(theta, feed, q6, weights=w), heavy))
    m_q6p1 = line("this: y_quantiles 6 levels, 1 pass", blocks(lambda: prod.y_quantiles(theta, feed, q6, passes=1), heavy))
    m_q2p1 = line("this: y_quantiles 2 levels, 1 pass", blocks(lambda: prod.y_quantiles(theta, feed, q2, passes=1), heavy))

    # --- the torch route: pred, ndtr, (weighted) mean; and a bisection on the [n, batch] matrix
    wn = (w / w.sum()).float()

    def torch_cdf(t, weights=None):
        p = prod(theta, feed)
        out = torch.empty(t.shape[0], B, device=dev)
        for i in range(t.shape[0]):
            ph = torch.special.ndtr((t[i][None, :] - p) * s_vec[:, None])
            out[i] = ph.mean(0) if weights is None else (weights[:, None] * ph).sum(0)
        return out

    def torch_bisect(qs, iters=26):
        p = prod(theta, feed)
        out = torch.empty(len(qs), B, device=dev)
        span = 6.0 / float(s_vec.min())
        for i, q in enumerate(qs):
            lo, hi = p.min(0).values - span, p.max(0).values + span
            for _ in range(iters):
                mid = 0.5 * (lo + hi)
                below = torch.special.ndtr((mid[None, :] - p) * s_vec[:, None]).mean(0) < q
                lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
            out[i] = hi
        return out
    t_c1 = line("torch: pred + ndtr + mean, 1 point", blocks(lambda: torch_cdf(t1), calls))
    t_c8 = line("torch: pred + ndtr + mean, 8 points", blocks(lambda: torch_cdf(t8), heavy))
    t_c8w = line("torch: pred + ndtr + weighted sum, 8 points", blocks(lambda: torch_cdf(t8, wn), heavy))
    few = max(1, calls // 10)
    t_q2 = line("torch: pred + bisection (26 halvings), 2 levels", blocks(lambda: torch_bisect(q2), few, warm=1))
    t_q6 = line("torch: pred + bisection (26 halvings), 6 levels", blocks(lambda: torch_bisect(q6), few, warm=1))
    say("  peak device memory of one call: y_cdf 8 points %.2f MB, y_quantiles 6 levels %.2f MB; torch cdf 8 points %.2f MB, torch "
        "bisection %.2f MB" % (peak(lambda: prod.y_cdf(theta, feed, t8)), peak(lambda: prod.y_quantiles(theta, feed, q6)),
                               peak(lambda: torch_cdf(t8)), peak(lambda: torch_bisect(q2, 2))))

    def verdict(r):
        return "(THIS CALL LOSES TO TORCH)" if r > 1.0 else "(this call wins)"
    say("  1. y_cdf / summary (cost model 1 x): 1 point %.2f, 8 points %.2f; weighted against the weighted summary: %.2f, %.2f"
        % (m_c1 / m_sum, m_c8 / m_sum, m_c1w / m_wsum, m_c8w / m_wsum))
    for name, a, b in (("y_cdf 1 point", m_c1, t_c1), ("y_cdf 8 points", m_c8, t_c8), ("y_cdf 8 points, weighted", m_c8w, t_c8w)):
        say("     %s / torch route: %.3f  %s" % (name, a / b, verdict(a / b)))
    say("  2. y_quantiles / (9 x summary = %.4f ms): 2 levels %.2f, 6 levels %.2f, 6 levels weighted %.2f (of 9 x weighted summary)"
        % (9 * m_sum, m_q2 / (9 * m_sum), m_q6 / (9 * m_sum), m_q6w / (9 * m_wsum)))
    for name, a, b in (("y_quantiles 2 levels", m_q2, t_q2), ("y_quantiles 6 levels", m_q6, t_q6)):
        say("     %s / torch bisection: %.3f  %s" % (name, a / b, verdict(a / b)))
    pass6, pass2 = (m_q6 - m_q6p1) / 7.0, (m_q2 - m_q2p1) / 7.0
    say("     a refinement pass: 6 levels (42 erfcf per particle and row) %.4f ms, 2 levels (14) %.4f ms, the summary call %.4f ms: "
        "the forward pass is at most %.0f %% / %.0f %% of a pass, the rest erfcf, the sums and the finish"
        % (pass6, pass2, m_sum, 100 * min(1.0, m_sum / pass6), 100 * min(1.0, m_sum / pass2)))

    # --- 3. the existing calls, this commit against the parent's library: bits and time
    stream = torch.cuda.current_stream(dev).cuda_stream
    libs = {"this commit": _lib.load(), "parent commit": parent}
    res, outs = {}, {}
    cc = (ctypes.c_int64 * 6)(*cols) if cols else None
    for name, lib in libs.items():
        pr_, mean, var, lpd = (torch.empty(n, B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev))
        wmean, wvar, wlpd, ess = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(1, device=dev, dtype=torch.float64)
        ws = torch.empty(_lib.predict_weighted_workspace_bytes(n, B), dtype=torch.uint8, device=dev)
        rk = torch.empty(2, B, device=dev)
        rws = torch.empty(_lib.predict_ranks_workspace_bytes(n, B, 2), dtype=torch.uint8, device=dev)
        ranks = (ctypes.c_int64 * 2)(n // 20, n - 1 - n // 20)
        if model == "linear":
            def full(lib=lib, o=(pr_, mean, var, lpd), ws=ws):
                assert lib.stein_predict_glm(theta.data_ptr(), n, d, 0, 0, 0, width, X.data_ptr(), y.data_ptr(), B, 4.0, o[0].data_ptr(),
                                             o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0

            def wfull(lib=lib, o=(wmean, wvar, wlpd, ess), ws=ws):
                assert lib.stein_predict_glm_weighted(theta.data_ptr(), n, d, 0, 0, 0, width, X.data_ptr(), y.data_ptr(), B, 4.0, w.data_ptr(),
                                                      None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr(),
                                                      ws.numel(), stream) == 0

            def rank2(lib=lib, rk=rk, rws=rws, ranks=ranks):
                assert lib.stein_predict_glm_ranks(theta.data_ptr(), n, d, 0, 0, 0, width, X.data_ptr(), B, ranks, 2, rk.data_ptr(),
                                                   rws.data_ptr(), rws.numel(), stream) == 0
        else:
            def full(lib=lib, o=(pr_, mean, var, lpd), ws=ws):
                assert lib.stein_predict_bnn(theta.data_ptr(), n, d, 1, width, cc, 0, X.data_ptr(), y.data_ptr(), B, o[0].data_ptr(),
                                             o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0

            def wfull(lib=lib, o=(wmean, wvar, wlpd, ess), ws=ws):
                assert lib.stein_predict_bnn_weighted(theta.data_ptr(), n, d, 1, width, cc, 0, X.data_ptr(), y.data_ptr(), B, w.data_ptr(), None,
                                                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr(),
                                                      ws.numel(), stream) == 0

            def rank2(lib=lib, rk=rk, rws=rws, ranks=ranks):
                assert lib.stein_predict_bnn_ranks(theta.data_ptr(), n, d, 1, width, cc, 0, X.data_ptr(), B, ranks, 2, rk.data_ptr(),
                                                   rws.data_ptr(), rws.numel(), stream) == 0
        full()
        full_out = [t_.clone() for t_ in (pr_, mean, var, lpd)]
        wfull()
        rank2()
        torch.cuda.synchronize()
        outs[name] = full_out + [wmean.clone(), wvar.clone(), wlpd.clone(), ess.clone(), rk.clone()]
        res[name] = (full, wfull, rank2)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs["this commit"], outs["parent commit"]))
    say("  3. existing calls, this commit against the parent commit's library (alternated block by block)")
    for k, what in enumerate(("pred + mean + var + lpd (C call)", "weighted mean + var + lpd + ess (C call)", "2 ranks (C call)")):
        cnt = calls if k < 2 else heavy
        a_blocks, b_blocks = [], []
        for fn in (res["this commit"][k], res["parent commit"][k]):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(5):
            a_blocks += blocks(res["this commit"][k], cnt, nblocks=1, warm=0)
            b_blocks += blocks(res["parent commit"][k], cnt, nblocks=1, warm=0)
        ma, mb = line("this commit: " + what, a_blocks), line("parent commit: the same call", b_blocks)
        spread = max(max(a_blocks) - min(a_blocks), max(b_blocks) - min(b_blocks))
        say("     this - parent %+.4f ms; larger block-to-block spread %.4f ms: %s" % (ma - mb, spread, "not slower" if ma - mb <= spread else "SLOWER"))
    say("     pred / mean / var / lpd / weighted mean, var, lpd, ess / 2 ranks bit-identical: %s" % same)
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    parent = parent_lib(args.parent)
    shapes = [("A", "linear", 16384, 54, 4000, 20), ("B", "bnn", 8192, 666, 200, 20), ("C", "linear", 100, 54, 4000, 50),
              ("D", "bnn", 20, 100, 20, 50), ("E", "linear", 16384, 200, 4000, 20)]
    say("device: %s" % torch.cuda.get_device_name(0))
    for i, sh in enumerate(shapes):
        if args.only is None or args.only == i:
            shape_run(*sh[:5], parent, sh[5])
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "predict_y_ab.txt"), "w") as f:
                f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
