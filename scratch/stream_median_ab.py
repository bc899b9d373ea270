"""The streaming median (stein_stream_median; SvgdEngine(h2="median", median_every=k)) beside the streaming step at a
supplied bandwidth and the default stored-D step.
usage: stream_median_ab.py                      the table: 4096 x 256, 16384 x 256 (C3), 65536 x 256, 262144 x 256
       stream_median_ab.py --median-only N D    only the median call, 40 calls after 5: the run to put under
                                                `rocprofv3 --kernel-trace --stats` for the three k_stream_hist launches
Five measurements alternated on the same inputs, 5 repetitions each, ms by host clock around synchronised loops:
    median      eng.refresh_bandwidth(theta) alone (stein_stream_median)
    every 1     the streaming step with the median taken in every call
    every 10    ... in every tenth call (loops are multiples of ten calls: exactly one median per ten steps)
    supplied    the streaming step at a supplied h2 (the stored-D engine's tensor where that engine exists)
    stored-D    the default step: exact median of the stored n x n image, speculative window warm
A shape whose stored-D workspace does not fit the card has the streaming columns only.  Loop lengths follow a warm-up
timing so that one measurement lasts about half a second (2 to 50 calls; multiples of ten for `every 10`)."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stein_amd import _lib
from stein_amd.engine import SvgdEngine
def timed(fn, calls):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3
def inputs(n, d):
    torch.manual_seed(0)
    return torch.randn(n, d, device="cuda"), torch.randn(n, d, device="cuda")
def calls_for(ms, multiple=1):
    c = max(2, min(50, int(500.0 / max(ms, 1e-3))))
    return max(multiple, c // multiple * multiple)
if len(sys.argv) > 1 and sys.argv[1] == "--median-only":
    n, d = int(sys.argv[2]), int(sys.argv[3])
    T, G = inputs(n, d)
    eng = SvgdEngine(n, d, device="cuda", h2="median")
    timed(lambda: eng.refresh_bandwidth(T), 5)
    print("%d x %d median call only: %.4f ms per call (40 calls after 5), h2 %.6f" %
          (n, d, timed(lambda: eng.refresh_bandwidth(T), 40), eng.h2.item()))
    sys.exit(0)
for n, d in ((4096, 256), (16384, 256), (65536, 256), (262144, 256)):
    T, G = inputs(n, d)
    stored_bytes = _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3)[0]
    stored = SvgdEngine(n, d, device="cuda") if stored_bytes < 0.8 * torch.cuda.mem_get_info()[0] else None
    m1 = SvgdEngine(n, d, device="cuda", h2="median", median_every=1)
    m10 = SvgdEngine(n, d, device="cuda", h2="median", median_every=10)
    if stored is not None:
        timed(lambda: stored.compute_phi(T, G), 10)    # warms the median window; leaves the bandwidth in stored.h2
    supplied = SvgdEngine(n, d, device="cuda", h2=stored.h2 if stored is not None else m1.refresh_bandwidth(T).clone())
    runs = [("median", lambda: m1.refresh_bandwidth(T), 1), ("every 1", lambda: m1.compute_phi(T, G), 1),
            ("every 10", lambda: m10.compute_phi(T, G), 10), ("supplied", lambda: supplied.compute_phi(T, G), 1)]
    if stored is not None:
        runs.append(("stored-D", lambda: stored.compute_phi(T, G), 1))
    calls = {name: calls_for(timed(fn, 2 * mult), mult) for name, fn, mult in runs}
    res = {name: [] for name, _, _ in runs}
    for rep in range(5):
        for name, fn, _ in runs:
            res[name].append(timed(fn, calls[name]))
    print("%d x %d  tiles, workgroups %s;  workspace: streaming (median included) %.1f MiB, stored-D %.1f MiB%s" %
          (n, d, _lib.stream_median_plan(n, d)[2:], m1.ws_bytes / 2.0 ** 20, stored_bytes / 2.0 ** 20,
           "" if stored is not None else " (does not fit the card)"))
    for name, _, _ in runs:
        print("  %-9s ms per call, %2d calls per repetition: %s  median %.4f" %
              (name, calls[name], ["%.4f" % x for x in res[name]], sorted(res[name])[2]))
    print("  h2: streaming median %.7g%s" % (m1.h2.item(), ", stored-D %.7g" % stored.h2.item() if stored is not None else ""))
    del stored, m1, m10, supplied, runs
    torch.cuda.empty_cache()
