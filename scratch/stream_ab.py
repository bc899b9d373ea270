"""The streaming step (SvgdEngine(h2=...), stein_svgd_phi_stream) against the default stored-D step.
usage: stream_ab.py                      the A/B table: 4096 x 256, 16384 x 256 (C3), 65536 x 256, 8192 x 2001 (C4)
       stream_ab.py --stream-only N D    only the streaming step, 60 calls: the run to put under
                                         `rocprofv3 --kernel-trace --stats` for k_phi_stream's share of the step
Alternates the default engine (exact median of all n^2 distances, speculative window warm) with a streaming engine fed that
engine's h2 tensor, 5 x 50 steps each (step time by host clock around synchronised loops), and prints ms per step for both
and both workspace sizes.  A shape whose stored-D workspace does not fit the card is reported for the streaming step alone."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stein_amd import _lib
from stein_amd.engine import SvgdEngine
def run(eng, T, G, steps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        eng.compute_phi(T, G)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3
def inputs(n, d):
    torch.manual_seed(0)
    return torch.randn(n, d, device="cuda"), torch.randn(n, d, device="cuda")
if len(sys.argv) > 1 and sys.argv[1] == "--stream-only":
    n, d = int(sys.argv[2]), int(sys.argv[3])
    T, G = inputs(n, d)
    eng = SvgdEngine(n, d, device="cuda", h2=2.0 * d / torch.log(torch.tensor(float(n))).item())
    print("%d x %d streaming only: %.4f ms per step (60 calls after 10)" % (n, d, (run(eng, T, G, 10), run(eng, T, G, 60))[1]))
    sys.exit(0)
for n, d in ((4096, 256), (16384, 256), (65536, 256), (8192, 2001)):
    T, G = inputs(n, d)
    stored_bytes = _lib.workspace_layout(n, n, d, _lib.F32, _lib.FLAG_X3)[0]
    free = torch.cuda.mem_get_info()[0]
    stored = SvgdEngine(n, d, device="cuda") if stored_bytes < 0.8 * free else None
    if stored is not None:
        run(stored, T, G, 10)                      # warms the median window; leaves the bandwidth in stored.h2
        h2 = stored.h2
    else:
        h2 = torch.full((1,), 2.0 * d / torch.log(torch.tensor(float(n))).item(), device="cuda")
    stream = SvgdEngine(n, d, device="cuda", h2=h2)
    run(stream, T, G, 10)
    res = {"stored": [], "stream": []}
    for rep in range(5):
        if stored is not None:
            res["stored"].append(run(stored, T, G, 50))
        res["stream"].append(run(stream, T, G, 50))
    med = {k: (sorted(v)[2] if v else float("nan")) for k, v in res.items()}
    print("%d x %d  plan (row tiles, column groups, j ranges) %s" % (n, d, (stream.row_tiles, stream.col_groups, stream.jsplit)))
    print("  step ms per rep: stored-D %s | streaming %s" % (["%.4f" % x for x in res["stored"]], ["%.4f" % x for x in res["stream"]]))
    print("  median step: stored-D %.4f ms, streaming %.4f ms (x %.2f);  workspace: stored-D %.1f MiB, streaming %.1f MiB" %
          (med["stored"], med["stream"], med["stream"] / med["stored"], stored_bytes / 2.0 ** 20, stream.ws_bytes / 2.0 ** 20))
    del stored, stream
    torch.cuda.empty_cache()
