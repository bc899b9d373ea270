"""What does STEIN_FLAG_KSD cost the step?  usage: ksd_cost.py <c2|c3>.  Alternates a plain engine and a ksd=True engine on
the same inputs (step time by host clock around synchronised loops; the finish stage by the library's stage events)."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stein_amd import _lib
from stein_amd.engine import SvgdEngine
which = sys.argv[1] if len(sys.argv) > 1 else "c3"
n, d, dt = (4096, 128, torch.bfloat16) if which == "c2" else (16384, 256, torch.float32)
torch.manual_seed(0)
T = torch.randn(n, d, device="cuda").to(dt); G = torch.randn(n, d, device="cuda").to(dt)
engs = {"plain": SvgdEngine(n, d, device="cuda", dtype=dt), "ksd": SvgdEngine(n, d, device="cuda", dtype=dt, ksd=True)}
def run(eng, steps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        eng.compute_phi(T, G)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3
def finish_ms(eng, steps):
    _lib.timing_reserve(steps)
    for _ in range(steps):
        eng.compute_phi(T, G, timing=True)
    st = _lib.timing_read(steps)
    return sorted(s["finish"] for s in st)[steps // 2] * 1e3
for e in engs.values():
    run(e, 10)
res = {k: [] for k in engs}
for rep in range(5):
    for k, e in engs.items():
        res[k].append(run(e, 50))
print("%s step ms per rep: plain %s | ksd %s" % (which, ["%.4f" % x for x in res["plain"]], ["%.4f" % x for x in res["ksd"]]))
print("%s median step: plain %.4f ms, ksd %.4f ms (delta %.1f us)" % (which, sorted(res["plain"])[2], sorted(res["ksd"])[2],
      (sorted(res["ksd"])[2] - sorted(res["plain"])[2]) * 1e3))
print("%s finish stage median (stage events): plain %.1f us, ksd %.1f us" % (which, finish_ms(engs["plain"], 40), finish_ms(engs["ksd"], 40)))
