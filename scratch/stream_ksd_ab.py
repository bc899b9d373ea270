"""A/B of the streaming step with and without discrepancy=True, the standalone statistic with phi = NULL, and the stored-D
step with and without ksd=True (profiles/stream_ksd_ab.txt).  Device events around blocks of steps, variants alternated.

    python scratch/stream_ksd_ab.py [--parent-lib PATH] [--out FILE]
    python scratch/stream_ksd_ab.py --trace N D          70 discrepancy steps and nothing else, for a profiler run of its own

--parent-lib: a libsteinhip.so built from the parent commit; its plain streaming step is then called at the C ABI on the same
tensors, alternated with this tree's, and the outputs are compared bit for bit."""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stein_amd.engine import SvgdEngine  # noqa: E402


def _opt(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


PARENT_LIB, OUT_FILE = _opt("--parent-lib"), _opt("--out")
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def ab(variants, warm, blocks, steps):
    """variants: {name: fn}; alternated block by block -> {name: [ms per step of each block]}"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            res[k].append(timed(fn, steps))
    return res


def report(tag, res):
    say(tag)
    for k, v in res.items():
        say("  %-34s median %.4f ms   per block %s" % (k, statistics.median(v), ["%.4f" % x for x in v]))


def parent_plain(n, d, T, G, h2, phi, sq):
    lib = ctypes.CDLL(PARENT_LIB)
    vp, i64, ci, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    lib.stein_svgd_phi_stream.argtypes = [vp, vp, i64, i64, ci, vp, vp, vp, vp, sz, ci, vp]
    lib.stein_stream_workspace_bytes.argtypes = [i64, i64, ci, ci, ctypes.POINTER(sz)]
    need = sz(0)
    assert lib.stein_stream_workspace_bytes(n, d, 0, 0, ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)

    def fn():
        rc = lib.stein_svgd_phi_stream(vp(T.data_ptr()), vp(G.data_ptr()), n, d, 0, vp(h2.data_ptr()), vp(phi.data_ptr()),
                                       vp(sq.data_ptr()), vp(ws.data_ptr()), need.value, 0, stream)
        assert rc == 0, rc
    return fn


def stream_case(n, d, blocks=5, steps=50):
    gen = torch.Generator(device="cpu").manual_seed(0)
    T, G = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, d, generator=gen).to(dev)
    ref = SvgdEngine(n, d, device=dev)
    ref.compute_phi(T, G)
    h2 = ref.h2.clone()
    plain = SvgdEngine(n, d, device=dev, h2=h2)
    withk = SvgdEngine(n, d, device=dev, h2=h2)
    pphi, psq = torch.empty(n, d, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    variants = {"this, plain step": lambda: plain.compute_phi(T, G),
                "this, discrepancy=True": lambda: withk.compute_phi(T, G, discrepancy=True)}
    if PARENT_LIB:
        variants["parent, plain step"] = parent_plain(n, d, T, G, h2, pphi, psq)
    res = ab(variants, 10, blocks, steps)
    torch.cuda.synchronize()
    same = torch.equal(plain.phi, withk.phi) and torch.equal(plain.sqnorm, withk.sqnorm) and \
        (not PARENT_LIB or (torch.equal(plain.phi, pphi) and torch.equal(plain.sqnorm, psq)))
    report("streaming %d x %d, plan %s, %d x %d steps; phi / |phi|^2 of all %d bit-identical: %s" %
           (n, d, (plain.row_tiles, plain.col_groups, plain.jsplit), blocks, steps, len(variants), same), res)
    m = {k: statistics.median(v) for k, v in res.items()}
    say("  discrepancy=True costs %+.4f ms (%+.2f %%)" % (m["this, discrepancy=True"] - m["this, plain step"],
                                                         100 * (m["this, discrepancy=True"] / m["this, plain step"] - 1)))
    if PARENT_LIB:
        say("  this plain vs parent plain %+.2f %%" % (100 * (m["this, plain step"] / m["parent, plain step"] - 1)))
    st0, st1 = SvgdEngine(n, d, device=dev), SvgdEngine(n, d, device=dev, ksd=True)
    res = ab({"stored-D step": lambda: st0.compute_phi(T, G), "stored-D step, ksd=True": lambda: st1.compute_phi(T, G)},
             10, blocks, steps)
    report("stored-D %d x %d (median heuristic, window warm)" % (n, d), res)
    m = {k: statistics.median(v) for k, v in res.items()}
    say("  ksd=True costs %+.4f ms (%+.2f %%)" % (m["stored-D step, ksd=True"] - m["stored-D step"],
                                                  100 * (m["stored-D step, ksd=True"] / m["stored-D step"] - 1)))


def standalone(n, d, blocks=5, steps=10):
    gen = torch.Generator(device="cpu").manual_seed(0)
    T, G = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, d, generator=gen).to(dev)
    h2 = torch.full((1,), 2.0 * d / torch.log(torch.tensor(float(n))).item(), device=dev)
    eng = SvgdEngine(n, d, device=dev, h2=h2)
    plain = SvgdEngine(n, d, device=dev, h2=h2)
    res = ab({"statistic alone (phi = NULL)": lambda: eng.stream_discrepancy_sums(T, G),
              "plain step": lambda: plain.compute_phi(T, G)}, 3, blocks, steps)
    report("standalone %d x %d, workspace %.1f MiB (plain %.1f MiB), %d x %d calls" %
           (n, d, eng.ws_bytes / 2.0 ** 20, plain.ws_bytes / 2.0 ** 20, blocks, steps), res)
    say("  U = %.6e  V = %.6e" % (eng.stein_discrepancy("u").item(), eng.stein_discrepancy("v").item()))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n, d = int(sys.argv[2]), int(sys.argv[3])
        gen = torch.Generator(device="cpu").manual_seed(0)
        T, G = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, d, generator=gen).to(dev)
        eng = SvgdEngine(n, d, device=dev, h2=2.0 * d / 9.7)
        for _ in range(70):
            eng.compute_phi(T, G, discrepancy=True)
        torch.cuda.synchronize()
        sys.exit(0)
    stream_case(4096, 256)
    stream_case(16384, 256)
    standalone(65536, 256)
    if OUT_FILE:
        with open(OUT_FILE, "w") as f:
            f.write("\n".join(lines) + "\n")
