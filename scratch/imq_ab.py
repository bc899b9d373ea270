"""A/B of the IMQ step (stein_svgd_phi_imq, stein_svgd_phi_imq_ksd; this tree's library) against the RBF streaming step of a
library built from the PARENT commit, at the C ABI, alternated on the same tensors and one workspace (profiles/imq_ab.txt).
Host clock around synchronised loops; rounds of at least a quarter of a second.

    python scratch/imq_ab.py --parent-lib PATH [--out FILE]
    python scratch/imq_ab.py --imq-only N D            60 IMQ steps and nothing else, for a profiler run of its own

--parent-lib: a libsteinhip.so built from the parent commit's sources."""
import ctypes
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stein_amd import _lib  # noqa: E402



def _opt(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


new = _lib.load()
par = ctypes.CDLL(_opt("--parent-lib")) if _opt("--parent-lib") else new      # (--imq-only needs no parent)
vp, i64, sz, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
STEP = [vp, vp, i64, i64, ci, vp, vp, vp, vp, sz, ci, vp]
for name in ("stein_svgd_phi_stream", "stein_svgd_phi_stream_ksd"):
    getattr(par, name).argtypes = STEP
    getattr(par, name).restype = ci
for name in ("stein_stream_workspace_bytes", "stein_stream_ksd_workspace_bytes"):
    getattr(par, name).argtypes = [i64, i64, ci, ci, ctypes.POINTER(sz)]
    getattr(par, name).restype = ci


def p(t):
    return vp(t.data_ptr())


def main(shapes, reps=5, steps=50, only=None):
    dev = torch.device("cuda:0")
    out = open(_opt("--out"), "a") if _opt("--out") else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    for n, d in shapes:
        gen = torch.Generator(device="cpu").manual_seed(0)
        T = torch.randn(n, d, generator=gen).to(dev)
        G = torch.randn(n, d, generator=gen).to(dev)
        h2 = torch.full((1,), 2.0 * d / math.log(n), dtype=torch.float32, device=dev)
        phi = torch.empty(n, d, device=dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        b = sz(0)
        sizes = {}
        par.stein_stream_workspace_bytes(n, d, _lib.F32, 0, ctypes.byref(b)); sizes["stream"] = b.value
        par.stein_stream_ksd_workspace_bytes(n, d, _lib.F32, 0, ctypes.byref(b)); sizes["stream_ksd"] = b.value
        sizes["imq"] = _lib.imq_workspace_bytes(n, d)
        sizes["imq_ksd"] = _lib.imq_ksd_workspace_bytes(n, d)
        ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        calls = {
            "stream": lambda: par.stein_svgd_phi_stream(p(T), p(G), n, d, _lib.F32, p(h2), p(phi), p(sums), p(ws), sizes["stream"], 0, stream),
            "stream_this": lambda: new.stein_svgd_phi_stream(p(T), p(G), n, d, _lib.F32, p(h2), p(phi), p(sums), p(ws), sizes["stream"], 0, stream),
            "imq": lambda: new.stein_svgd_phi_imq(p(T), p(G), n, d, _lib.F32, p(h2), p(phi), p(sums), p(ws), sizes["imq"], 0, stream),
            "stream_ksd": lambda: par.stein_svgd_phi_stream_ksd(p(T), p(G), n, d, _lib.F32, p(h2), p(phi), p(sums), p(ws), sizes["stream_ksd"], 0, stream),
            "imq_ksd": lambda: new.stein_svgd_phi_imq_ksd(p(T), p(G), n, d, _lib.F32, p(h2), p(phi), p(sums), p(ws), sizes["imq_ksd"], 0, stream),
        }
        if only:
            calls = {k: v for k, v in calls.items() if k in only}
        for name, f in calls.items():
            for _ in range(10):
                rc = f()
                assert rc == 0, (name, rc)
            torch.cuda.synchronize()
            assert torch.isfinite(phi).all() and torch.isfinite(sums).all(), name
        ms = {k: [] for k in calls}
        count = {}
        for name, f in calls.items():          # windows of at least a quarter of a second, at least `steps` calls
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                f()
            torch.cuda.synchronize()
            count[name] = max(steps, int(0.25 / ((time.perf_counter() - t0) / 20)) + 1)
        for _ in range(reps):
            for name, f in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(count[name]):
                    f()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / count[name])
        say("%d x %d  IMQ plan (row tiles, column blocks, j ranges) %s; RBF streaming plan %s" %
            (n, d, _lib.imq_plan(n, d), _lib.stream_plan(n, d)))
        med = {}
        for name in calls:
            v = sorted(ms[name])
            med[name] = v[len(v) // 2]
            say("  %-11s %5d calls per round, ms per round %s  median %.4f  spread %.1f %%  workspace %.1f MiB" %
                (name, count[name], ["%.4f" % x for x in ms[name]], med[name], 100.0 * (v[-1] - v[0]) / med[name],
                 sizes[name.replace("_this", "")] / 2.0 ** 20))
        if "imq" in med and "stream" in med:
            say("  imq / stream x %.2f;  imq_ksd / stream_ksd x %.2f" % (med["imq"] / med["stream"], med["imq_ksd"] / med["stream_ksd"]))
    if out:
        out.close()


if __name__ == "__main__":
    if "--imq-only" in sys.argv:
        at = sys.argv.index("--imq-only")
        main([(int(sys.argv[at + 1]), int(sys.argv[at + 2]))], reps=1, steps=60, only=("imq",))
    else:
        if not _opt("--parent-lib"):
            sys.exit("--parent-lib PATH: a libsteinhip.so built from the parent commit")
        main([(4096, 256), (16384, 256), (8192, 2001)])
