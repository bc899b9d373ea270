"""Host time per compute_phi of a streaming engine and of the default stored-D engine between source trees, every tree in a
process of its own, alternated (profiles/engine_split_ab.txt).  The GPU work is the same library's in every tree; the shape
is small enough (256 x 16) that the host's time per call is what a loop of calls followed by one synchronise measures;
"issue only" stops the clock before the synchronise.

    python scratch/engine_split_ab.py --trees parentA=DIR parentB=DIR new=DIR [--out FILE] [--rounds 4] [--calls 4000]

DIR holds a stein_amd package with its built library.  The trees named parent* are the parent's own code (the same DIR
twice will do).  A tree's figure is the MINIMUM over its rounds: on a shared host a disturbance only ever adds time, and the
processes fall into two modes some 6 us apart whatever the tree, so a mean of a few rounds measures the mix of modes and the
minimum the code.  The verdict: the figure of every other tree is no larger than the larger of the parent trees' two figures
(exit 1 if it is).  Means and medians are printed beside it.  Each worker runs under a time limit and the driver stops at the
first worker that does not exit 0 (exit 2).

    python scratch/engine_split_ab.py --worker DIR [--calls 4000]      one round of both engines, one JSON line"""
import json
import os
import subprocess
import sys
import time

N, D = 256, 16
ENGINES = {"streaming (h2=1.5)": {"h2": 1.5}, "stored-D (defaults)": {}}


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def worker(root, calls):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from stein_amd.engine import SvgdEngine
    gen = torch.Generator().manual_seed(0)
    T, G = (torch.randn(N, D, generator=gen).cuda() for _ in range(2))
    out = {}
    for label, kw in ENGINES.items():
        eng = SvgdEngine(N, D, device="cuda", **kw)
        for _ in range(calls // 10):
            eng.compute_phi(T, G)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            eng.compute_phi(T, G)
        t1 = time.perf_counter()        # every call issued: the host's own time, unless the queue filled up and made it wait
        torch.cuda.synchronize()
        out[label] = (time.perf_counter() - t0) / calls * 1e6
        out[label + ", issue only"] = (t1 - t0) / calls * 1e6
        out[label + " |phi|^2"] = float(eng.sqnorm.item())
    print(json.dumps(out))


def main():
    if "--worker" in sys.argv:
        return worker(_opt("--worker"), int(_opt("--calls", "4000")))
    trees = [a.split("=", 1) for a in sys.argv[sys.argv.index("--trees") + 1:] if "=" in a and not a.startswith("--")]
    rounds, calls = int(_opt("--rounds", "4")), _opt("--calls", "4000")
    outf = open(_opt("--out"), "w") if _opt("--out") else None

    def say(line):
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()

    say("host time per compute_phi, us (%d x %d, %s calls then one synchronise; %d rounds, trees alternated)" % (N, D, calls, rounds))
    runs = {name: [] for name, _ in trees}
    for r in range(rounds):
        for name, root in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, "--calls", calls],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                say("worker %s failed (exit %d): %s" % (name, p.returncode, p.stderr[-2000:]))
                return 2
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    verdict = 0
    for label in [e + suffix for e in ENGINES for suffix in ("", ", issue only")]:
        say("")
        say(label)
        limit = max(min(x[label] for x in runs[name]) for name in runs if name.startswith("parent"))
        sums = {x[label.split(",")[0] + " |phi|^2"] for name in runs for x in runs[name]}
        for name in runs:
            v = [x[label] for x in runs[name]]
            note = "" if name.startswith("parent") else "   within the parent's" if min(v) <= limit else "   ABOVE the parent's"
            verdict |= "ABOVE" in note
            say("  %-8s min %6.2f  median %6.2f  mean %6.2f   rounds %s%s" %
                (name, min(v), sorted(v)[len(v) // 2], sum(v) / len(v), " ".join("%6.2f" % x for x in v), note))
        say("  the larger of the parent's minima %.2f; |phi|^2 %s" %
            (limit, "the same bits in every run" if len(sums) == 1 else "DIFFERS: %s" % sorted(sums)))
        verdict |= len(sums) != 1
    return verdict


if __name__ == "__main__":
    sys.exit(main())
