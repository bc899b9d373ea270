"""Bit identity and same-box timing of the four streaming step entry points (stein_svgd_phi_stream{,_ksd},
stein_svgd_phi_imq{,_ksd}) and stein_stream_median between library builds, at the C ABI, every library in a process of its
own (profiles/stream_imq_shared_ab.txt; the method of profiles/contraction_one_geometry_ab.txt).

    python scratch/stream_imq_shared_ab.py --libs parentA=PATH parentB=PATH new=PATH [--out FILE] [--rounds 5]

The first library is the reference of the bit comparison; the spread between the libraries named parent* is the tolerance of
the timing.  Each worker process runs under a time limit and the driver stops at the first worker that does not exit 0.

    python scratch/stream_imq_shared_ab.py --worker LIB --dump FILE      one library's outputs of every identity case
    python scratch/stream_imq_shared_ab.py --worker LIB --time [--shape NxD]     one timing round, one JSON line"""
import ctypes
import json
import math
import os
import subprocess
import sys
import time

F32 = 0
vp, i64, sz, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
STEP = [vp, vp, i64, i64, ci, vp, vp, vp, vp, sz, ci, vp]
STEPS = {"stream": ("stein_svgd_phi_stream", "stein_stream_workspace_bytes", 1),
         "stream_ksd": ("stein_svgd_phi_stream_ksd", "stein_stream_ksd_workspace_bytes", 3),
         "imq": ("stein_svgd_phi_imq", "stein_imq_workspace_bytes", 1),
         "imq_ksd": ("stein_svgd_phi_imq_ksd", "stein_imq_ksd_workspace_bytes", 3)}
TIMED_SHAPES = [(4096, 256), (16384, 256), (8192, 2001)]


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def load(path):
    lib = ctypes.CDLL(path)
    for fn, wsfn, _ in STEPS.values():
        getattr(lib, fn).argtypes = STEP
        getattr(lib, wsfn).argtypes = [i64, i64, ci, ci, ctypes.POINTER(sz)]
    lib.stein_stream_median_workspace_bytes.argtypes = [i64, i64, ci, ci, ctypes.POINTER(sz)]
    lib.stein_stream_median.argtypes = [vp, i64, i64, ci, vp, vp, vp, sz, ci, vp]
    lib.stein_debug_stream_jsplit.argtypes = [ci]
    lib.stein_last_error.restype = ctypes.c_char_p
    return lib


def ws_bytes(lib, fn, n, d):
    b = sz(0)
    rc = getattr(lib, fn)(n, d, F32, 0, ctypes.byref(b))
    assert rc == 0, (fn, n, d, rc)
    return b.value


def off4(torch, x):
    """x's values in storage that starts 4 bytes past a 16-byte boundary"""
    buf = torch.zeros(x.numel() + 4, dtype=x.dtype, device=x.device)
    y = buf[1:1 + x.numel()].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 == 4
    return y


def worker_dump(lib, path):
    import torch
    dev = torch.device("cuda:0")
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    out = {}

    def p(t):
        return vp(t.data_ptr()) if t is not None else vp(None)

    def inputs(n, d):
        gen = torch.Generator(device="cpu").manual_seed(1000 * n + d)
        return torch.randn(n, d, generator=gen).to(dev), torch.randn(n, d, generator=gen).to(dev)

    def step(tag, name, T, G, h2, phi_mode="own", jsplit=0):
        n, d = T.shape
        fn, wsfn, nsum = STEPS[name]
        assert lib.stein_debug_stream_jsplit(jsplit) == 0
        nb = ws_bytes(lib, wsfn, n, d)
        ws = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        sums = torch.zeros(nsum, dtype=torch.float64, device=dev)
        phi = None if phi_mode == "null" else torch.zeros(n, d, device=dev)
        if phi_mode == "off4":
            phi = off4(torch, phi)
        rc = getattr(lib, fn)(p(T), p(G), n, d, F32, p(h2), p(phi), p(sums), p(ws), nb, 0, stream)
        assert rc == 0, (tag, name, rc, lib.stein_last_error())
        torch.cuda.synchronize()
        assert lib.stein_debug_stream_jsplit(0) == 0
        if phi is not None:
            out["%s %s phi" % (tag, name)] = phi.cpu().clone()
        out["%s %s sums" % (tag, name)] = sums.cpu()

    for n, d in [(2, 1), (129, 129), (150, 37), (300, 260), (384, 513), (1536, 256)]:
        T, G = inputs(n, d)
        h2 = torch.full((1,), 2.0 * d / math.log(n), dtype=torch.float32, device=dev)
        for name in STEPS:
            step("%dx%d" % (n, d), name, T, G, h2)
        # the streaming median, then the RBF step at the bandwidth it left on the device
        nb = ws_bytes(lib, "stein_stream_median_workspace_bytes", n, d)
        ws = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        hm, med = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        rc = lib.stein_stream_median(p(T), n, d, F32, p(hm), p(med), p(ws), nb, 0, stream)
        assert rc == 0, ("median", n, d, rc, lib.stein_last_error())
        torch.cuda.synchronize()
        out["%dx%d median h2" % (n, d)] = hm.cpu()
        out["%dx%d median median" % (n, d)] = med.cpu()
        step("%dx%d h2=median" % (n, d), "stream", T, G, hm)
    T, G = inputs(700, 300)
    h2 = torch.full((1,), 2.0 * 300 / math.log(700), dtype=torch.float32, device=dev)
    for js in (1, 2, 3):
        for name in STEPS:
            step("700x300 jsplit=%d" % js, name, T, G, h2, jsplit=js)
    for name in STEPS:
        step("700x300", name, T, G, h2)
    # the scalar finish chosen by alignment (d % 4 == 0), the KSD forms without phi and with a score off the 16 bytes
    for n, d in [(300, 260), (1536, 256)]:
        T, G = inputs(n, d)
        h2 = torch.full((1,), 2.0 * d / math.log(n), dtype=torch.float32, device=dev)
        for name in STEPS:
            step("%dx%d theta+4" % (n, d), name, off4(torch, T), G, h2)
            step("%dx%d phi+4" % (n, d), name, T, G, h2, phi_mode="off4")
        for name in ("stream_ksd", "imq_ksd"):
            step("%dx%d phi=NULL" % (n, d), name, T, G, h2, phi_mode="null")
            step("%dx%d score+4" % (n, d), name, T, off4(torch, G), h2)
            step("%dx%d score+4 phi=NULL" % (n, d), name, T, off4(torch, G), h2, phi_mode="null")
    torch.save(out, path)
    print("dumped %d tensors" % len(out), flush=True)


def worker_time(lib):
    import torch
    dev = torch.device("cuda:0")
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    res = {}
    only = _opt("--shape")   # e.g. 16384x256: that shape alone, for a profiler run of its own
    for n, d in [tuple(int(x) for x in only.split("x"))] if only else TIMED_SHAPES:
        gen = torch.Generator(device="cpu").manual_seed(0)
        T = torch.randn(n, d, generator=gen).to(dev)
        G = torch.randn(n, d, generator=gen).to(dev)
        h2 = torch.full((1,), 2.0 * d / math.log(n), dtype=torch.float32, device=dev)
        phi = torch.empty(n, d, device=dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        sizes = {name: ws_bytes(lib, STEPS[name][1], n, d) for name in STEPS}
        ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
        a = [vp(x.data_ptr()) for x in (T, G, h2, phi, sums, ws)]
        for name in STEPS:
            fn = getattr(lib, STEPS[name][0])

            def f():
                return fn(a[0], a[1], n, d, F32, a[2], a[3], a[4], a[5], sizes[name], 0, stream)
            for _ in range(10):
                assert f() == 0, (name, lib.stein_last_error())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                f()
            torch.cuda.synchronize()
            count = max(50, int(0.25 / ((time.perf_counter() - t0) / 20)) + 1)   # a quarter of a second
            t0 = time.perf_counter()
            for _ in range(count):
                f()
            torch.cuda.synchronize()
            res["%dx%d %s" % (n, d, name)] = (time.perf_counter() - t0) * 1e3 / count
    print("RESULT " + json.dumps(res), flush=True)


def run(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit("worker %s exited %d; nothing further is started\n%s\n%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return r.stdout


def driver():
    import torch
    at = sys.argv.index("--libs")
    libs = []
    for a in sys.argv[at + 1:]:
        if a.startswith("--"):
            break
        libs.append(a.split("=", 1))
    rounds = int(_opt("--rounds", "5"))
    outf = open(_opt("--out"), "a") if _opt("--out") else None
    tmp = _opt("--tmp", "/tmp")

    def say(s):
        print(s, flush=True)
        if outf:
            outf.write(s + "\n")
            outf.flush()
    # ---- bit identity against the first library
    dumps = {}
    for name, path in libs:
        f = os.path.join(tmp, "stream_imq_shared_%s_%d.pt" % (name, os.getpid()))
        run(["--worker", path, "--dump", f], 240)
        dumps[name] = torch.load(f)
        os.remove(f)
    ref_name = libs[0][0]
    ref = dumps[ref_name]
    for name, _ in libs[1:]:
        got = dumps[name]
        assert sorted(got) == sorted(ref)
        differ = [k for k in sorted(ref) if ref[k].shape != got[k].shape or
                  not torch.equal(ref[k].contiguous().view(torch.uint8), got[k].contiguous().view(torch.uint8))]
        say("identity %s against %s: %d tensors compared, %d differ%s" %
            (name, ref_name, len(ref), len(differ), "".join("\n    " + k for k in differ)))
    # ---- timing: every library in its own process, alternated, rotating start
    ms = {name: {} for name, _ in libs}
    for r in range(rounds):
        order = libs[r % len(libs):] + libs[:r % len(libs)]
        for name, path in order:
            line = [x for x in run(["--worker", path, "--time"], 300).splitlines() if x.startswith("RESULT ")][-1]
            for k, v in json.loads(line[7:]).items():
                ms[name].setdefault(k, []).append(v)
            say("round %d %-8s %s" % (r, name, "  ".join("%s %.4f" % (k, v[-1]) for k, v in ms[name].items())))
    parents = [name for name, _ in libs if name.startswith("parent")]
    say("medians of %d rounds, ms per call; in = the median lies inside [min, max] of all rounds of %s" % (rounds, " and ".join(parents)))
    for k in ms[libs[0][0]]:
        lo = min(min(ms[p][k]) for p in parents)
        hi = max(max(ms[p][k]) for p in parents)
        row = "  %-22s" % k
        for name, _ in libs:
            v = sorted(ms[name][k])
            row += "  %s %.4f (%.4f - %.4f)" % (name, v[len(v) // 2], v[0], v[-1])
            if name not in parents:
                med = v[len(v) // 2]
                row += "  %s  %+.2f %% against the parents' mid-range" % ("in" if lo <= med <= hi else "OUT", 100.0 * (med / (0.5 * (lo + hi)) - 1.0))
        say(row + "  parents' range %.4f - %.4f" % (lo, hi))
    if outf:
        outf.close()


if __name__ == "__main__":
    if "--worker" in sys.argv:
        import torch  # noqa: F401  (before the library: both then share the HIP runtime torch loads)
        lib = load(_opt("--worker"))
        if "--dump" in sys.argv:
            worker_dump(lib, _opt("--dump"))
        else:
            worker_time(lib)
    elif "--libs" in sys.argv:
        driver()
    else:
        sys.exit(__doc__)
