"""Measurements of the Stein-kernel products and the Stein importance weights (the output is
profiles/weights_ab.txt).

    python scratch/weights_ab.py [--parent-lib PATH] [--shapes 4096x256,...] [--rounds 5] [--out FILE]

--parent-lib: a libsteinhip.so built from the parent commit; stein_ksd_boot and stein_thin are then timed from both
libraries, alternated round by round in one process, and their outputs compared bit for bit.
Every figure is the median over --rounds rounds (min .. max beside it); a round repeats the call until a quarter of a second has
passed (at least once), between two device synchronisations, and the variants of one comparison take turns round by round.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from stein_amd import _lib  # noqa: E402

IMQ = _lib.KERNEL_IMQ
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def open_lib(path):
    lib = ctypes.CDLL(path)
    for name in ("stein_ksd_boot", "stein_ksd_boot_workspace_bytes", "stein_thin", "stein_thin_workspace_bytes"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib._SIGNATURES[name], ctypes.c_int
    return lib


def alternated(variants, rounds, min_s=0.25):
    """{name: fn} -> {name: (median ms per call, min, max)}; the variants take turns round by round"""
    for fn in variants.values():      # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            calls = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while True:
                fn()
                calls += 1
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= min_s:
                    break
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ms.items()}


def fmt(r):
    return "%9.4f ms (%.4f .. %.4f)" % r


def torch_pairwise_u(X, G, h2):
    """the IMQ Stein-kernel matrix [n, n] in torch, fp32, from Gram products"""
    d = X.shape[1]
    c2 = 2.0 * h2
    r, a = (X * X).sum(1), (G * X).sum(1)
    XX, GX = X @ X.T, G @ X.T
    D = (r[:, None] + r[None, :] - 2.0 * XX).clamp_min_(0.0)
    cross = a[:, None] + a[None, :] - GX - GX.T
    k = torch.rsqrt(1.0 + D / c2)
    k3 = k * k * k
    return k * (G @ G.T) + k3 * cross / c2 + d * k3 / c2 - 3.0 * k3 * k * k * D / (c2 * c2)


def torch_frank_wolfe(X, G, h2, iters):
    """the same Frank-Wolfe loop in torch on the device: no n x n matrix beyond g_0's (formed in row blocks), no host read
    -> (w, idx, gamma)"""
    n, d = X.shape
    c2 = 2.0 * h2
    r, a = (X * X).sum(1), (G * X).sum(1)
    g2 = (G * G).sum(1).double() + d / c2
    w = torch.full((n,), 1.0 / n, dtype=torch.float64, device=X.device)
    g = torch.empty(n, dtype=torch.float64, device=X.device)
    for i0 in range(0, n, 2048):
        Xi, Gi = X[i0:i0 + 2048], G[i0:i0 + 2048]
        D = (r[i0:i0 + 2048, None] + r[None, :] - 2.0 * Xi @ X.T).clamp_min_(0.0)
        cross = a[i0:i0 + 2048, None] + a[None, :] - Gi @ X.T - Xi @ G.T
        k = torch.rsqrt(1.0 + D / c2)
        k3 = k * k * k
        g[i0:i0 + 2048] = (k * (Gi @ G.T) + k3 * cross / c2 + d * k3 / c2 - 3.0 * k3 * k * k * D / (c2 * c2)).double().mean(1)
    idx = torch.empty(iters, dtype=torch.int64, device=X.device)
    gam = torch.empty(iters, dtype=torch.float64, device=X.device)
    zero, one = torch.zeros((), dtype=torch.float64, device=X.device), torch.ones((), dtype=torch.float64, device=X.device)
    for t in range(iters):
        s = g.argmin().view(1)
        f, gs = (w * g).sum(), g.index_select(0, s)[0]
        num, den = f - gs, f - 2.0 * gs + g2.index_select(0, s)[0]
        gamma = torch.where((num > 0) & (den > 0), torch.minimum(one, num / den), zero)
        idx[t:t + 1], gam[t] = s, gamma
        B = torch.cat([X.index_select(0, s), G.index_select(0, s)], 0).T           # [d, 2] = [x_s | g_s]
        XB, GB = X @ B, G @ B
        D = (r + r.index_select(0, s) - 2.0 * XB[:, 0]).clamp_min(0.0)
        cross = a + a.index_select(0, s) - XB[:, 1] - GB[:, 0]
        k = torch.rsqrt(1.0 + D / c2)
        k3 = k * k * k
        u = k * GB[:, 1] + k3 * cross / c2 + d * k3 / c2 - 3.0 * k3 * k * k * D / (c2 * c2)
        g = (1.0 - gamma) * g + gamma * u.double()
        w = (1.0 - gamma) * w
        w.index_add_(0, s, gamma.view(1))
    return w, idx, gam


def products(args, parent, n, d):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(n + d)
    X = (1.3 * torch.randn(n, d, device=dev, generator=gen) + 0.5).contiguous()
    G = -X
    h2 = 0.5 * d
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=dev)
    lib = _lib.load()
    for reps in (1, 256):
        V = torch.randn(reps, n, device=dev, generator=gen)
        V[0] = 1.0
        out = torch.empty(reps, n, device=dev)
        q = torch.empty(reps, dtype=torch.float64, device=dev)
        ws_m = torch.empty(_lib.ksd_matmul_workspace_bytes(n, d, reps), dtype=torch.uint8, device=dev)
        ws_b = torch.empty(_lib.ksd_boot_workspace_bytes(n, d, reps), dtype=torch.uint8, device=dev)

        def boot(which, dst):
            rc = which.stein_ksd_boot(P(X), P(G), n, d, _lib.F32, P(h2_t), IMQ, P(V), reps, P(dst), None, P(ws_b), ws_b.numel(), 0, None)
            assert rc == 0, rc

        def matmul():
            rc = lib.stein_ksd_matmul(P(X), P(G), n, d, _lib.F32, P(h2_t), IMQ, P(V), reps, P(out), P(ws_m), ws_m.numel(), 0, None)
            assert rc == 0, rc
        variants = {"stein_ksd_matmul": matmul, "stein_ksd_boot (this)": lambda: boot(lib, q)}
        if parent is not None:
            q_par = torch.empty_like(q)
            variants["stein_ksd_boot (parent)"] = lambda: boot(parent, q_par)
        if n * n * 4 <= 1 << 30:
            variants["torch pairwise U @ V.T"] = lambda: torch_pairwise_u(X, G, h2) @ V.T
        res = alternated(variants, args.rounds)
        say("%7d x %4d, reps %3d:" % (n, d, reps))
        for k, r in res.items():
            say("    %-26s %s" % (k, fmt(r)))
        if parent is not None:
            say("    stein_ksd_boot: this / parent %.4f; q_out bit-identical: %s" %
                (res["stein_ksd_boot (this)"][0] / res["stein_ksd_boot (parent)"][0], bool(torch.equal(q, q_par))))
        if "torch pairwise U @ V.T" in res:
            ref = (torch_pairwise_u(X, G, h2).double() @ V.T.double()).T
            say("    products against the torch fp64 contraction of the fp32 matrix: largest |diff| / largest |out| %.3g; "
                "torch / ours %.2fx" % (float((out.double() - ref).abs().max() / ref.abs().max()),
                                         res["torch pairwise U @ V.T"][0] / res["stein_ksd_matmul"][0]))


def weights(args, parent, n, d):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(n + d)
    X = (1.3 * torch.randn(n, d, device=dev, generator=gen) + 0.5).contiguous()
    G = -X
    h2 = 0.5 * d
    h2_t = torch.full((1,), h2, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = torch.empty(_lib.weights_workspace_bytes(n, d), dtype=torch.uint8, device=dev)
    ws_t = torch.empty(_lib.thin_workspace_bytes(n, d), dtype=torch.uint8, device=dev)
    w, stats = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)

    def run(iters, idx=None, gam=None):
        rc = lib.stein_weights(P(X), P(G), n, d, _lib.F32, P(h2_t), IMQ, iters, P(w), P(stats), P(idx), P(gam), P(ws), ws.numel(), 0, None)
        assert rc == 0, rc

    def thin(which, m, idx, ksd2):
        rc = which.stein_thin(P(X), P(G), n, d, _lib.F32, P(h2_t), IMQ, m, P(idx), P(ksd2), P(ws_t), ws_t.numel(), 0, None)
        assert rc == 0, rc
    # a step count that fills a quarter of a second, from a first estimate
    run(64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(256)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 256
    K = int(min(20000, max(256, 0.3 / per)))
    ti, tk = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.float64, device=dev)
    variants = {"weights, K steps": lambda: run(K), "weights, 0 steps": lambda: run(0), "thin (this), K picks": lambda: thin(lib, K, ti, tk)}
    if parent is not None:
        pi, pk = torch.empty_like(ti), torch.empty_like(tk)
        variants["thin (parent), K picks"] = lambda: thin(parent, K, pi, pk)
    res = alternated(variants, args.rounds)
    step = [(a - b) / K for a, b in zip(res["weights, K steps"], (res["weights, 0 steps"][0],) * 3)]
    moved = 8.0 * n * d + 32.0 * n
    say("%7d x %4d, K = %d:" % (n, d, K))
    say("    stein_weights per step      %9.4f ms (%.4f .. %.4f)  [(K steps - 0 steps) / K; 0 steps = two products + finish: %s]"
        % (step[0], step[1], step[2], fmt(res["weights, 0 steps"])))
    say("    %.1f GB/s over the 8 n d + 32 n = %.3g bytes a step moves; at 8 TB/s they take %.4f ms: the step is %.1fx that" %
        (moved / (step[0] * 1e-3) / 1e9, moved, moved / 8e12 * 1e3, step[0] / (moved / 8e12 * 1e3)))
    say("    stein_thin per pick (this)  %9.4f ms (%.4f .. %.4f)" % tuple(x / K for x in res["thin (this), K picks"]))
    if parent is not None:
        say("    stein_thin per pick (parent)%9.4f ms (%.4f .. %.4f); this / parent %.4f; picks and ksd2 bit-identical: %s" %
            (tuple(x / K for x in res["thin (parent), K picks"]) +
             (res["thin (this), K picks"][0] / res["thin (parent), K picks"][0], bool(torch.equal(ti, pi) and torch.equal(tk, pk)))))
    if not args.no_torch:
        Kt = min(K, 512)
        gi, gg = torch.empty(Kt, dtype=torch.int64, device=dev), torch.empty(Kt, dtype=torch.float64, device=dev)
        got = []
        tv = alternated({"torch": lambda: got.__setitem__(slice(None), [torch_frank_wolfe(X, G, h2, Kt)]),
                         "torch0": lambda: torch_frank_wolfe(X, G, h2, 0), "ours": lambda: run(Kt, gi, gg), "ours0": lambda: run(0)},
                        max(2, args.rounds // 2))
        t_step, o_step = (tv["torch"][0] - tv["torch0"][0]) / Kt, (tv["ours"][0] - tv["ours0"][0]) / Kt
        same = (got[0][1] == gi)
        first = int(same.long().cumprod(0).sum())
        say("    torch loop per step         %9.4f ms over %d steps (ours over the same %d: %.4f ms): torch / ours %.2fx;"
            " vertices equal %.3f, the first %d all equal; largest |gamma diff| over those %.2e" %
            (t_step, Kt, Kt, o_step, t_step / o_step, float(same.double().mean()), first,
             float((got[0][2][:first] - gg[:first]).abs().max()) if first else 0.0))


def decisive_cases():
    """the torch loop on the four specified cases of the tests: the same vertices as the library on every decisive step"""
    import weights_cases as C
    dev = torch.device("cuda")
    lib = _lib.load()
    for c in C.PATH_CASES:
        r = C.reference(c.name)
        if c.kernel != "imq":
            continue
        X, G = torch.from_numpy(r.X).to(dev), torch.from_numpy(r.G).to(dev)
        n, d = r.X.shape
        h2_t = torch.full((1,), r.h2, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.weights_workspace_bytes(n, d), dtype=torch.uint8, device=dev)
        w, stats = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
        gi, gg = torch.empty(c.iters, dtype=torch.int64, device=dev), torch.empty(c.iters, dtype=torch.float64, device=dev)
        rc = lib.stein_weights(P(X), P(G), n, d, _lib.F32, P(h2_t), IMQ, c.iters, P(w), P(stats), P(gi), P(gg), P(ws), ws.numel(), 0, None)
        assert rc == 0
        _, ti, tg = torch_frank_wolfe(X, G, r.h2, c.iters)
        dec = torch.from_numpy(r.forced.decisive).to(dev)
        say("    %s: torch loop and library agree on %d of %d decisive steps (%d of %d steps in all)" %
            (c.name, int((ti == gi)[dec].sum()), int(dec.sum()), int((ti == gi).sum()), c.iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shapes", default="4096x256,16384x256,8192x2001,262144x16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only", default="products,weights,cases")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs a GPU")
    parent = open_lib(args.parent_lib) if args.parent_lib else None
    say("%s; IMQ kernel, X = 1.3 z + 0.5, score -X, fixed bandwidth h2 = d / 2; rounds of >= 0.25 s, %d per variant, alternated;"
        " median (min .. max)" % (torch.cuda.get_device_name(0), args.rounds))
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    try:
        if "products" in args.only:
            say("== Stein-kernel products: ms per call")
            for n, d in shapes:
                products(args, parent, n, d)
        if "weights" in args.only:
            say("== Stein importance weights: ms per Frank-Wolfe step")
            for n, d in shapes:
                weights(args, parent, n, d)
        if "cases" in args.only:
            say("== the torch loop on the tests' specified cases (IMQ)")
            decisive_cases()
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
