"""What a workspace holds between two calls, and the yardstick a call is held to whatever it held (a helper of
test_gpu_workspace_state.py and test_workspace_layout.py, not a test).

include/steinhip.h promises that a step's result is the same "for any workspace contents", that only the SELECT section
persists from one fused call to the next, and that one workspace serves call after call.  The helpers here make the
contents hostile (poison), produce the one right answer (fresh_result: a new engine, a zeroed workspace, one call) and the
inputs that change from call to call (input_sequence), and drive the paths that have no SvgdEngine of their own (the
row blocks through stein_rank_*, the fused call at the ABI).

    zeros     0x00 bytes: the baseline
    ones      0xFF bytes: NaN as fp32, fp16 and bf16, -1 as an integer, a huge count
    large     0x7B bytes: about 1.3e36 as fp32 and 6.1e4 as fp16, finite: an unwritten value that meets an exact zero
              factor stays hidden under NaN-free arithmetic, but shows wherever it is added
    leftover  the workspace of the same configuration after a complete step on unrelated inputs (another seed, theta
              times 2^5, the score times 2^-3): plausible, wrong values
"""
import os
import re

import numpy as np
import torch

import conditioning_inputs as ci
from stein_amd import _lib
from stein_amd.engine import HipStages, SvgdEngine, untile_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_BYTES = {"zeros": 0x00, "ones": 0xFF, "large": 0x7B}
PATTERNS = ("zeros", "ones", "large", "leftover")


def spec_magic_words():
    """SPEC_MAGIC1 / SPEC_MAGIC2 as stein_common.h spells them: the words that make the fused call trust the predictor
    state of the SELECT section"""
    with open(os.path.join(ROOT, "stein_amd", "csrc", "stein_common.h")) as f:
        m = re.search(r"SPEC_MAGIC1\s*=\s*0x([0-9A-Fa-f]+)u\s*,\s*SPEC_MAGIC2\s*=\s*0x([0-9A-Fa-f]+)u", f.read())
    assert m, "stein_common.h no longer defines SPEC_MAGIC1 / SPEC_MAGIC2 on one line"
    return int(m.group(1), 16), int(m.group(2), 16)


def pattern_can_forge_magic(byte):
    """a section filled with one byte holds the word byte * 0x01010101 everywhere"""
    return byte * 0x01010101 in spec_magic_words()


def _sections(eng):
    """the (workspace, offsets) pairs of an engine: one, or one per row block"""
    return [(b.ws, b._offs) for b in eng.blocks] if hasattr(eng, "blocks") else [(eng.ws, eng._offs)]


def poison(eng, pattern, keep_select, leftover=None):
    """Overwrite every byte of eng.ws (of every block's workspace for RankBlocks); keep_select=True leaves the
    SELECT_BYTES of the SELECT section alone.  `leftover`: what leftover_of(...) returned, for that pattern."""
    pairs = _sections(eng)
    donors = leftover if isinstance(leftover, (list, tuple)) else [leftover] * len(pairs)
    for (ws, offs), donor in zip(pairs, donors):
        o = offs[_lib.WS_SELECT]
        saved = ws[o:o + _lib.SELECT_BYTES].clone() if keep_select else None
        if pattern in PATTERN_BYTES:
            # keep_select=False: the predictor restarts only if SpecState::magic is neither SPEC_MAGIC1 nor SPEC_MAGIC2
            # (stein_common.h).  A one-byte pattern repeats its byte four times in every word and the magic words do not:
            # checked against the header, so that a new magic word cannot make this poison a valid state by accident.
            assert keep_select or not pattern_can_forge_magic(PATTERN_BYTES[pattern]), pattern
            ws.fill_(PATTERN_BYTES[pattern])
        elif pattern == "leftover":
            assert donor is not None and donor.numel() == ws.numel(), "leftover needs the donor workspace of leftover_of()"
            ws.copy_(donor)
            if not keep_select:
                # the donor's SELECT section is a genuine predictor state WITH its magic word: that one pattern would be
                # trusted, as the header says it is.  The section gets zeros instead.
                ws[o:o + _lib.SELECT_BYTES].zero_()
        else:
            raise ValueError(pattern)
        if keep_select:
            ws[o:o + _lib.SELECT_BYTES].copy_(saved)


# ---------------------------------------------------------------------------------------------------------------
# inputs that change from call to call
# ---------------------------------------------------------------------------------------------------------------
THETA_EXP = (0, 3, -2, 2, -3, 1, -1, 4)      # theta times 2^a: h2 moves by 4^(difference) >= 16 between neighbours
SCORE_EXP = (0, -5, 7, -1, 4, -6, 2, -3)
FAMILY_STEP = 2                               # this step's values come from conditioning_inputs


def family_of(n, d):
    """the conditioning_inputs family of a sequence's FAMILY_STEP (zero_const needs three columns)"""
    return "graded" if d < 3 or (n + d) % 2 == 0 else "zero_const"


def input_sequence(n, d, seed, steps=5, drift=0):
    """`steps` seeded (theta, score) pairs as fp64 arrays of fp32 values, every one with its own draws and its own
    power-of-two scales (THETA_EXP, SCORE_EXP), so that neither the operand planes nor anything derived from h2 (W and
    its scales) can survive from the call before unnoticed; step FAMILY_STEP is conditioning_inputs' `graded` or
    `zero_const`.  Then `drift` steps in which theta grows by a thousandth per step under fresh scores: the median
    moves as it does in a run, so the speculative window has something to hit."""
    out = []
    for k in range(steps):
        a, b = THETA_EXP[k % len(THETA_EXP)], SCORE_EXP[k % len(SCORE_EXP)]
        if k == FAMILY_STEP:
            T, G = ci.make(family_of(n, d), n, d, seed)
        else:
            rng = np.random.default_rng([seed, k, n, d])
            T, G = ci.f32(rng.normal(size=(n, d))), ci.f32(rng.normal(size=(n, d)))
        T, G = T * 2.0 ** a, G * 2.0 ** b
        assert np.array_equal(ci.f32(T), T) and np.array_equal(ci.f32(G), G)
        out.append((T, G))
    for j in range(drift):
        rng = np.random.default_rng([seed, 1000 + j, n, d])
        T = ci.f32(out[-1][0] * 1.001)
        out.append((T, ci.f32(rng.normal(size=(n, d))) * 2.0 ** SCORE_EXP[j % len(SCORE_EXP)]))
    return out


def unrelated_inputs(n, d, seed):
    """the donor step of the `leftover` pattern"""
    rng = np.random.default_rng([seed + 7919, n, d, 5])
    return ci.f32(rng.normal(size=(n, d))) * 2.0 ** 5, ci.f32(rng.normal(size=(n, d))) * 2.0 ** -3


def to_device(x, device, dtype=torch.float32):
    return torch.tensor(x, dtype=torch.float32, device=device).to(dtype).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# one call and everything it leaves
# ---------------------------------------------------------------------------------------------------------------
def scrub_outputs(eng):
    """NaN into what a call must write: a call that skips an output must not find the previous call's there"""
    eng.phi.fill_(float("nan"))
    eng.h2.fill_(float("nan"))
    eng._sums[:3 if eng.ksd else 1].fill_(float("nan"))


def engine_call(eng, T, G, dK=False, K=False, staged=False, extra=None):
    """one compute_phi -> dict of clones: phi, h2, sums, D (unless the one-kernel path ran), dK and K where asked, and
    what extra(eng) adds (a dict of tensors read from the engine after the call, e.g. its operand planes)"""
    n, d, dev = eng.n, eng.d, eng.device
    dK_out = torch.full((n, d), float("nan"), device=dev) if dK else None
    K_out = torch.full((n, n), float("nan"), device=dev) if K else None
    scrub_outputs(eng)
    eng.compute_phi(T, G, K_out=K_out, dK_out=dK_out, **({"mark": lambda s: None} if staged else {}))
    torch.cuda.synchronize()
    res = dict(phi=eng.phi.clone(), h2=eng.h2.clone(), sums=eng._sums.clone())
    if eng._have_dist:
        res["D"] = eng.dist_matrix()
    if dK:
        res["dK"] = dK_out
    if K:
        res["K"] = K_out
    if extra is not None:
        res.update(extra(eng))
    return res


def fresh_result(n, d, T, G, dK=False, K=False, staged=False, extra=None, **engine_kw):
    """A new SvgdEngine, its whole workspace zeroed, one call: the right answer of every state test.  (Window hit and
    miss are asserted bit-identical elsewhere, so one fresh call is the right answer whatever the predictor does.)"""
    engine_kw.setdefault("dtype", T.dtype)
    eng = SvgdEngine(n, d, device=T.device, **engine_kw)
    eng.ws.zero_()
    return engine_call(eng, T, G, dK, K, staged, extra)


def assert_same(tag, got, want):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for key in want:
        assert torch.equal(got[key], want[key]), (tag, key, "differs from a fresh engine's in %d entries" %
                                                  int((got[key] != want[key]).sum()))


def leftover_of(make, run):
    """the workspace(s) a donor built by make() holds after run(donor) -- one complete step on unrelated inputs"""
    donor = make()
    run(donor)
    torch.cuda.synchronize()
    images = [ws.clone() for ws, _ in _sections(donor)]
    return images if hasattr(donor, "blocks") else images[0]


# ---------------------------------------------------------------------------------------------------------------
# row blocks through the rank segments (n_local < n), the collectives done by hand
# ---------------------------------------------------------------------------------------------------------------
class _Block:
    pass


class RankBlocks:
    """The rows of one step dealt to row blocks [(row0, n_local), ...], every block with a workspace of its own, through
    stein_rank_begin / _pick / _radix / _finish as SvgdEngine._sharded_step issues them; the all-reduces are sums over the
    blocks' histograms (window form: tables) written back to every block."""

    def __init__(self, n, d, bounds, device, window):
        self.n, self.d, self.device, self.window = n, d, device, window
        self.st = HipStages()
        self.flags = _lib.FLAG_X3 | (_lib.FLAG_RANK_WINDOW if window else 0)
        self.blocks = []
        assert sum(nl for _, nl in bounds) == n and bounds[0][0] == 0
        for row0, nl in bounds:
            b = _Block()
            b.row0, b.nl = row0, nl
            total, b._offs, extra = _lib.workspace_layout(nl, n, d, _lib.F32, _lib.FLAG_X3 | _lib.FLAG_TILED)
            b.ld = extra[_lib.WSX_LD_DIST]
            b.ws = torch.zeros(total, dtype=torch.uint8, device=device)
            b.h2, b.median = torch.zeros(1, device=device), torch.zeros(1, device=device)
            self.blocks.append(b)
        self.flags_host = torch.zeros(8, dtype=torch.int32).pin_memory()

    @staticmethod
    def _view(b, sec, nbytes, dtype, at=0):
        o = b._offs[sec] + at
        return b.ws[o:o + nbytes].view(dtype)

    def _hist(self, b, level):
        nb = 2 * _lib.HIST_BINS * 8
        return self._view(b, _lib.WS_HIST, nb, torch.int64, level * nb)

    def _all_reduce(self, views):
        total = torch.stack(views).sum(0)
        for v in views:
            v.copy_(total)

    def _radix(self, T, need_level0_pass):
        st, n, d = self.st, self.n, self.d
        if need_level0_pass:
            for b in self.blocks:
                st.rank_radix(T, 0, True, n, d, b.row0, b.nl, b.ws, self.flags, b.h2, b.median)
        for level in range(_lib.HIST_LEVELS):
            self._all_reduce([self._hist(b, level) for b in self.blocks])
            for b in self.blocks:
                st.rank_radix(T, level, False, n, d, b.row0, b.nl, b.ws, self.flags, b.h2, b.median)

    def window_stats(self):
        w = self._view(self.blocks[0], _lib.WS_SELECT, 8, torch.int32, _lib.SPEC_NSTEPS_OFFSET).cpu()
        return int(w[0]), int(w[1])

    def step(self, T, G, dK=False):
        st, n, d, dev = self.st, self.n, self.d, self.device
        for b in self.blocks:
            b.h2.fill_(float("nan"))
            st.rank_begin(T, n, d, b.row0, b.nl, b.ws, self.flags)
        if self.window:
            self._all_reduce([self._view(b, _lib.WS_SPEC, 8 * _lib.SPEC_TABLE_WORDS, torch.int64, 8 * _lib.SPEC_TABLE_OFFSET_WORDS)
                              for b in self.blocks])
            seen = []
            for b in self.blocks:
                st.rank_pick(T, n, d, b.row0, b.nl, b.ws, self.flags, b.h2, b.median, self.flags_host)
                torch.cuda.synchronize()
                seen.append((bool(self.flags_host[0]), bool(self.flags_host[6])))
            assert len(set(seen)) == 1, ("the blocks disagree about the window", seen)
            if not seen[0][0]:
                self._radix(T, not seen[0][1])
        else:
            self._radix(T, False)
        phis, sums, dKs, Ds = [], [], [], []
        for b in self.blocks:
            st.x3_prepare(None, G, n, d, b.ws[b._offs[_lib.WS_PLANES]:])
            phi = torch.full((b.nl, d), float("nan"), device=dev)
            sq = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
            dK_out = torch.full((b.nl, d), float("nan"), device=dev) if dK else None
            st.rank_finish(T, G, n, d, b.row0, b.nl, b.h2, phi, sq, dK_out, b.ws, self.flags)
            torch.cuda.synchronize()
            rows = (b.nl + 127) // 128 * 128
            image = self._view(b, _lib.WS_DIST, rows * b.ld * 4, torch.float32).view(rows, b.ld)
            phis.append(phi), sums.append(sq), dKs.append(dK_out), Ds.append(untile_distances(image, b.nl, n))
        for b in self.blocks[1:]:
            assert torch.equal(b.h2, self.blocks[0].h2), "the blocks disagree about the bandwidth"
        res = dict(phi=torch.cat(phis), h2=self.blocks[0].h2.clone(), sums=torch.cat(sums), D=torch.cat(Ds))
        if dK:
            res["dK"] = torch.cat(dKs)
        return res


# ---------------------------------------------------------------------------------------------------------------
# the fused call at the ABI, explicit flags, a caller-owned workspace
# ---------------------------------------------------------------------------------------------------------------
class AbiCaller:
    """stein_svgd_phi through HipStages.svgd_phi on ONE workspace sized for the largest of `flag_sets`"""

    def __init__(self, n, d, device, flag_sets):
        self.n, self.d, self.device = n, d, device
        self.st = HipStages()
        layouts = [_lib.workspace_layout(n, n, d, _lib.F32, f) for f in flag_sets]
        self._offs = layouts[0][1]
        self.ld = layouts[0][2][_lib.WSX_LD_DIST]
        self.ws = torch.zeros(max(lay[0] for lay in layouts), dtype=torch.uint8, device=device)

    def call(self, T, G, flags, dK=False, K=False):
        n, d, dev = self.n, self.d, self.device
        phi = torch.full((n, d), float("nan"), device=dev)
        h2 = torch.full((1,), float("nan"), device=dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        sums[:1].fill_(float("nan"))
        dK_out = torch.full((n, d), float("nan"), device=dev) if dK else None
        K_out = torch.full((n, n), float("nan"), device=dev) if K else None
        self.st.svgd_phi(T, G, n, d, phi, h2, sums, K_out, dK_out, self.ws, flags)
        torch.cuda.synchronize()
        rows = (n + 127) // 128 * 128
        o = self._offs[_lib.WS_DIST]
        image = self.ws[o:o + rows * self.ld * 4].view(torch.float32).view(rows, self.ld)
        res = dict(phi=phi, h2=h2, sums=sums, D=untile_distances(image, n, n, upper=bool(flags & _lib.FLAG_X3)))
        if dK:
            res["dK"] = dK_out
        if K:
            res["K"] = K_out
        return res
