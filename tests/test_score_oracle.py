"""The score (csrc/kernels/lp_core.h) against golden.score_reference on hand-built tables, and
against golden.analyze on hand-laid text, with every ScoringParams field off its default.

The device kernels and the host loop compile the same source, so comparing them with each other
cannot see a wrong window bound or operand order. Here both are compared with a plain-Python
re-statement of golden.py's factor functions over hit sets (linear scans, no CSR arithmetic),
at hits placed ON the edges: x±w against x±(w+1), one line across a document border, a sequence
event on the cursor's own line, a 10- against an 11-line context, rate == threshold.

Every factor but proximity is asserted bit-equal. Proximity is the one factor through ``exp``:

**The proximity bound.** Reference: ``P* = 1 + sum_k w_k * RN(exp(q_k))`` in Python doubles, q_k the
EXACT quotient -d_k/decay, RN the correctly rounded double (golden.exp_correctly_rounded). The
backend computes ``qh = fl(-d/decay)``, ``eh = EXP(qh)``, ``fl(w*eh)``, adds from 0.0, then
``fl(1 + tot)``. With u = 2^-53 (a rounding moves x by at most u|x|; one ulp of x is at most 2u|x|),
E_k = exp(q_k) and K the documented ulp bound of the backend's fp64 exp:

* argument: qh = q(1+d0), |d0| <= u, so exp(qh) = E * exp(q*d0): off by |q| u E
* exp: eh is within K ulp of exp(qh): 2K u E; RN(exp(q)) is within u E. |eh - e*| <= (2K + |q| + 1) u E
* multiply: one rounding on either side: |fl(w eh) - fl(w e*)| <= |w| E (2K + |q| + 3) u
* adds: the first add (to 0.0) is exact; add i >= 2 rounds a partial sum of magnitude at most
  A_i = sum_{j<=i} |w_j| E_j on either side: 2u A_i. The final 1 + tot: 2u (1 + A_m)

so ``|Ph - P*| <= u * [sum_k |w_k| E_k (2K + |q_k| + 3) + 2 sum_{i=2..m} A_i + 2 (1 + A_m)]``, times
(1 + 2^-30) for the second-order terms. K: the ROCm install carries no accuracy statement for
ocml's fp64 exp, so the device uses the OpenCL C fp64 limit, 3 ulp (OpenCL C spec, "Relative
error as ULPs": exp <= 3 ulp); the host uses glibc's documented 1 ulp (glibc manual, "Known Maximum
Errors in Math Functions", exp on x86_64 / aarch64). For one secondary at weight 0.5, d = 1,
decay 6 the device bound is 7.5e-16 (3.4 ulp of the factor), the host bound 5.6e-16 (2.5 ulp). An
exp evaluated in float is off by ~6e-8 relative, eight orders of magnitude outside either. The
observed distances are in docs/PARITY.md.
"""
import dataclasses
import math

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import ScoringParams

# every field off its default and different from every other field; thresholds are binary fractions
PARAMS = ScoringParams(decay_constant=6.0, max_window=7, early_bonus_threshold=0.25, max_early_bonus=3.5,
                       penalty_threshold=0.75, max_context_factor=1.75, freq_threshold=2.0,
                       freq_max_penalty=0.5, freq_window_hours=3)
DEFAULTS = ScoringParams()
# the context sum of an ERROR + exception line lands exactly on this cap ...
ON_CAP = dataclasses.replace(PARAMS, max_context_factor=1.0 + (0.0 + 0.4 + 0.3))
# ... and no context case reaches this one
WIDE = dataclasses.replace(PARAMS, max_context_factor=6.5)
# at rate == threshold the penalty (rate - thr) / thr is 0 whether the comparison is > or >=; only under a
# negative cap does min(cap, 0) tell the two apart (the specification returns 0.0 before it takes the min)
NEGATIVE_CAP = dataclasses.replace(PARAMS, freq_max_penalty=-0.125)
PARAM_SETS = {"nondefault": PARAMS, "defaults": DEFAULTS, "on_cap": ON_CAP, "wide": WIDE,
              "negative_cap": NEGATIVE_CAP}

EXP_ULP = {"cpu": 1, "cuda": 3}     # documented fp64 exp bounds: glibc, OpenCL C (see the docstring)
U = 2.0 ** -53


def prox_bound(terms, decay, k_ulp):
    """Allowed |backend - reference| of 1 + sum w*exp(-d/decay) (derivation in the module docstring)."""
    from fractions import Fraction
    tot, a, adds = Fraction(0), Fraction(0), Fraction(0)
    for i, (w, d) in enumerate(terms):
        q = d / decay
        e = Fraction(golden.exp_correctly_rounded(-d, decay)) * (1 + Fraction(1, 2 ** 50))   # >= exp(q)
        a += abs(Fraction(w)) * e
        tot += abs(Fraction(w)) * e * (2 * k_ulp + Fraction(q) + 3)
        if i >= 1:
            adds += 2 * a
    return float((tot + adds + 2 * (1 + a)) * Fraction(U) * (1 + Fraction(1, 2 ** 30)))


def ulp_distance(a, b):
    return abs(a - b) / math.ulp(b)


# ------------------------------------------------------------------------------------------------
# one batch of 401 lines in four segments
DOC_A = (0, 40, 0, 0, 40)                # a 40-line document
DOC_B = (40, 41, 40, 0, 1)               # a 1-line document
DOC_C = (41, 341, 41, 0, 300)            # a 300-line document
G0, NBIG = 2 ** 31 + 7, 2 ** 32 + 12345
SHARD = (341, 401, 351, G0, NBIG)        # a shard: ten halo lines before own_lo, global offset, n != hi - lo
SEGMENTS = [DOC_A, DOC_B, DOC_C, SHARD]
A, B, C, S = 0, 1, 2, 3
L = 401
X = 141                                  # doc C's line 100: the proximity / temporal cases' cursor


def c(off):
    return DOC_C[0] + off


class Build:
    """Patterns, regex hit sets, feature bytes and events laid by hand."""

    def __init__(self):
        self.patterns, self.hits, self.feat = [], [], [0] * L
        self.events, self.names, self.want, self.carry, self.keys = [], [], [], [], []

    def rx(self, *lines):
        self.hits.append(set(lines))
        return len(self.hits) - 1

    def key(self, carry):
        self.carry.append(carry)
        return len(self.carry) - 1

    def pat(self, ctx=None, secs=(), seqs=(), key=-1):
        p = len(self.patterns)
        sev = (5.0, 3.0, 2.0, 1.5, 1.0)[p % 5]
        self.patterns.append({"conf": round(0.31 + 0.017 * p, 3), "sev": sev, "context": ctx,
                              "secondaries": list(secs), "sequences": [(b, list(r), list(f)) for b, r, f in seqs]})
        self.keys.append(key)
        return p

    def ev(self, name, p, x, seg, rank=0, **want):
        lo, hi = SEGMENTS[seg][:2]
        assert lo <= x < hi, name
        self.events.append((x, p, seg, rank, self.keys[p]))
        self.names.append(name)
        self.want.append(want)

    def tables(self):
        return {"patterns": self.patterns, "hits": self.hits, "feat": self.feat, "segments": SEGMENTS}


def one_sec(b, name, lines, w=3, weight=0.5, x=X, seg=C, **want):
    """One pattern with one secondary whose regex hits `lines`, one event on x."""
    r = b.rx(*lines)
    b.ev(name, b.pat(secs=[(r, w, weight)]), x, seg, **want)
    return r


def one_seq(b, name, chain, x=X, seg=C, bonus=0.5, flags=None, **want):
    """One pattern with one sequence; `chain` lists each event's hit lines, first event first."""
    regs = [b.rx(*lines) for lines in chain]
    b.ev(name, b.pat(seqs=[(bonus, regs, flags or [0] * len(regs))]), x, seg, **want)


def build_cases():
    b = Build()
    plain = b.pat()

    # ---- proximity (first: regex 0 is an empty row followed by a hit inside the window)
    r0 = b.rx()
    b.rx(X + 1)
    b.ev("prox regex 0 empty, neighbour row hits x+1", b.pat(secs=[(r0, 3, 0.5)]), X, C, d=[])
    b.ev("prox no secondaries", plain, X, C, prox=1.0)
    b.ev("prox sec_reg -1", b.pat(secs=[(-1, 3, 0.5)]), X, C, d=[])
    one_sec(b, "prox regex without hits", [], d=[])
    one_sec(b, "prox only hit on x", [X], d=[])
    one_sec(b, "prox x-1 and x+1", [X - 1, X + 1], d=[1])
    one_sec(b, "prox nearer after", [X - 3, X + 2], d=[2])
    one_sec(b, "prox nearer before", [X - 2, X, X + 3], d=[2])
    one_sec(b, "prox x-w", [X - 3], d=[3])
    one_sec(b, "prox x+w", [X + 3], d=[3])
    one_sec(b, "prox x-w-1", [X - 4], d=[])
    one_sec(b, "prox x+w+1", [X + 4], d=[])
    one_sec(b, "prox both just outside", [X - 4, X, X + 4], d=[])
    one_sec(b, "prox w=0", [X - 1, X, X + 1], w=0, d=[])
    one_sec(b, "prox w=-1", [X - 1, X, X + 1], w=-1, d=[])
    one_sec(b, "prox w=-3", [X - 3, X - 1, X, X + 1, X + 3], w=-3, d=[])
    one_sec(b, "prox clipped at lo, hit across the border", [40], x=42, d=[])
    one_sec(b, "prox clipped at lo, hit on lo", [40, 41], x=42, d=[1])
    one_sec(b, "prox clipped at hi, hit across the border", [40], x=38, seg=A, d=[])
    one_sec(b, "prox clipped at hi, hit on hi-1", [39, 40], x=38, seg=A, d=[1])
    one_sec(b, "prox doc C clipped at hi, hit in the shard's halo", [341], x=339, d=[])
    one_sec(b, "prox one-line document, hits on both neighbours", [39, 41], x=40, seg=B, d=[])
    b.rx(X - 30, X - 1)               # row r-1: its last hit lies inside the window
    one_sec(b, "prox x below every hit of r, row r-1 ends inside the window", [X + 10, X + 20], d=[])
    one_sec(b, "prox x above every hit of r, row r+1 starts inside the window", [X - 20, X - 10], d=[])
    b.rx(X + 1, X + 30)               # row r+1
    w4 = [(b.rx(X - 1), 3, 0.1), (b.rx(X + 2), 3, 0.2), (b.rx(X - 3), 3, 0.3), (b.rx(X + 1), 3, 0.7)]
    b.ev("prox four secondaries", b.pat(secs=w4), X, C, d=[1, 2, 3, 1])
    one_sec(b, "prox zero weight", [X - 2], weight=0.0, d=[2], prox=1.0)
    one_sec(b, "prox negative weight", [X - 2], weight=-0.25, d=[2])
    b.ev("prox zero, negative and positive weight",
         b.pat(secs=[(b.rx(X + 1), 3, 0.0), (b.rx(X - 1), 3, -0.25), (b.rx(X + 3), 3, 0.5)]), X, C, d=[1, 1, 3])
    one_sec(b, "prox w=7 hit at x+7", [X + 7], w=7, d=[7])

    # ---- temporal
    b.ev("temp no sequences", plain, X + 1, C, temp=1.0)
    b.ev("temp sequence without events", b.pat(seqs=[(0.5, [], [])]), X, C, temp=1.0)
    one_seq(b, "temp one event at x-5", [[X - 5]], temp=1.5)
    one_seq(b, "temp one event on x", [[X]], temp=1.5)
    one_seq(b, "temp one event at x+5", [[X + 5]], temp=1.5)
    one_seq(b, "temp one event at x-6", [[X - 6]], temp=1.0)
    one_seq(b, "temp one event at x+6", [[X + 6]], temp=1.0)
    one_seq(b, "temp window clipped at hi, hit across", [[40]], x=37, seg=A, temp=1.0)
    one_seq(b, "temp window clipped at hi, hit on hi-1", [[39, 40]], x=37, seg=A, temp=1.5)
    one_seq(b, "temp window clipped at lo, hit across", [[40]], x=43, temp=1.0)
    one_seq(b, "temp window clipped at lo, hit on lo", [[40, 41]], x=43, temp=1.5)
    one_seq(b, "temp three events strictly backwards", [[X - 10], [X - 3], [X + 2]], temp=1.5)
    one_seq(b, "temp three events, first not before the second", [[X - 3, X - 1], [X - 3], [X + 2]], temp=1.0)
    one_seq(b, "temp earlier event only on the cursor's line", [[X], [X]], temp=1.0)
    one_seq(b, "temp earlier event one line before the cursor", [[X - 1], [X + 4]], temp=1.5)
    one_seq(b, "temp earlier event in the previous document", [[40], [X]], temp=1.0)
    same = b.rx(X)
    b.ev("temp same regex twice, one line", b.pat(seqs=[(0.5, [same, same], [0, 0])]), X, C, temp=1.0)
    same2 = b.rx(X - 1, X)
    b.ev("temp same regex twice, two lines", b.pat(seqs=[(0.5, [same2, same2], [0, 0])]), X, C, temp=1.5)
    same3 = b.rx(X - 2, X + 1)
    b.ev("temp same regex three times, two lines", b.pat(seqs=[(0.5, [same3] * 3, [0, 0, 0])]), X, C, temp=1.0)
    one_seq(b, "temp missing event before own_lo, carry 0", [[345], [361]], x=360, seg=S, flags=[0, 0], temp=1.0)
    one_seq(b, "temp missing event before own_lo, carry 1", [[345], [361]], x=360, seg=S, flags=[1, 0], temp=1.5)
    one_seq(b, "temp event on own_lo", [[351], [361]], x=360, seg=S, temp=1.5)
    one_seq(b, "temp three events, the first before own_lo, carry 1", [[350], [355], [360]], x=360, seg=S,
            flags=[1, 0, 0], temp=1.5)
    one_seq(b, "temp carry flag of a later slot only", [[350], [355], [360]], x=360, seg=S, flags=[0, 1, 1], temp=1.0)
    two = [(0.5, [b.rx(X - 2), b.rx(X + 1)], [0, 0]), (0.25, [b.rx(X + 3)], [0])]
    b.ev("temp two sequences, both match", b.pat(seqs=two), X, C, temp=1.75)
    two = [(0.5, [b.rx(X), b.rx(X + 1)], [0, 0]), (0.25, [b.rx(X + 3)], [0])]
    b.ev("temp two sequences, the second matches", b.pat(seqs=two), X, C, temp=1.25)
    one_seq(b, "temp negative bonus", [[X - 1]], bonus=-0.25, temp=0.75)

    # ---- chronological (doc A: 0.25 * 40 = 10 and 0.75 * 40 = 30 are lines)
    b.ev("chrono first line", plain, 0, A, chrono=3.5)
    b.ev("chrono pos == early", plain, 10, A, chrono=1.5)
    b.ev("chrono one line after early", plain, 11, A)
    b.ev("chrono pos == penalty", plain, 30, A, chrono=1.0)
    b.ev("chrono one line after penalty", plain, 31, A)
    b.ev("chrono last line", plain, 39, A, chrono=0.5 + (1.0 - 39.0 / 40))
    b.ev("chrono n = 1", plain, 40, B, chrono=3.5)
    b.ev("chrono g0 + (x - lo) above 2^31, n above 2^32", plain, 400, S,
         chrono=1.0 + (0.75 - float(G0 + 59) / NBIG) * (0.5 / (0.75 - 0.25)))
    b.ev("chrono shard's first own line", plain, 351, S)

    # ---- context; the cap hides sums above it, so the expected sums are those of the `wide` parameters
    f = b.feat
    f[c(9)], f[c(10)], f[c(11)] = 0x0F, 1 | 8, 0x0F
    b.ev("ctx rules null, neighbours set", plain, c(10), C, ctx=1.0 + (0.0 + 0.4 + 0.3))
    b.ev("ctx before = after = 0", b.pat(ctx=(0, 0)), c(10), C, ctx=1.0 + (0.0 + 0.4 + 0.3))
    f[0], f[8], f[9] = 2, 2, 0x0F
    f[29], f[30], f[39], f[40] = 0x0F, 2, 2, 4
    wide = b.pat(ctx=(8, 6))
    b.ev("ctx clipped at lo", wide, 2, A, ctx=1.0 + (0.0 + 0.2 + 0.2))
    b.ev("ctx clipped at hi", wide, 38, A, ctx=1.0 + (0.0 + 0.2 + 0.2))
    b.ev("ctx clipped on both sides", wide, 40, B, ctx=1.0 + ((0.0 + 0.1) + 0.1))
    for n, x, before, after in ((7, c(30), 3, 3), (8, c(50), 3, 4), (9, c(70), 4, 4), (16, c(95), 8, 7),
                                (17, c(125), 8, 8)):
        a0, b0 = x - before, x + 1 + after
        assert b0 - a0 == n
        f[a0 - 1], f[a0], f[b0 - 1], f[b0] = 0x0F, 2, 2, 0x0F
        b.ev(f"ctx window of {n} lines", b.pat(ctx=(before, after)), x, C, ctx=1.0 + (0.0 + 0.2 + 0.2))
    # ERROR 0.4 (else WARN 0.2), stack 0.1, exception 0.3, then the stack bonus 0.1; bit 1 under bit 0 is ignored
    adds = [(), (0.4,), (0.2,), (0.4,), (0.1, 0.1), (0.4, 0.1, 0.1), (0.2, 0.1, 0.1), (0.4, 0.1, 0.1),
            (0.3,), (0.4, 0.3), (0.2, 0.3), (0.4, 0.3), (0.1, 0.3, 0.1), (0.4, 0.1, 0.3, 0.1), (0.2, 0.1, 0.3, 0.1),
            (0.4, 0.1, 0.3, 0.1)]
    for v in range(16):
        f[c(200 + v)] = v
        b.ev(f"ctx feat {v:#x}", plain, c(200 + v), C, ctx=1.0 + sum(adds[v], 0.0))
    for k in range(5):
        f[c(220 + k)] = 4
    for k in range(6):
        f[c(230 + k)] = 4
    six = b.pat(ctx=(0, 5))
    b.ev("ctx five stack lines", six, c(220), C, ctx=1.0 + (sum([0.1] * 5, 0.0) + 0.5))
    b.ev("ctx six stack lines", six, c(230), C, ctx=1.0 + (sum([0.1] * 6, 0.0) + 0.5))
    for k in list(range(240, 250)) + list(range(260, 271)):
        f[c(k)] = 4
    b.ev("ctx total = 10", b.pat(ctx=(5, 4)), c(245), C, ctx=1.0 + (sum([0.1] * 10, 0.0) + 0.5))
    b.ev("ctx total = 11", b.pat(ctx=(5, 5)), c(265), C, ctx=1.0 + (sum([0.1] * 11, 0.0) + 0.5) * 0.8)
    for k in range(7):
        f[c(165 + k)] = f[c(140 + k)] = 1 | 4
    f[c(147)] = 4
    twenty = b.pat(ctx=(10, 9))
    assert 14 <= 20 * 0.7 < 15
    b.ev("ctx stack + err = 14 of 20", twenty, c(175), C, ctx=1.0 + (sum([0.4, 0.1] * 7, 0.0) + 0.5))
    b.ev("ctx stack + err = 15 of 20", twenty, c(150), C, ctx=1.0 + (sum([0.4, 0.1] * 7 + [0.1], 0.0) + 0.5) * 0.8)

    # ---- frequency: counts 4 .. 19 cross rate == threshold and the cap of both parameter sets
    fk = b.pat(key=b.key(4))
    for rank in range(16):
        want = {6: 0.0, 7: (7 / 3.0 - 2.0) / 2.0, 9: 0.5, 10: 0.5}.get(4 + rank)
        b.ev(f"freq count {4 + rank}", fk, 352 + rank, S, rank=rank, **({} if want is None else {"pen": want}))
    b.ev("freq no key", plain, 353, S, rank=9, pen=0.0)
    b.ev("freq carry 0", b.pat(key=b.key(0)), 354, S, pen=0.0)
    b.ev("freq carry 2^40", b.pat(key=b.key(2 ** 40)), 355, S, rank=3, pen=0.5)

    # ---- the last regex: an empty row behind a row whose last hit lies inside the window
    b.rx(X - 1)
    b.ev("prox regex R-1 empty, neighbour row hits x-1", b.pat(secs=[(b.rx(), 3, 0.5)]), X, C, d=[])
    return b


CASES = build_cases()
_REF = {}


def reference(name):
    """golden.score_reference of the case events under one parameter set (computed once, read-only)."""
    if name not in _REF:
        _REF[name] = golden.score_reference(CASES.tables(), PARAM_SETS[name], CASES.events, CASES.carry)
    return _REF[name]


class Flat:
    """The case tables as the tensors and the 21-entry pointer tuple Engine.finish hands to K.score_fused.
    Every array ends in one spare element, so an empty table still has an address; hit_line's spare is
    a line inside the last case's window."""

    def __init__(self, b, dev):
        i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
        P = b.patterns
        sec_off, seq_off, seq_ev_off = [0], [0], [0]
        sec_reg, sec_w, sec_weight, seq_bonus, seq_ev_reg, seq_carry = [], [], [], [], [], []
        for p in P:
            for r, w, weight in p["secondaries"]:
                sec_reg.append(r), sec_w.append(w), sec_weight.append(weight)
            sec_off.append(len(sec_reg))
            for bonus, regs, flags in p["sequences"]:
                seq_bonus.append(bonus), seq_ev_reg.extend(regs), seq_carry.extend(flags)
                seq_ev_off.append(len(seq_ev_reg))
            seq_off.append(len(seq_bonus))
        hit_off, hit_line = [0], []
        for h in b.hits:
            hit_line.extend(sorted(h))
            hit_off.append(len(hit_line))

        def T(v, dt, spare=0):
            return torch.tensor(list(v) + [spare], dtype=dt).to(dev)
        self.t = [T([p["conf"] for p in P], f64), T([p["sev"] for p in P], f64),
                  T([-1 if p["context"] is None else p["context"][0] for p in P], i32),
                  T([-1 if p["context"] is None else p["context"][1] for p in P], i32),
                  T(sec_off, i32), T(sec_reg, i32), T(sec_w, i32), T(sec_weight, f64), T(seq_off, i32),
                  T(seq_bonus, f64), T(seq_ev_off, i32), T(seq_ev_reg, i32), T(seq_carry, u8, 1),
                  T(hit_off, i64, len(hit_line)), T(hit_line, i32, X + 1), T(b.feat, u8, 0x0F),
                  T([s[0] for s in SEGMENTS], i32), T([s[1] for s in SEGMENTS], i32),
                  T([s[2] for s in SEGMENTS], i32), T([s[3] for s in SEGMENTS], i64),
                  T([s[4] for s in SEGMENTS], i64)]
        self.st = tuple(t.data_ptr() for t in self.t)
        assert len(self.st) == 21
        self.carry = T(b.carry, i64)
        self.dev = dev

    def events(self, idx):
        ev = [CASES.events[i] for i in idx]
        col = lambda k, dt: torch.tensor([e[k] for e in ev], dtype=dt).to(self.dev)   # noqa: E731
        return (col(0, torch.int32), col(1, torch.int32), col(2, torch.int32), col(3, torch.int64),
                col(4, torch.int64))


_FLAT = {}


def flat(dev):
    key = str(dev)
    if key not in _FLAT:
        _FLAT[key] = Flat(CASES, dev)
    return _FLAT[key]


def sp_tuple(params):
    from log_parser_amd.engine import Engine
    return Engine.score_param_tuple(params)


def run_backend(dev, pname, idx, with_factors=True):
    fl = flat(dev)
    score, fac = K.score_fused(*fl.events(idx), fl.carry, fl.st, sp_tuple(PARAM_SETS[pname]), with_factors)
    return score.cpu().tolist(), (fac.cpu().tolist() if with_factors else None)


def check_against_reference(dev, pname, idx, score, fac):
    """Six factors bit-equal, the score bit-equal to the left-to-right product with the backend's own
    proximity, the proximity inside the derived bound. Returns the largest ulp distance of a
    proximity factor from the reference."""
    ref = reference(pname)
    k_ulp = EXP_ULP[torch.device(dev).type]
    decay = PARAM_SETS[pname].decay_constant
    worst = 0.0
    for row, i in enumerate(idx):
        r, f, name = ref[i], fac[row], f"{CASES.names[i]} [{pname}, event {row}]"
        for k, what in ((0, "confidence"), (1, "severity"), (2, "chronological"), (4, "temporal"), (5, "context"),
                        (6, "penalty")):
            assert f[k] == r["factors"][k], f"{what}: {name}: got {f[k]!r}, reference {r['factors'][k]!r}"
        product = f[0] * f[1] * f[2] * f[3] * f[4] * f[5] * (1.0 - f[6])
        assert score[row] == product, f"product order: {name}: got {score[row]!r}, left to right {product!r}"
        bound = prox_bound(r["prox_terms"], decay, k_ulp) if r["prox_terms"] else 0.0
        dist = abs(f[3] - r["factors"][3])
        assert dist <= bound, f"proximity: {name}: got {f[3]!r}, reference {r['factors'][3]!r}, bound {bound:g}"
        worst = max(worst, ulp_distance(f[3], r["factors"][3]))
    return worst


ALL = list(range(len(CASES.events)))


def tiled(n):
    return [ALL[i % len(ALL)] for i in range(n)]


# ------------------------------------------------------------------------------------------------
# the reference itself: the cases sit where they claim to

def test_cases_land_on_their_edges():
    """Hand-computed factors of the reference: each case's hit is counted or not as its name says."""
    ref, wide = reference("nondefault"), reference("wide")
    assert len(CASES.patterns) >= 36 and len(CASES.hits) >= 36
    for i, (name, want) in enumerate(zip(CASES.names, CASES.want)):
        fac = ref[i]["factors"]
        if "d" in want:
            assert [d for _, d in ref[i]["prox_terms"]] == [float(d) for d in want["d"]], name
            if not want["d"]:
                assert fac[3] == 1.0, name
        for key, col in (("chrono", 2), ("prox", 3), ("temp", 4), ("pen", 6)):
            if key in want:
                assert fac[col] == want[key], (name, fac[col], want[key])
        if "ctx" in want:
            assert wide[i]["factors"][5] == want["ctx"], (name, wide[i]["factors"][5], want["ctx"])
            assert fac[5] == min(want["ctx"], PARAMS.max_context_factor), name
    # exactly on the cap, and one step over it
    on = {n: r["factors"][5] for n, r in zip(CASES.names, reference("on_cap"))}
    assert on["ctx feat 0x9"] == ON_CAP.max_context_factor == wide[CASES.names.index("ctx feat 0x9")]["factors"][5]
    assert on["ctx feat 0xd"] == ON_CAP.max_context_factor < wide[CASES.names.index("ctx feat 0xd")]["factors"][5]
    # the four secondaries' terms do not sum associatively
    four = ref[CASES.names.index("prox four secondaries")]["prox_terms"]
    t = [w * golden.exp_correctly_rounded(-d, PARAMS.decay_constant) for w, d in four]
    assert ((t[0] + t[1]) + t[2]) + t[3] != t[0] + (t[1] + (t[2] + t[3]))
    # the defaults' rate == threshold and cap
    pen = {n: r["factors"][6] for n, r in zip(CASES.names, reference("defaults"))}
    assert pen["freq count 10"] == 0.0 < pen["freq count 11"] == 0.1
    assert pen["freq count 17"] < pen["freq count 18"] == 0.8 == pen["freq count 19"]
    pen = {n: r["factors"][6] for n, r in zip(CASES.names, reference("negative_cap"))}
    assert pen["freq count 6"] == 0.0 and pen["freq count 7"] == -0.125


def test_reference_proximity_equals_golden_text_functions():
    """score_reference's proximity and temporal factors equal golden.proximity_factor /
    temporal_factor on a text whose lines carry one token per hit (math.exp against the correctly
    rounded exp: within glibc's 1 ulp per term, so inside the host bound)."""
    from log_parser_amd.models.schema import Pattern
    lo, hi = DOC_C[:2]
    lines = [" ".join(f"r{r}q" for r, h in enumerate(CASES.hits) if j in h) for j in range(lo, hi)]
    ref = reference("nondefault")
    seen = 0
    for i, (x, p, seg, _, _) in enumerate(CASES.events):
        pat = CASES.patterns[p]
        if seg != C:
            continue
        model = Pattern.model_validate({
            "secondary_patterns": [{"regex": f"r{r}q" if r >= 0 else None, "weight": wt, "proximity_window": w}
                                   for r, w, wt in pat["secondaries"]],
            "sequence_patterns": [{"bonus_multiplier": bo, "events": [{"regex": f"r{r}q"} for r in regs]}
                                  for bo, regs, _ in pat["sequences"]]})
        prox = golden.proximity_factor(model, x - lo, lines, PARAMS)
        if ref[i]["prox_terms"]:
            assert abs(prox - ref[i]["factors"][3]) <= prox_bound(ref[i]["prox_terms"], 6.0, 1), CASES.names[i]
        else:
            assert prox == ref[i]["factors"][3] == 1.0, CASES.names[i]
        assert golden.temporal_factor(model, x - lo, lines) == ref[i]["factors"][4], CASES.names[i]
        seen += 1
    assert seen > 60


# ------------------------------------------------------------------------------------------------
# the host loop (score_host)

@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_score_host_matches_reference(pname):
    score, fac = run_backend("cpu", pname, ALL)
    worst = check_against_reference("cpu", pname, ALL, score, fac)
    print(f"host proximity: largest distance from the reference {worst:.3f} ulp [{pname}]")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_score_host_event_counts(n):
    idx = tiled(n)
    score, fac = run_backend("cpu", "nondefault", idx)
    check_against_reference("cpu", "nondefault", idx, score, fac)
    assert run_backend("cpu", "nondefault", idx, with_factors=False)[0] == score


# ------------------------------------------------------------------------------------------------
# k_score

@pytest.mark.gpu
@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_k_score_matches_reference(gpu_device, pname):
    score, fac = run_backend(gpu_device, pname, ALL)
    worst = check_against_reference(gpu_device, pname, ALL, score, fac)
    print(f"device proximity: largest distance from the reference {worst:.3f} ulp [{pname}]")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_k_score_event_counts(gpu_device, n):
    """Event counts around k_score's 64-event workgroup, with and without the factor rows."""
    idx = tiled(n)
    score, fac = run_backend(gpu_device, "nondefault", idx)
    check_against_reference(gpu_device, "nondefault", idx, score, fac)
    assert run_backend(gpu_device, "nondefault", idx, with_factors=False)[0] == score


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 64])
def test_k_score_device_count_below_capacity(gpu_device, count):
    """A device event count dn[0] under a capacity of 130: the first dn[0] rows are scored, the rest
    of the score and factor arrays is not written."""
    from log_parser_amd.native import N
    cap, sentinel = 130, -12345.678
    idx = tiled(cap)
    fl = flat(gpu_device)
    ev = fl.events(idx)
    out = torch.full((cap,), sentinel, dtype=torch.float64, device=gpu_device)
    fac = torch.full((cap, 7), sentinel, dtype=torch.float64, device=gpu_device)
    dn = torch.tensor([count], dtype=torch.int64, device=gpu_device)
    N.score_dev(*(t.data_ptr() for t in ev), fl.carry.data_ptr(), cap, fl.st, sp_tuple(PARAMS), out.data_ptr(),
                fac.data_ptr(), torch.cuda.current_stream(gpu_device).cuda_stream, dn.data_ptr())
    torch.cuda.synchronize()
    out, fac = out.cpu(), fac.cpu()
    check_against_reference(gpu_device, "nondefault", idx[:count], out[:count].tolist(), fac[:count].tolist())
    assert bool((out[count:] == sentinel).all()) and bool((fac[count:] == sentinel).all())
    out2 = torch.full((cap,), sentinel, dtype=torch.float64, device=gpu_device)
    K.score_fused(*ev, fl.carry, fl.st, sp_tuple(PARAMS), False, out=out2, dn=dn)
    assert torch.equal(out2.cpu(), out)


# ================================================================================================
# engine level: hand-laid text, golden.analyze as the reference, the non-default parameters with
# max_window = 7 (the only place the min(max_window, proximity_window) clamp and the parameter tuple
# sit on the path)

def _library():
    from log_parser_amd.models.schema import PatternSet

    def P(name, primary, pid="", sev="HIGH", conf=0.83, **kw):
        d = {"name": name, "severity": sev, "primary_pattern": {"regex": primary, "confidence": conf}, **kw}
        if pid is not None:
            d["id"] = pid or name
        return d

    def sec(rx, w, weight):
        return {"regex": rx, "weight": weight, "proximity_window": w}

    def seq(bonus, *events):
        return {"description": "s", "bonus_multiplier": bonus, "events": [{"regex": e} for e in events]}
    pats = [
        P("plain", "PRIMPLAIN", sev="LOW", conf=0.91),
        P("edge3", "PRIMEDGE3", conf=0.77, secondary_patterns=[sec("SECAAA", 3, 0.5)]),
        P("edge7", "PRIMEDGE7", sev="CRITICAL", conf=0.59, secondary_patterns=[sec("SECBBB", 7, 0.4)],
          context_extraction={"lines_before": 0, "lines_after": 0}),
        P("edge50", "PRIMEDGE50", sev="MEDIUM", conf=0.68, secondary_patterns=[sec("SECCCC", 50, 0.3)],
          context_extraction={"lines_before": 8, "lines_after": 6}),
        P("multi", "PRIMMULTI", conf=0.47, secondary_patterns=[sec("SECAAA", 3, 0.1), sec("SECBBB", 7, 0.2),
                                                               sec("SECCCC", 50, 0.3), sec("SECDDD", 3, 0.7)]),
        P("seq1", "PRIMSEQONE", sev="INFO", conf=0.88, sequence_patterns=[seq(0.5, "EVTONE")]),
        P("seq3", "PRIMSEQTHREE", conf=0.36, sequence_patterns=[seq(0.75, "EVTA", "EVTB", "EVTC"),
                                                                seq(0.25, "EVTSAME", "EVTSAME")]),
        P("noid", "PRIMNOID", pid=None, conf=0.93, secondary_patterns=[sec("SECAAA", 3, 0.5)]),
        P("freq", "PRIMFREQ", sev="MEDIUM", conf=0.71),
        P("ctx86", "PRIMCTX", conf=0.64, context_extraction={"lines_before": 8, "lines_after": 6}),
        P("negseq", "PRIMNEG", conf=0.52, sequence_patterns=[seq(-0.25, "EVTONE")],
          secondary_patterns=[sec("SECDDD", 3, -0.25)]),
        # a bit-parallel (BPG) program: with one in the library the runner verifies every candidate
        # before the join and a request's tail runs as the one k_request_tail kernel
        P("bpg", r"BPGTOK refused.{0,600}port \d+", conf=0.81),
    ]
    return [PatternSet.model_validate({"metadata": {"library_id": "oracle"}, "patterns": pats})]


def _doc(n, lines):
    return "\n".join(lines.get(i, f"filler line {i} all quiet") for i in range(n))


STACK = "\tat com.acme.Worker.run(Worker.java:42)"

# proximity: x-w / x+w against x±(w+1) for windows 3, 7 and 50 (clamped to 7); chronological edges of
# a 60-line document (0.25 * 60 = 15, 0.75 * 60 = 45)
DOC_PROX = _doc(60, {
    0: "PRIMPLAIN", 5: "PRIMNOID", 7: "SECAAA", 10: "PRIMEDGE3", 15: "PRIMPLAIN", 16: "PRIMPLAIN",
    20: "PRIMEDGE3", 24: "SECAAA", 23: "PRIMEDGE50", 30: "SECCCC", 32: "PRIMEDGE7", 38: "PRIMEDGE50",
    39: "SECBBB", 45: "PRIMPLAIN", 46: "PRIMPLAIN", 47: "PRIMEDGE7", 51: "PRIMNEG", 54: "SECDDD", 56: "SECAAA",
    57: "PRIMMULTI", 58: "SECCCC", 59: "SECBBB PRIMPLAIN"})
# two documents packed next to each other: the border lines carry each other's tokens
DOC_X = _doc(30, {10: "EVTA", 15: "EVTB", 17: STACK, 25: "PRIMCTX", 27: "PRIMSEQTHREE", 28: "PRIMEDGE7",
                  29: "ERROR SECAAA EVTONE at the end of X"})
DOC_Y = _doc(30, {0: "WARN SECBBB EVTC at the start of Y", 1: "PRIMEDGE3", 2: "PRIMSEQONE", 3: "PRIMCTX",
                  4: "PRIMSEQTHREE", 9: "java.lang.IllegalStateException: boom"})
# temporal: ±5 against ±6, the event on the cursor's own line, chains
DOC_TEMP = _doc(40, {3: "EVTA", 5: "EVTONE", 10: "PRIMSEQONE", 14: "EVTB", 20: "PRIMSEQTHREE EVTSAME", 21: "EVTC",
                     22: "PRIMSEQONE", 23: "PRIMSEQONE", 28: "EVTONE", 30: "PRIMSEQTHREE EVTC EVTB", 36: "PRIMSEQONE EVTONE",
                     38: "PRIMNEG"})
DOC_TEMP2 = _doc(30, {2: "EVTA", 11: "EVTSAME", 12: "PRIMSEQTHREE EVTB EVTC EVTSAME", 20: "BPGTOK refused by peer on port 8443",
                      25: "PRIMSEQTHREE EVTC"})
# context windows of 8 / 6 lines: dense stack frames (the 0.8 factor and the cap), a sparse one under the cap
DOC_CTX = _doc(40, {**{i: STACK for i in range(12, 20)}, 20: "ERROR PRIMCTX", 21: STACK, 22: STACK,
                    33: "WARN disk nearly full", 35: "PRIMCTX", 36: "java.lang.IllegalStateException: boom"})
# frequency: rate == threshold after 6 matches in a 3 h window, the cap after 9
DOC_FREQ = _doc(30, {2 * i + 1: "PRIMFREQ" for i in range(12)})


def _repeat(n):
    return "\n".join(f"PRIMPLAIN repeat {i}" for i in range(n))


BATCHES = [[DOC_PROX, DOC_X, DOC_Y, DOC_TEMP, DOC_TEMP2, DOC_CTX, DOC_FREQ], [_repeat(255)], [DOC_FREQ, _repeat(244)],
           [_repeat(257)], [DOC_FREQ, DOC_PROX]]
# seconds: the first batch leaves the 3 h window before the last one, the others stay inside it
TIMES = [1000.0, 4000.0, 7000.0, 10000.0, 11900.0]
_ENGINE_REF = {}


def _setup():
    if not _ENGINE_REF:
        from log_parser_amd.models.compiled import CompiledLibrary
        sets = _library()
        clk = [0.0]
        tracker = golden.FrequencyTracker(PARAMS, clock=lambda: clk[0])
        ref = []
        for t, batch in zip(TIMES, BATCHES):
            clk[0] = t
            ref.append([golden.analyze(d, sets, PARAMS, tracker) for d in batch])
        _ENGINE_REF.update(sets=sets, lib=CompiledLibrary(sets, PARAMS), ref=ref,
                           by_name={p.name: p for p in sets[0].patterns})
        n = [sum(len(g["events"]) for g in b) for b in ref]
        assert n[1:4] == [255, 256, 257], n
    return _ENGINE_REF


def _score_tolerance(dev_type, pattern, i, lines, score):
    """|engine - golden| allowed for one score: both proximity factors lie within prox_bound of the
    correctly rounded reference (golden's math.exp is glibc's), and the factor enters a
    left-to-right product that rounds once per multiply, four times from the proximity on, on
    either side. Zero without a counted secondary."""
    terms = []
    for s in pattern.secondary_patterns or []:
        w = min(PARAMS.max_window, s.proximity_window)
        near = [abs(j - i) for j in range(max(0, i - w), min(len(lines), i + w + 1))
                if j != i and golden._find(s.regex, lines[j])]
        if near:
            terms.append((s.weight, float(min(near))))
    if not terms:
        return 0.0
    d = prox_bound(terms, PARAMS.decay_constant, EXP_ULP[dev_type]) + prox_bound(terms, PARAMS.decay_constant, 1)
    prox = golden.proximity_factor(pattern, i, lines, PARAMS)
    return abs(score) * (d / abs(prox) + 8 * U) * (1 + 2.0 ** -30)


def _check_doc(dev_type, got_events, g, logs):
    """got_events: [(line number, pattern name, context or None, score)] against golden result g."""
    ref = _setup()
    lines = golden.split_lines(logs)
    assert len(got_events) == len(g["events"])
    for (ln, name, ctx, score), e in zip(got_events, g["events"]):
        assert ln == e["lineNumber"] and name == e["matchedPattern"]["name"]
        if ctx is not None:
            assert ctx == e["context"]
        tol = _score_tolerance(dev_type, ref["by_name"][name], ln - 1, lines, e["score"])
        assert abs(score - e["score"]) <= tol, (name, ln, score, e["score"], tol)


def _json_events(o):
    return [(e["lineNumber"], e["matchedPattern"]["name"], e["context"], e["score"]) for e in o["events"]]


def _engine(dev, clk, **overrides):
    from log_parser_amd.engine import Engine
    from log_parser_amd.frequency import DeviceFrequencyState, FrequencyState
    from log_parser_amd.utils.config import Config
    ref = _setup()
    dev = torch.device(dev)
    clock = lambda: clk[0]   # noqa: E731
    freq = (DeviceFrequencyState(ref["lib"].freq_ids, PARAMS.freq_window_hours, dev, clock=clock)
            if dev.type == "cuda" else FrequencyState(PARAMS.freq_window_hours, clock=clock))
    return Engine(ref["lib"], Config.load(overrides={"engine.device": str(dev), **overrides}), device=dev, freq=freq)


def _run_batches(eng, clk, dev_type, before=None, after=None):
    import json
    ref = _setup()
    outs = []
    for k, (t, batch) in enumerate(zip(TIMES, BATCHES)):
        clk[0] = t
        if before:
            before(k)
        res = [json.loads(o) for o in eng.analyze_batch_json(batch)]
        if after:
            after(k)
        for o, g, logs in zip(res, ref["ref"][k], batch):
            _check_doc(dev_type, _json_events(o), g, logs)
            assert o["summary"] == g["summary"]
        outs.append([_json_events(o) for o in res])
    return outs


def test_hand_laid_documents_sit_on_the_edges():
    """The golden results of the hand-laid text: the edges are where the layout claims."""
    from log_parser_amd.models.compiled import CompiledLibrary   # noqa: F401
    ref = _setup()
    assert ref["lib"].summary()["nfa_bpg"] >= 1
    P, lines = ref["by_name"], golden.split_lines(DOC_PROX)
    prox = lambda name, i, ls=lines: golden.proximity_factor(P[name], i, ls, PARAMS)   # noqa: E731
    assert prox("edge3", 10) == 1.0 + 0.5 * math.exp(-3.0 / 6.0) and prox("edge3", 20) == 1.0       # x-3 | x+4
    assert prox("edge7", 32) == 1.0 + 0.4 * math.exp(-7.0 / 6.0) and prox("edge7", 47) == 1.0       # x+7 | x-8
    assert prox("edge50", 23) == 1.0 + 0.3 * math.exp(-7.0 / 6.0) and prox("edge50", 38) == 1.0     # clamp: 7 | 8
    assert prox("multi", 57) == 1.0 + (((0.1 * math.exp(-1 / 6.0) + 0.2 * math.exp(-2 / 6.0)) + 0.3 * math.exp(-1 / 6.0))
                                       + 0.7 * math.exp(-3 / 6.0))
    x, y = golden.split_lines(DOC_X), golden.split_lines(DOC_Y)
    assert prox("edge7", 28, x) == 1.0 and prox("edge3", 1, y) == 1.0          # the hit is one document over
    assert prox("edge7", 28, x + y) > 1.0 and prox("edge3", 31, x + y) > 1.0
    temp = lambda name, i, ls: golden.temporal_factor(P[name], i, ls)   # noqa: E731
    assert temp("seq3", 27, x) == 1.0 and temp("seq3", 27, x + y) == 1.75
    assert temp("seq1", 2, y) == 1.0 and temp("seq1", 32, x + y) == 1.5
    assert temp("seq3", 4, y) == 1.0 and temp("seq3", 34, x + y) == 1.75
    t = golden.split_lines(DOC_TEMP)
    assert [temp("seq1", i, t) for i in (10, 22, 23, 36)] == [1.5, 1.0, 1.5, 1.5]      # x-5 | x+6 | x+5 | on x
    assert temp("seq3", 20, t) == 1.75 and temp("seq3", 30, t) == 1.75 and temp("negseq", 38, t) == 0.75
    t2 = golden.split_lines(DOC_TEMP2)
    assert temp("seq3", 12, t2) == 1.25 and temp("seq3", 25, t2) == 1.75
    pens = [1.0 - e["score"] / (0.71 * 2.0 * golden.chronological_factor(e["lineNumber"] - 1, 30, PARAMS))
            for e in ref["ref"][0][6]["events"]]
    assert pens[:7] == [0.0] * 7 and 0.0 < pens[7] < pens[8] < pens[9] and abs(pens[9] - 0.5) < 1e-15
    assert abs(pens[10] - 0.5) < 1e-15
    # the last batch: the first batch's 12 matches have left the window, the third batch's 12 have not
    last = ref["ref"][4][0]["events"]
    assert last[0]["score"] == 0.71 * 2.0 * golden.chronological_factor(1, 30, PARAMS) * (1.0 - 0.5)


def test_cpu_engine_matches_golden():
    clk = [0.0]
    _run_batches(_engine("cpu", clk), clk, "cpu")


def _stream_file():
    return "\n".join([DOC_PROX, DOC_TEMP, DOC_CTX, DOC_FREQ, DOC_TEMP2])


def _check_stream(dev):
    """A 200-line file through the chunked stream in three chunks: the chunks' scores are completed by
    k_rescore / its host twin with the non-default chronological parameters."""
    from log_parser_amd.parallel.stream import StreamAnalyzer
    ref = _setup()
    logs = _stream_file()
    data = logs.encode()
    clk = [500.0]
    out = StreamAnalyzer(_engine(dev, clk), chunk_bytes=len(data) // 3 + 1, topk=5).run(data)
    assert out.chunks == 3
    g = golden.analyze(logs, ref["sets"], PARAMS, golden.FrequencyTracker(PARAMS, clock=lambda: 500.0))
    gl, pat, score = out.events
    names = [p.name for p in ref["sets"][0].patterns]
    got = [(int(a) + 1, names[int(b)], None, float(s)) for a, b, s in zip(gl, pat, score)]
    assert len(got) > 30
    _check_doc(torch.device(dev).type, got, g, logs)


def test_cpu_stream_in_three_chunks_matches_golden():
    _check_stream("cpu")


@pytest.mark.gpu
def test_gpu_stream_in_three_chunks_matches_golden(gpu_device):
    _check_stream(gpu_device)


@pytest.mark.gpu
def test_gpu_engine_orchestrated_matches_golden(gpu_device):
    """engine.native-runner=false: the Python orchestration, scores from k_score."""
    clk = [0.0]
    eng = _engine(gpu_device, clk, **{"engine.native-runner": False})
    _run_batches(eng, clk, "cuda")
    assert eng._runner in (None, False)
    clk[0] = 50000.0
    one = eng.analyze(DOC_TEMP)                            # every earlier record has left the 3 h window
    g = golden.analyze(DOC_TEMP, _setup()["sets"], PARAMS, golden.FrequencyTracker(PARAMS, clock=lambda: 0.0))
    _check_doc("cuda", _json_events(one), g, DOC_TEMP)


@pytest.mark.gpu
def test_gpu_runner_tail_matches_golden_and_orchestration(gpu_device):
    """The native runner with every batch's tail in the one k_request_tail kernel (its phase stamp,
    slot 15, is written by nothing else): scores bit-equal to the orchestration's k_score, both held
    to golden; batches of 255, 256 and 257 events around the tail's 256-event pass; consecutive
    batches, so the penalties come from the device window with its 3-hour divisor."""
    from log_parser_amd.native import N
    clk = [0.0]
    off = _run_batches(_engine(gpu_device, clk, **{"engine.native-runner": False}), clk, "cuda")
    eng = _engine(gpu_device, clk, **{"engine.native-runner": True})
    prof = torch.zeros(16, dtype=torch.int64, device=gpu_device)
    stamps = []

    def before(k):
        prof.zero_()
        torch.cuda.synchronize()
        N.set_small_profile(prof.data_ptr())

    def after(k):
        torch.cuda.synchronize()
        N.set_small_profile(0)
        stamps.append(int(prof[15]))
    try:
        on = _run_batches(eng, clk, "cuda", before, after)
    finally:
        N.set_small_profile(0)
    assert eng._runner not in (None, False)
    assert all(stamps), f"k_request_tail did not run for every batch: {stamps}"
    assert on == off


@pytest.mark.gpu
def test_gpu_run_document_matches_golden(gpu_device):
    ref = _setup()
    names = [p.name for p in ref["sets"][0].patterns]
    clk = [0.0]
    eng = _engine(gpu_device, clk)
    tracker = golden.FrequencyTracker(PARAMS, clock=lambda: clk[0])
    for logs in (DOC_PROX, DOC_FREQ, DOC_TEMP, DOC_FREQ):
        data = logs.encode()
        t = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        res = eng.run_document(t.to(gpu_device), len(data), with_factors=True)
        g = golden.analyze(logs, ref["sets"], PARAMS, tracker)
        score, fac = res.score.cpu().tolist(), res.factors.cpu().tolist()
        got = [(int(a) + 1, names[int(b)], None, s) for a, b, s in zip(res.ev_line.cpu(), res.ev_pat.cpu(), score)]
        _check_doc("cuda", got, g, logs)
        for s, f in zip(score, fac):
            assert s == f[0] * f[1] * f[2] * f[3] * f[4] * f[5] * (1.0 - f[6])
