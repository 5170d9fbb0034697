"""Cases for the pauses tests (test_pauses.py, test_gpu_pauses.py): runs of (stamp, signature) lists
for ``K.pause_scan`` with what a plain Python loop gives for them, and the 4000-line log with its
parameter sets. A case is (min_ms, first line_base, first carry, [(ts, sig), ...]): the runs of one
log, each continuing the last with the carry it returned."""
import functools
import random

import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.synth import log_templates, pause_log

NONE = K.TS_NONE
I64_MAX = (1 << 63) - 1
TILE = K.PS_TILE
T0 = 1_758_283_200_000
SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 2048 * 257 + 1)     # the last: two tiles per lane of the prefix block


def reference(ts, sig, min_ms, line_base=0, carry=None):
    """(rows, stats, hist, carry) of one run: the specification as a loop."""
    rows, stats, hist = [], [0, 0, 0, I64_MAX, NONE], [0] * 64
    for i, (t, s) in enumerate(zip(ts, sig)):
        if t == NONE:
            continue
        stats[0] += 1
        stats[3], stats[4] = min(stats[3], t), max(stats[4], t)
        if carry is not None:
            step = t - carry[0]
            if step < 0:
                stats[1] += 1
            else:
                hist[step.bit_length()] += 1
                if step >= min_ms:
                    stats[2] += step
                    rows.append((line_base + i, carry[1], step, carry[2], s))
        carry = (t, line_base + i, s)
    return rows, stats, hist, carry


def _random_run(L: int, seed: int, t: int = T0):
    rng = random.Random(seed)
    sigs = [rng.getrandbits(64) - (1 << 63) for _ in range(7)]
    ts, sig = [], []
    for _ in range(L):
        t += rng.choice((0, 0, 1, 5, 50, 400, 999, 1000, 1500, 70_000, -30))
        ts.append(NONE if rng.random() < 0.2 else t)
        sig.append(rng.choice(sigs))
    return ts, sig


def _at(L: int, stamps: dict):
    """A run of L lines, stamped where ``stamps`` says; line i has the signature 100 + i % 5."""
    return [stamps.get(i, NONE) for i in range(L)], [100 + i % 5 for i in range(L)]


def _steps(steps):
    """Stamped lines 0, s0, 0, s1, ...: every step of ``steps``, a backward step after each."""
    ts = [0]
    for s in steps:
        ts += [s, 0]
    return ts, list(range(len(ts)))


@functools.lru_cache(maxsize=None)
def scan_cases():
    cases = {"L=%d" % L: (1000, 0, None, [_random_run(L, L)]) for L in SIZES}
    L3 = 3 * TILE
    cases["no stamp"] = (1000, 0, None, [_at(300, {})])
    cases["only the first line stamped"] = (1000, 0, None, [_at(5000, {0: T0})])
    cases["only the last line stamped"] = (1000, 0, None, [_at(5000, {4999: T0})])
    # the border step of tile 2 jumps over tile 1: once a pause, once one millisecond short of one
    cases["a tile without a stamp, pause across it"] = (1000, 0, None, [_at(L3, {5: T0, 700: T0 + 10, 2 * TILE + 9: T0 + 1010})])
    cases["a tile without a stamp, no pause across it"] = (1000, 0, None, [_at(L3, {5: T0, 700: T0 + 10, 2 * TILE + 9: T0 + 1009})])
    edges = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, L3 - 1]
    cases["stamps on the first and last line of tiles"] = (1000, 0, None, [_at(L3, {i: T0 + 2000 * k for k, i in enumerate(edges)})])
    cases["every step a pause"] = (1, 0, None, [([T0 + i for i in range(4097)], [i % 3 for i in range(4097)])])
    cases["equal stamps"] = (1, 0, None, [([T0] * 600, [7] * 600)])
    cases["backward steps"] = (1000, 0, None, [([T0 + 5000 * (i % 3) for i in range(700)], [i % 4 for i in range(700)])])
    # (the sum of the pauses stays below 2^63: powers up to 2^59, then the widest step the stamps allow)
    edge_steps = [0, 1, 2, 3, 4] + [x for k in range(3, 60) for x in ((1 << k) - 1, 1 << k)]
    cases["bucket edges"] = (1, 0, None, [_steps(edge_steps)])
    cases["the widest step"] = (1000, 0, None, [([-(1 << 61), 1 << 61, NONE, 1 << 61], [1, 2, 3, 4])])
    cases["steps of min_ms and min_ms - 1"] = (1000, 0, None, [([T0, T0 + 1000, T0 + 1999, T0 + 2999, T0 + 3998], [1, 2, 3, 4, 5])])
    cases["a carry with line_base > 0"] = (1000, 4000, (T0 - 1500, 3990, -77), [_at(300, {3: T0, 9: T0 + 20, 200: T0 + 5000})])
    cases["a carry and no stamp"] = (1000, 10, (T0, 2, 55), [_at(40, {})])
    cases["an empty carry with line_base > 0"] = (1000, 4000, None, [_at(300, {3: T0, 200: T0 + 5000})])
    whole = _at(6000, {10: T0, 2999: T0 + 10, 3000: T0 + 4010, 3100: T0 + 4020, 3900: T0 + 9020, 5999: T0 + 9030})
    cases["two calls, cut between the lines of a pause"] = (1000, 0, None, [tuple(c[:3000] for c in whole), tuple(c[3000:] for c in whole)])
    cases["two calls, cut inside unstamped lines"] = (1000, 0, None, [tuple(c[:3500] for c in whole), tuple(c[3500:] for c in whole)])
    cases["three calls, the middle one without a stamp"] = (1000, 0, None, [tuple(c[:3200] for c in whole), tuple(c[3200:3800] for c in whole),
                                                                        tuple(c[3800:] for c in whole)])
    return cases


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """[(rows, stats, hist, carry)] of the runs of the case ``name``."""
    min_ms, base, carry, runs = scan_cases()[name]
    out = []
    for ts, sig in runs:
        out.append(reference(ts, sig, min_ms, base, carry))
        carry, base = out[-1][3], base + len(ts)
    return out


def run_case(name: str, device):
    """[(rows, stats, hist, carry)] of the case from ``K.pause_scan`` on ``device``, as lists."""
    min_ms, base, carry, runs = scan_cases()[name]
    out = []
    for ts, sig in runs:
        t = torch.tensor(ts, dtype=torch.int64, device=device)
        s = torch.tensor(sig, dtype=torch.int64, device=device)
        rows, stats, hist, carry = K.pause_scan(t, s, min_ms, base, carry)
        assert all(c.dtype == torch.int64 and c.device == t.device for c in rows + (stats, hist))
        out.append((list(zip(*(c.tolist() for c in rows))), stats.tolist(), hist.tolist(), carry))
        base += len(ts)
    return out


# ---- the report

KEYS = {"totalLines", "stampedLines", "steps", "backwardSteps", "minPauseMs", "pauses", "pausedMs", "spanMs", "pausedShare",
        "firstTimestamp", "lastTimestamp", "intervals", "longest", "templates"}
LONGEST_KEYS = {"ms", "fromLine", "toLine", "from", "to", "linesBetween", "before", "after", "signature"}
TEMPLATE_KEYS = {"signature", "pauses", "lines", "share", "totalMs", "maxMs", "maxLine", "firstLine", "template", "example"}


@functools.lru_cache(maxsize=None)
def report_log():
    """(text, planted): the 4000-line pause log, every 11th line ending in CRLF."""
    text, planted = pause_log(4000, log_templates(30, 1), seed=2)
    lines = text.split("\n")
    for i in range(7, 4000, 11):
        lines[i] += "\r"
    return "\n".join(lines), planted


def parameter_sets():
    sets = [{"by": by} for by in ("before", "after")] + [{"order": o, "min_ms": 300} for o in golden.PAUSE_ORDERS]
    sets += [{"min_ms": 300, "min_count": 3, "order": "count"}, {"min_ms": 350, "top": None, "by": "after"},
             {"min_ms": 1, "top": None}, {"min_ms": 1, "top": 3, "order": "share"}]
    return sets


@functools.lru_cache(maxsize=None)
def wanted():
    """The specification's report per parameter set, computed once."""
    text, _ = report_log()
    return [golden.pauses(text, **kw) for kw in parameter_sets()]
