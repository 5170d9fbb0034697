"""Cases for the cadence tests (test_cadence.py, test_gpu_cadence.py): runs of (ts, sig) for
``K.beat_scan`` with a plain Python loop as the reference -- a dict of the last stamped line per
signature -- and the 4000-line log with its parameter sets."""
import functools
import random

import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils import synth

NONE = K.TS_NONE
TILE = K.CD_TILE
T0 = 1_758_283_200_000
BIG = 1 << 61


def signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


def _mix(n: int, seed: int, unstamped: float = 0.2, n_sigs: int = 40):
    """A skewed mix: few templates hold most lines, stamps mostly move on, now and then back."""
    rng = random.Random(seed)
    sigs = [signed(rng.getrandbits(64)) for _ in range(n_sigs)]
    weights = [1.0 / (k + 1) for k in range(n_sigs)]
    t = T0
    ts = []
    for _ in range(n):
        t += rng.choice((0, 1, 1, 7, 50, 400, 9_000, -30))
        ts.append(NONE if rng.random() < unstamped else t)
    return ts, rng.choices(sigs, weights=weights, k=n)


def _cut(run, *cuts):
    ts, sig = run
    edges = [0] + list(cuts) + [len(ts)]
    return [(ts[a:b], sig[a:b]) for a, b in zip(edges, edges[1:])]


@functools.lru_cache(maxsize=None)
def scan_cases():
    """name -> [(ts, sig), ...]: the runs of one log, in order."""
    cases = {"n=%d" % n: [_mix(n, n)] for n in (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097)}
    # more than 256 * 256 rows: every block edge of the link kernels, two blocks per lane of its prefix
    n = 256 * 256 + 300
    cases["rows past every link block"] = [([T0 + i for i in range(n)], [i % 30_000 - 7 for i in range(n)])]
    # one template on the first line of 300 tiles and nowhere else: a segment wider than a link block
    n = 300 * TILE
    cases["one row per tile, 300 tiles"] = [([T0 + i if i % TILE == 0 else NONE for i in range(n)], [5] * n)]
    cases["one signature on every line"] = [([T0 + 3 * i for i in range(2 * TILE + 5)], [-9] * (2 * TILE + 5))]
    cases["all signatures distinct"] = [([T0 + i for i in range(2 * TILE)], list(range(-TILE, TILE)))]
    # once per tile: border beats only; the second template on the first and the last line of tiles
    n = 3 * TILE + 10
    sig = [100 + i for i in range(n)]
    for k in range(4):
        sig[k * TILE + 7] = 1
    for i in (0, TILE - 1, TILE, 2 * TILE - 1, 3 * TILE - 1, 3 * TILE):
        sig[i] = 2
    cases["borders only; first and last lines of tiles"] = [([T0 + 11 * i for i in range(n)], sig)]
    # a tile without any stamp between two occurrences
    n = 3 * TILE
    cases["a tile without a stamp between"] = [([T0 + i if not TILE <= i < 2 * TILE else NONE for i in range(n)],
                                                [i % 3 for i in range(n)])]
    cases["no stamp at all"] = [([NONE] * (TILE + 3), [i % 5 for i in range(TILE + 3)])]
    cases["equal stamps"] = [([T0] * 300, [i % 2 for i in range(300)])]
    cases["backward beats"] = [([T0 - 5 * i for i in range(600)], [i % 3 for i in range(600)]),
                               ([T0 - 10_000, T0, T0 - 1], [0, 0, 0])]
    # beats at every bucket edge 2^k - 1, 2^k, then the widest beat of all
    ts, t = [0], 0
    for k in range(1, 61):
        for d in ((1 << k) - 1, 1 << k):
            t += d
            ts.append(t)
    cases["bucket edges"] = [(ts, [3] * len(ts))]
    cases["widest beat"] = [([5, -BIG, BIG], [3, 4, 4]), ([BIG, -BIG], [4, 4])]
    # two equal maxima: inside a tile; the border beat (lines 2047 -> 2048) and a later one
    cases["equal maxima inside a tile"] = [([0, 10, 510, 520, 1020, 1030], [6] * 6)]
    ts = [NONE] * (TILE + 40)
    for i, t in ((5, 0), (TILE - 1, 100), (TILE, 1100), (TILE + 9, 1200), (TILE + 30, 2200)):
        ts[i] = t
    cases["equal maxima, one the border beat"] = [(ts, [6] * len(ts))]
    ts = list(ts)
    ts[3] = -1000                                  # ... and an earlier one inside the first tile
    cases["equal maxima, the border beat second"] = [(ts, [6] * len(ts))]
    cases["empty marker as a signature"] = [([T0, T0 + 5, NONE, T0 + 9, T0 + 20], [K.GT_EMPTY, 3, K.GT_EMPTY, K.GT_EMPTY, 3])]
    cases["skewed mix"] = [_mix(3 * TILE + 123, 77)]
    # several runs with state
    cases["cut between the lines of a beat"] = _cut(([T0, T0 + 70, T0 + 4070, T0 + 4080], [8, 8, 8, 8]), 2)
    mix = _mix(5000, 5)
    for i in range(2100, 2400):
        mix[0][i] = NONE
    cases["a middle run without a stamp"] = _cut(mix, 2100, 2400)
    ts, sig = _mix(5000, 6)
    sig = [12345 if i % 40 == 0 and not 1500 <= i < 3800 else s for i, s in enumerate(sig)]
    cases["a template absent from a middle run"] = _cut((ts, sig), 1500, 3800)
    cases["many small runs"] = _cut(_mix(4500, 9), *range(37, 4500, 211))
    return cases


def bucket(beat: int) -> int:
    return golden.pause_bucket(beat) if beat >= 0 else NONE


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(beat per run, bkt per run, state rows sorted by signature) by the definition: one walk in
    line order with a dict."""
    rows = {}
    beats, bkts = [], []
    line = 0
    for ts, sig in scan_cases()[name]:
        beat, bkt = [NONE] * len(ts), [NONE] * len(ts)
        for i, (t, s) in enumerate(zip(ts, sig)):
            g = line + i
            if t == NONE:
                continue
            r = rows.get(s)
            if r is None:
                rows[s] = {"lines": 1, "beats": 0, "back": 0, "sum": 0, "min": K.I64_MAX, "max": -1, "from": -1, "to": -1,
                           "to_ts": 0, "first": g, "first_ts": t, "last": g, "last_ts": t}
                continue
            beat[i] = t - r["last_ts"]
            bkt[i] = bucket(beat[i])
            r["lines"] += 1
            if beat[i] < 0:
                r["back"] += 1
            else:
                r["beats"] += 1
                r["sum"] += beat[i]
                r["min"] = min(r["min"], beat[i])
                if beat[i] > r["max"]:
                    r["max"], r["from"], r["to"], r["to_ts"] = beat[i], r["last"], g, t
            r["last"], r["last_ts"] = g, t
        beats.append(beat)
        bkts.append(bkt)
        line += len(ts)
    state = [(s, r["lines"], r["beats"], r["back"], r["sum"], r["min"], r["max"], r["from"], r["to"], r["first"], r["last"],
              r["last_ts"], r["first_ts"], r["to_ts"]) for s, r in sorted(rows.items())]
    return beats, bkts, state


def state_rows(state: torch.Tensor):
    return [tuple(r) for r in state.t().cpu().tolist()]


def run_runs(runs, device, cap=None):
    """``K.beat_scan`` over the runs of one log: (beat per run, bkt per run, state rows)."""
    state, line = None, 0
    beats, bkts = [], []
    for ts, sig in runs:
        t = torch.tensor(ts, dtype=torch.int64, device=device)
        s = torch.tensor(sig, dtype=torch.int64, device=device)
        beat, bkt, state = K.beat_scan(t, s, line, state, cap=cap)
        assert state.shape[0] == K.CD_COLS and state.is_contiguous() and state.device == t.device
        beats.append(beat.cpu().tolist())
        bkts.append(bkt.cpu().tolist())
        line += len(ts)
    return beats, bkts, state_rows(state)


def run_case(name: str, device, cap=None):
    return run_runs(scan_cases()[name], device, cap)


def joined(name: str):
    """The runs of a case as one run."""
    runs = scan_cases()[name]
    return [(sum((r[0] for r in runs), []), sum((r[1] for r in runs), []))]


# ---- the report

@functools.lru_cache(maxsize=None)
def report_log():
    """(text, the three plants' numbers) of the 4000-line log of the report tests."""
    return synth.cadence_log(4000, synth.log_templates(40, seed=3), seed=11)


def parameter_sets():
    return [{},
            {"kind": "all", "top": None},
            {"kind": "missed", "order": "count"},
            {"kind": "stopped", "order": "overdue"},
            {"kind": "all", "order": "first", "min_regularity": 0, "top": None},
            {"kind": "all", "order": "count", "min_regularity": 0, "min_count": 1, "top": 7},
            {"min_ms": 60_000, "ratio": 2},
            {"order": "gap", "ratio": 12, "min_ms": 1, "top": 1},
            {"kind": "all", "min_regularity": 0.5, "min_count": 30, "order": "overdue"}]


@functools.lru_cache(maxsize=None)
def wanted():
    text, _ = report_log()
    return [golden.cadence(text, **kw) for kw in parameter_sets()]
