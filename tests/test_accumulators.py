"""The host side that the report accumulators share, on the CPU engine (log_parser_amd/accumulator.py,
pieces.py, the table base of ops/kernels.py): mixed sources continue one log for every accumulator
that continues a log, the gap accumulator's sources are documents of a corpus, the example ledger
keeps the smallest ordinal, the join of table rows by key, and one growth scenario over both tables."""
import random

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.accumulator import Examples
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.pieces import stream_lines
from log_parser_amd.utils.config import Config

W = 96                      # bytes per line, line end included: a chunk of k * W bytes holds k lines
CUTS = (23, 41)             # the log's three parts: lines [0, 23), [23, 41), [41, 60)
CHUNK_LINES = (1, 7, 60)
HEALTHY = "INFO boot ok\n2024-05-01T09:59:00.000Z INFO tick 1 pad=x\n"


def _library():
    return [PatternSet.model_validate({"metadata": {"library_id": "acc"}, "patterns": [
        {"id": "boom", "name": "boom", "severity": "HIGH",
         "primary_pattern": {"regex": r"BOOM", "confidence": 0.9},
         "context_extraction": {"lines_before": 2, "lines_after": 1}}]})]


def _log():
    """60 lines of W bytes: stamped lines a second apart with a numeric field, two silences (one of
    them across the second cut), event lines (one just behind the first cut: the lines before the
    cut are in its lead-up and inside its context window), error lines that no event covers (one
    just before the second cut), two stack traces away from the cuts, and an unstamped line as the
    first line of the second and third part (its time is the previous part's last)."""
    t = [0]

    def stamped(body, step=1000):
        t[0] += step
        return "2024-05-01T10:%02d:%02d.%03dZ %s" % (t[0] // 60000, t[0] // 1000 % 60, t[0] % 1000, body)

    def frame(k):
        return "\tat com.acme.%s.run(Worker.java:%d)" % ("W" * (W - 34), k)        # (padded inside the class name)

    rng = random.Random(4)
    lines = []
    for i in range(60):
        if i in (6, 24, 25, 50):
            lines.append(stamped("ERROR worker %d: BOOM" % rng.randrange(100)))
        elif i in (10, 30):
            lines.append(stamped("ERROR request %d failed: java.lang.IllegalStateException: bad state" % i))
        elif i in (11, 12, 31, 32, 34):
            lines.append(frame(i))
        elif i == 33:
            lines.append("Caused by: java.io.IOException: disk " + "d" * 40)
        elif i in CUTS:
            lines.append("  continued without a stamp %d" % i)
        elif i in (3, 18, 40, 55):
            lines.append(stamped("ERROR cache shard %d lost quorum" % rng.randrange(64)))
        elif i == 42:
            lines.append(stamped("INFO [gateway] woke up after %dms" % 95000, step=95000))
        elif i == 20:
            lines.append(stamped("INFO [gateway] served request in %dms" % 31000, step=4000))
        elif i >= 45 and i % 2:
            lines.append(stamped("WARN [late] queue depth %d of 512MB" % rng.randrange(1, 900)))
        else:
            lines.append(stamped("INFO [gateway] served request in %dms" % rng.randrange(5, 50)))
    out = []
    for x in lines:
        out.append(x if len(x) == W - 1 else x + " " + "x" * (W - 2 - len(x)))
    assert all(len(x) == W - 1 for x in out)
    return "".join(x + "\n" for x in out).encode()


@pytest.fixture(scope="module")
def case():
    """(CPU parser, the whole log, its three parts)."""
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    data = _log()
    a, b = CUTS[0] * W, CUTS[1] * W
    return lp, data, (data[:a], data[a:b], data[b:])


def _feed(lp, acc, parts, k):
    """The three parts as a document, a stream in chunks of ``k`` lines and a resident log."""
    a, b, c = parts
    acc.add_document(a)
    acc.add_stream(b, k * W)
    acc.add_resident(lp.load_resident(c))
    return acc


REPORTS = {
    "novelty": (lambda lp: lp._novelty_accumulator(_baseline(lp)), lambda acc: acc.report(None, "first"),
                lambda lp, d: golden.novelty(d, [HEALTHY], _library(), lp.config.scoring, None, "first")),
    "leadup": (lambda lp: lp.leadup_accumulator(3), lambda acc: acc.report(None, "share", 1),
               lambda lp, d: golden.leadup(d, _library(), lp.config.scoring, 3, None, "share", 1)),
    "traces": (lambda lp: lp._trace_accumulator(), lambda acc: acc.report(None),
               lambda lp, d: golden.traces(d, _library(), lp.config.scoring, None)),
    "values": (lambda lp: lp.value_accumulator(), lambda acc: acc.report(None, "first", 1, 0.0, False),
               lambda lp, d: golden.values(d, None, "first", 1, 0.0, False)),
    "trends": (lambda lp: lp.trend_accumulator(60), lambda acc: acc.report(min_count=1, kind="all", top=None),
               lambda lp, d: golden.trends(d, bucket_seconds=60, min_count=1, kind="all", top=None)),
    "pauses": (lambda lp: lp.pause_accumulator(2000, "before", None), lambda acc: acc.report(top=None),
               lambda lp, d: golden.pauses(d, 2000, "before", top=None)),
    "timeline": (lambda lp: lp._timeline_accumulator(60, 65536), lambda acc: acc.report(),
                 lambda lp, d: golden.timeline(d, _library(), lp.config.scoring, 60)),
}


def _baseline(lp):
    base = lp.baseline()
    base.add_document(HEALTHY)
    return base


def test_the_log_is_what_it_says(case):
    lp, data, parts = case
    assert len(data) == 60 * W and b"".join(parts) == data and [len(p) // W for p in parts] == [23, 18, 19]
    for k in CHUNK_LINES:
        with stream_lines(lp.engine, parts[1], k * W) as pieces:
            runs = [(p.ls.numel(), p.line_base, p.ev_line.numel(), p.last) for p in pieces]
        assert [n for n, _, _, _ in runs] == [k] * (18 // k) + ([18 % k] if 18 % k else [])
        assert [b for _, b, _, _ in runs] == [sum(n for n, _, _, _ in runs[:j]) for j in range(len(runs))]
        assert all(e == 0 for _, _, e, _ in runs) and [x for _, _, _, x in runs] == [False] * (len(runs) - 1) + [True]
    s = lp.config.scoring
    tr = golden.traces(data, _library(), s, None)
    assert tr["traces"] == 2 and tr["events"] == 4
    lead = {x for x in range(60) if any(x < e <= x + 3 for e in (6, 24, 25, 50))}
    assert golden.leadup(data, _library(), s, 3, None, "share", 1)["leadLines"] == len(lead) == 10
    assert [r["ms"] for r in golden.pauses(data, 2000, "before", top=None)["longest"]] == [95000, 4000]
    assert golden.values(data, None, "first", 1, 0.0, False)["fields"] >= 4
    assert golden.timeline(data, _library(), s, 60)["undatedLines"] == 0
    assert golden.novelty(data, [HEALTHY], _library(), s, None, "first")["templates"] >= 5


@pytest.mark.parametrize("k", CHUNK_LINES)
@pytest.mark.parametrize("name", sorted(REPORTS))
def test_mixed_sources_continue_one_log(case, name, k):
    """A document, a stream and a resident log, one after the other, are ONE log: the report of the
    three parts is the one-document report of their concatenation (for traces too: the cuts lie
    between the traces, and a trace does not continue across sources)."""
    lp, data, parts = case
    make, report, want = REPORTS[name]
    assert report(_feed(lp, make(lp), parts, k)) == want(lp, data)


def test_timeline_accumulator_takes_a_document(case):
    lp, data, _ = case
    acc = lp._timeline_accumulator(60, 65536)
    acc.add_document(data)
    assert acc.report() == lp.engine.timeline_bytes(data, bucket_seconds=60) == lp.timeline(data)
    assert acc.lines == 60


@pytest.mark.parametrize("cover", ["context", "events"])
def test_gap_accumulator_sources_are_documents(case, cover):
    lp, data, parts = case
    sets, s = _library(), lp.config.scoring
    for k in CHUNK_LINES:
        got = _feed(lp, lp.gap_accumulator(cover), parts, k).report(None)
        assert got == golden.gaps_corpus(list(parts), sets, s, None, cover) and got["documents"] == 3
    assert got["uncoveredErrorLines"] > 0
    for add in (lambda acc: acc.add_document(data), lambda acc: acc.add_stream(data, 7 * W),
                lambda acc: acc.add_resident(lp.load_resident(data))):
        acc = lp.gap_accumulator(cover)
        add(acc)
        assert acc.report(None) == lp.engine.gaps_bytes(data, top=None, cover=cover) == golden.gaps(data, sets, s, None, cover)


# ---- the example ledger

def test_ledger_keeps_the_smallest_ordinal():
    cand = [(5, 9, b"late"), (5, 3, b"early"), (-7, 4, b"other"), (5, 7, b"middle"), (-7, 8, b"other, later")]
    for order in (cand, cand[::-1], sorted(cand, key=lambda c: c[1])):
        single, tensor = Examples("Some"), Examples("Some")
        for key, ordinal, raw in order:
            single.put(key, ordinal, raw)
        key = torch.tensor([c[0] for c in order] + [11])                # (a pair that is no winner: not recorded)
        ordinal = torch.tensor([c[1] for c in order] + [0])
        tensor.record(key, ordinal, torch.arange(len(order)), [c[2] for c in order])
        for ex in (single, tensor):
            assert ex.take(5, 3) == b"early" and ex.take(-7, 4) == b"other"
            with pytest.raises(KeyError):
                ex.take(11, 0)
    ex = Examples("Some")
    ex.put(-7, 4, (1, b"payload"))
    assert ex.take(-7, 4) == (1, b"payload")
    with pytest.raises(RuntimeError, match="Some: the example of %016x is not its first line" % ((1 << 64) - 7)):
        ex.take(-7, 3)


# ---- the join

def test_lookup_matches_a_dict():
    rng = random.Random(2)
    keys = [K.GT_EMPTY, 0, -1, (1 << 63) - 1] + [rng.randrange(-(1 << 63), 1 << 63) for _ in range(40)]
    pairs = [(rng.choice(keys), rng.randrange(1 << 40)) for _ in range(500)]
    want = {}
    for k, o in pairs:
        c, f = want.get(k, (0, o))
        want[k] = (c + 1, min(f, o))
    table = K.GapTable("cpu")
    table.fold(torch.tensor([k for k, _ in pairs]), torch.tensor([o for _, o in pairs]), winners=False)
    absent = [k + 1 for k in keys if k + 1 not in want and k + 1 < 1 << 63]
    assert K.GT_EMPTY in want and len(absent) > 30
    ask = keys + absent + keys[:3]
    count, first, found, groups = table.lookup(torch.tensor(ask))
    assert groups == len(want) and found.dtype == torch.bool
    assert list(zip(count.tolist(), first.tolist())) == [want.get(k, (0, 0)) for k in ask]
    assert found.tolist() == [k in want for k in ask]
    by_key = sorted(want.items())
    assert [c.tolist() for c in table.sorted_rows()] == [[k for k, _ in by_key], [v[0] for _, v in by_key], [v[1] for _, v in by_key]]
    for t in (K.GapTable("cpu"), table):
        count, first, found, _ = t.lookup(torch.empty(0, dtype=torch.int64))
        assert count.numel() == first.numel() == found.numel() == 0
    count, first, found, groups = K.GapTable("cpu").lookup(torch.tensor(ask))
    assert groups == 0 and not found.any() and not count.any() and not first.any() and count.numel() == len(ask)


# ---- the table base: one scenario over both tables

def _gap_side():
    state = {}

    def fold(table, idx, done):
        sig = [k * 0x9E3779B97F4A7C15 % (1 << 64) - (1 << 63) for k in idx]
        ords = [(7 * j + 3) % 1000 for j in range(done, done + len(idx))]
        for s, o in zip(sig, ords):
            c, f = state.get(s, (0, o))
            state[s] = (c + 1, min(f, o))
        table.fold(torch.tensor(sig), torch.tensor(ords), winners=False)

    def rows(table):
        sig, count, first, docs = table.rows()
        assert docs.tolist() == [1] * sig.numel()
        return dict(zip(sig.tolist(), zip(count.tolist(), first.tolist())))

    return K.GapTable, fold, rows, state, lambda t, a, b: t.fold(a, b)


def _cell_side():
    state, cw = {}, 1000

    def fold(table, idx, done):
        sig = [k % 20 - 10 for k in idx]
        eff = [K.TS_NONE if k // 20 == 14 else (k // 20 - 3) * cw + k % 7 for k in idx]       # (negative times too)
        for j, (s, e) in enumerate(zip(sig, eff)):
            cell = (s, K.CT_UNDATED if e == K.TS_NONE else e // cw)
            c, f = state.get(cell, (0, done + j))
            state[cell] = (c + 1, min(f, done + j))
        table.fold(torch.tensor(sig), torch.tensor(eff), done, cw)

    def rows(table):
        sig, bucket, count, first = table.rows()
        return dict(zip(zip(sig.tolist(), bucket.tolist()), zip(count.tolist(), first.tolist())))

    return K.CellTable, fold, rows, state, lambda t, a, b: t.fold(a, b, 0, cw)


@pytest.mark.parametrize("side", [_gap_side, _cell_side])
def test_tables_grow_by_one_rule(side):
    cls, fold, rows, state, bad_fold = side()
    table = cls("cpu", cap=2, tile=256)
    assert table.cap == 2 and table.used == 0 and rows(table) == {}
    rng = random.Random(8)
    idx = list(range(300)) + [rng.randrange(300) for _ in range(228)]        # 300 distinct keys, some of them again
    rng.shuffle(idx)
    done, caps = 0, []
    for n in (1, 7, 256, 1, 7, 256):
        fold(table, idx[done:done + n], done)
        done += n
        assert rows(table) == state
        used = table.used
        assert used == len(state) and table.cap & (table.cap - 1) == 0 and 2 * used <= table.cap
        caps.append(table.cap)
    assert done == len(idx) and table.used == 300 and caps == sorted(caps) and caps[0] == 2 and caps[2] >= 512
    name = cls.__name__
    with pytest.raises(ValueError, match=name + ": cap must be a power of two"):
        cls("cpu", cap=6)
    with pytest.raises(ValueError, match=name + ": tile must be 256"):
        cls("cpu", tile=100)
    with pytest.raises(ValueError, match=name + ".fold: .* differ in length"):
        bad_fold(table, torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    assert rows(table) == state
