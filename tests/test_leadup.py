"""Lead-up report on the CPU engine (log_parser_amd/leadup.py, csrc/kernels/leadup.hip host twin):
the sign-and-mark pass against ``golden.line_signature`` and the lead-up predicate, the report
against ``golden.leadup`` for documents, streams in chunks of any size and resident logs, the
pending carry between pieces, side effects, guards and the command line."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd import leadup as LU
from log_parser_amd.api import LogParser
from log_parser_amd.models.library import load_pattern_directory
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.pieces import stream_pieces
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, templated_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
KEYS = {"totalLines", "events", "eventLines", "window", "leadLines", "templates", "top"}
GROUP_KEYS = {"count", "total", "share", "lift", "firstLine", "signature", "template", "example"}
CPU = {"engine.device": "cpu"}


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


# ---- 1. the host twin against the specification's predicate

def _stage(data: bytes) -> torch.Tensor:
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return text


def test_host_twin_matches_golden():
    rng = random.Random(3)
    lines = [bytes(rng.choice(b"ab1 9\tZ-.:") for _ in range(n)) for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 5000)]
    lines += [b"a \t\t  b\t \tc", b"caf\xc3\xa9 \xff\xfe 42 \x80\x80abc1\x80", b"retry in 30", b"", b"x" * 1020 + b" tail AAAA"]
    lines += [b"INFO step %d of %d" % (i, rng.randrange(99)) for i in range(40)] + [b"end"]
    data = b"\n".join(lines)
    text = _stage(data)
    ls, ll = K.split_lines(text, len(data))
    L = len(lines)
    assert ls.numel() == L
    sigs = [_signed(golden.line_signature(x)) for x in lines]
    for events in ([], [0], [L - 1], [0, L - 1], [20, 21], list(range(L)), sorted(rng.sample(range(L), 5))):
        ev = torch.tensor(events, dtype=torch.int32)
        for W in (1, 2, 7, 50, 4096):
            want = [any(x < e <= x + W for e in events) for x in range(L)]
            pairs = [(x, sigs[x]) for x in range(L) if want[x]]
            for cap in (None, L, 1, 0, max(0, len(pairs) - 1)):       # cap below the count: the re-run
                for e in ((ev, None) if not events else (ev,)):
                    sig, lead, line, psig, n = K.lead_lines(text, ls, ll, e, W, cap=cap)
                    assert sig.dtype == torch.int64 and lead.dtype == torch.uint8 and line.dtype == torch.int32
                    assert psig.dtype == torch.int64 and n == len(pairs)
                    assert sig.tolist() == sigs and lead.tolist() == [int(w) for w in want]
                    assert list(zip(line.tolist(), psig.tolist())) == pairs      # (the twin appends in line order)
    none = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int32)
    sig, lead, line, psig, n = K.lead_lines(text, *none, torch.tensor([3], dtype=torch.int32), 5)
    assert (sig.numel(), lead.numel(), line.numel(), psig.numel(), n) == (0, 0, 0, 0, 0)
    for bad in (lambda: K.lead_lines(text, ls, ll, None, 0), lambda: K.lead_lines(text, ls, ll, None, 4097),
                lambda: K.lead_lines(text, ls, ll, torch.tensor([1], dtype=torch.int64), 5),
                lambda: K.lead_lines(text, ls, ll, torch.tensor([[1]], dtype=torch.int32), 5),
                lambda: K.lead_lines(text, ls, ll, torch.tensor([1, 2, 3, 4], dtype=torch.int32)[::2], 5),
                lambda: K.lead_lines(text, ls, ll, None, 5, per_block=4096)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. the report against golden.leadup: a templated log with the example library

@pytest.fixture(scope="module")
def example():
    """(pattern sets of the example library, a CPU parser on them, a templated log of 80 templates
    plus two that the library matches, on ~0.3 % of the lines each)."""
    sets = load_pattern_directory(PAT)
    lp = LogParser(sets, config=Config.load(overrides=CPU))
    temps = log_templates(80, seed=5) + ["%02d:%02d:%03d java.lang.OutOfMemoryError: Java heap space %d",
                                         "%02d:%02d:%03d WARN  [kubelet] Liveness probe failed: timeout %d"]
    return sets, lp, templated_log(3000, temps, seed=7, crlf_rate=0.1)


@pytest.mark.parametrize("order", ["share", "count", "first"])
def test_report_equals_golden(example, order):
    sets, lp, log = example
    full = golden.leadup(log, sets, lp.config.scoring, top=None, order=order, min_count=1)
    assert full["events"] >= full["eventLines"] > 3 and full["window"] == 50
    assert 0 < full["leadLines"] < full["totalLines"] // 2 and full["templates"] == len(full["top"]) > 20
    assert sum(g["count"] for g in full["top"]) == full["leadLines"]
    for top in (None, 2):
        for min_count in (1, 2):
            want = golden.leadup(log, sets, lp.config.scoring, 50, top, order, min_count)
            got = lp.leadup(log, top=top, order=order, min_count=min_count)
            assert got == want and set(got) == KEYS
            assert all(set(g) == GROUP_KEYS for g in got["top"])
            assert {k: v for k, v in got.items() if k != "top"} == {k: v for k, v in full.items() if k != "top"}
            assert all(g["count"] >= min_count for g in got["top"])
            assert len(got["top"]) == (2 if top else sum(g["count"] >= min_count for g in full["top"]))
    rows = lp.leadup(log, top=None, order=order, min_count=1)["top"]
    key = {"share": lambda g: (-g["share"], -g["count"], g["firstLine"]), "count": lambda g: (-g["count"], g["firstLine"]),
           "first": lambda g: g["firstLine"]}[order]
    assert rows == sorted(rows, key=key)
    for g in rows:
        assert g["share"] == g["count"] / g["total"] and 0 < g["count"] <= g["total"]
        assert g["lift"] == (g["count"] * full["totalLines"]) / (g["total"] * full["leadLines"])


@pytest.mark.parametrize("window", [1, 2, 50, 4096])
def test_windows(example, window):
    sets, lp, log = example
    want = golden.leadup(log, sets, lp.config.scoring, window, None, "share", 1)
    assert lp.leadup(log, window=window, top=None, min_count=1) == want
    assert lp.leadup_stream(log.encode(), chunk_bytes=4096, window=window, top=None, min_count=1) == want
    assert want["window"] == window and want["leadLines"] >= want["eventLines"] - 1
    if window == 4096:                                            # every line before the last event
        assert want["leadLines"] == max(e["lineNumber"] for e in lp.parse(log)["events"]) - 1 > 2000


# ---- 3. boundaries, each against golden: a library of one word

def _boom_library():
    """An event on every line that says BOOM (with a context window: it must not matter), a second
    pattern on some of the same lines (two events, one event line)."""
    return [PatternSet.model_validate({"metadata": {"library_id": "leadup"}, "patterns": [
        {"id": "boom", "name": "boom", "severity": "CRITICAL", "primary_pattern": {"regex": r"BOOM", "confidence": 0.9},
         "context_extraction": {"lines_before": 2, "lines_after": 1}},
        {"id": "big", "name": "big boom", "severity": "HIGH", "primary_pattern": {"regex": r"BIG BOOM", "confidence": 0.8}}]})]


QUIET = ["INFO request %d served in %dms", "DEBUG cache shard %d hit ratio 0.%d", "WARN pool exhausted, waiting %dms",
         "INFO héartbeat from node-%d", "WARN GC pause %dms", ""]


def _fill(rng, t: str) -> str:
    return t % tuple(rng.randrange(1000) for _ in range(t.count("%d")))


def _boom_log(n: int, events, seed: int = 0, eol: str = "\n", width: int = 0) -> str:
    """``n`` lines of the quiet templates with ``ERROR ... BOOM`` on the lines ``events``; ``width``:
    every line padded to that many bytes, line end included (chunks of k * width bytes hold k lines)."""
    rng = random.Random(seed)
    lines = [_fill(rng, rng.choice(QUIET)) for _ in range(n)]
    lines[-1] = lines[-1] or "INFO done"                         # (trailing empty lines are no lines)
    for k, e in enumerate(events):
        lines[e] = "ERROR worker %d: %sBOOM" % (rng.randrange(100), "BIG " if k % 3 == 1 else "")
    if width:
        lines = [x + " " * (width - len(eol) - len(x.encode())) for x in lines]
        assert all(len(x.encode()) == width - len(eol) for x in lines)
    return "".join(x + eol for x in lines)


@pytest.fixture(scope="module")
def boom():
    return LogParser(_boom_library(), config=Config.load(overrides=CPU))


def _golden(lp, log, **kw):
    return golden.leadup(log, _boom_library(), lp.config.scoring, **kw)


BOUNDARIES = {
    "event on line 0": (30, [0]),
    "event on the last line": (30, [29]),
    "first and last": (30, [0, 29]),
    "exactly window and window + 1 before": (30, [20]),          # window 5: line 15 is in, line 14 is out
    "two adjacent event lines": (30, [11, 12]),
    "every line an event": (12, list(range(12))),
    "no event at all": (30, []),
    "one line, an event": (1, [0]),
}


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_boundaries(boom, name):
    n, events = BOUNDARIES[name]
    log = _boom_log(n, events, seed=len(name))
    for window in (1, 5, 50):
        want = _golden(boom, log, window=window, top=None, order="first", min_count=1)
        lead = {x for x in range(n) if any(x < e <= x + window for e in events)}
        assert want["totalLines"] == n and want["eventLines"] == len(events) and want["leadLines"] == len(lead)
        assert want["events"] == len(events) + len(events[1::3])                  # (BIG BOOM: two events on one line)
        assert {g["firstLine"] - 1 for g in want["top"]} <= lead and sum(g["count"] for g in want["top"]) == len(lead)
        for got in (boom.leadup(log, window=window, top=None, order="first", min_count=1),
                    boom.leadup_stream(log.encode(), chunk_bytes=64, window=window, top=None, order="first", min_count=1)):
            assert got == want, (name, window)
    if name.startswith("exactly"):
        got = boom.leadup(log, window=5, top=None, order="first", min_count=1)
        assert got["leadLines"] == 5 and got["top"][0]["firstLine"] == 16         # line 15 (0-based) is the first one in
    if not events:
        assert want["leadLines"] == 0 and want["templates"] == 0 and want["top"] == []


def test_empty_and_crlf_logs(boom):
    for log in ("", "\n", "\r\n", "BOOM", "BOOM\n", "\n\nBOOM\n", "a\r\nb\r\nBOOM\r\nc\r\n", "a\r\nBOOM\nb\r\n\r\n"):
        want = _golden(boom, log, window=2, top=None, min_count=1)
        for got in (boom.leadup(log, window=2, top=None, min_count=1), boom.leadup(log.encode(), window=2, top=None, min_count=1),
                    boom.leadup_stream(log.encode(), window=2, top=None, min_count=1),
                    boom.leadup_stream(log.encode(), chunk_bytes=2, window=2, top=None, min_count=1)):
            assert got == want, repr(log)
    assert _golden(boom, "", window=2)["totalLines"] == 1 and _golden(boom, "\n", window=2)["totalLines"] == 0
    assert _golden(boom, "", window=2)["top"] == [] == _golden(boom, "\n", window=2)["top"]
    crlf = _boom_log(40, [7, 30], seed=2, eol="\r\n")
    want = _golden(boom, crlf, window=5, top=None, min_count=1)
    assert want["leadLines"] == 10 and all(not g["example"].endswith("\r") for g in want["top"])
    assert boom.leadup(crlf, window=5, top=None, min_count=1) == want
    assert boom.leadup_stream(crlf.encode(), chunk_bytes=100, window=5, top=None, min_count=1) == want


# ---- 4. sources and chunking: the pending carry

LW = 64             # bytes per line, line end included


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_stream_equals_document(boom, eol):
    """60 lines with events on 13, 14 and 40. With 4-line chunks and window 3 the chunk borders at
    lines 4 and 8 are more than a window of event-free lines away from the next event (their
    pending lines are dropped, a few chunks later for the one-line chunks), the border at 12 is not
    (lines 10 and 11 are kept and come into the lead-up of line 13), and line 40 is the first line
    of a chunk (lines 37..39 are in its lead-up, all of them pending)."""
    data = _boom_log(60, [13, 14, 40], seed=5, eol=eol, width=LW).encode()
    for window in (1, 3, 5, 50):
        want = _golden(boom, data, window=window, top=None, min_count=1)
        assert want["totalLines"] == 60 and want["eventLines"] == 3
        assert want["leadLines"] == len({x for x in range(60) if any(x < e <= x + window for e in (13, 14, 40))})
        assert boom.leadup(data, window=window, top=None, min_count=1) == want
        for k in (1, 2, 3, 4, 7, 13, 60):
            with stream_pieces(boom.engine, data, k * LW) as pieces:
                assert max(p.ls.numel() for p in pieces) == k              # one-line chunks up to the whole log
            for order in ("share", "count", "first"):
                got = boom.leadup_stream(data, chunk_bytes=k * LW, window=window, top=None, order=order, min_count=1)
                assert got == _golden(boom, data, window=window, top=None, order=order, min_count=1), (window, k, order)
            assert boom.leadup_stream(data, chunk_bytes=k * LW, window=window, top=2) == _golden(boom, data, window=window, top=2)


def test_pending_keep_and_drop_rules(boom):
    """The carry, piece by piece: one-line chunks, window 3."""
    data = _boom_log(20, [9, 10], seed=6, width=LW).encode()
    acc = LU.LeadupAccumulator(boom.engine, 3)
    seen = []
    with stream_pieces(boom.engine, data, LW) as pieces:
        for piece in pieces:
            acc._add_piece(piece)
            seen.append(([g for g, _, _ in acc._pending], acc.lead))
    assert len(seen) == 20
    assert seen[5] == ([3, 4, 5], 0)              # a line stays pending over `window` one-line pieces, no longer
    assert seen[8] == ([6, 7, 8], 0)
    assert seen[9] == ([9], 3)                    # the event on line 9: 6, 7, 8 resolved; its own line pending
    assert seen[10] == ([10], 4)                  # ... and in the lead-up of the event on line 10, which is pending now
    assert seen[13] == ([11, 12, 13], 4) and seen[14] == ([12, 13, 14], 4)
    assert all(len(p) <= 3 for p, _ in seen)
    assert acc.report(top=None, min_count=1) == _golden(boom, data, window=3, top=None, min_count=1)
    # the raw bytes of a pending line are its example when it is its group's first lead-up line
    assert {g["firstLine"] for g in acc.report(top=None, min_count=1)["top"]} <= {7, 8, 9, 10}


def test_resident_and_path_equal_document(boom, tmp_path):
    log = _boom_log(400, [3, 50, 51, 199, 200, 399], seed=9)
    data = log.encode()
    want = _golden(boom, log, top=None, min_count=1)
    assert want["leadLines"] > 100
    res = boom.load_resident(data, chunk_bytes=2048)
    assert len(res.chunks) > 3
    assert boom.leadup_resident(res, top=None, min_count=1) == want
    assert boom.leadup_resident(res, window=7, top=3, order="count") == _golden(boom, log, window=7, top=3, order="count")
    f = tmp_path / "app.log"
    f.write_bytes(data)
    assert boom.leadup_stream(str(f), chunk_bytes=300, top=None, min_count=1) == want
    assert boom.leadup_file(str(f), top=None, min_count=1) == want
    e = tmp_path / "empty.log"
    e.write_bytes(b"")
    assert boom.leadup_stream(str(e)) == boom.leadup(b"") == _golden(boom, "")


def test_accumulator_continues_one_log(boom):
    """Further sources continue the same log: document + stream + resident == the whole document,
    with a lead-up that straddles both borders (events on the first lines of the later sources)."""
    lines = _boom_log(300, [40, 100, 101, 252, 299], seed=10).split("\n")[:-1]
    lines[99], lines[249] = "INFO last line of the document", "INFO last line of the stream"    # (not empty ones)
    log = "\n".join(lines) + "\n"
    a, b, c = ("\n".join(x) + "\n" for x in (lines[:100], lines[100:250], lines[250:]))
    for window in (2, 50):
        acc = boom.leadup_accumulator(window)
        acc.add_document(a)
        part = acc.report(top=None, min_count=1)                  # (what is pending is in no lead-up yet)
        assert part == _golden(boom, a, window=window, top=None, min_count=1)
        acc.add_stream(b.encode(), chunk_bytes=128)
        acc.add_resident(boom.load_resident(c.encode(), chunk_bytes=1024))
        for order in ("share", "count", "first"):
            assert acc.report(top=None, order=order, min_count=1) == \
                _golden(boom, log, window=window, top=None, order=order, min_count=1)
        assert acc.report() == _golden(boom, log, window=window)
        assert len(acc._pending) <= window


# ---- 5. arguments, side effects and guards

def test_bad_arguments_raise(boom):
    log = _boom_log(20, [10])
    res = boom.load_resident(log.encode())
    for kw in ({"order": "line"}, {"order": ""}, {"window": 0}, {"window": 4097}, {"window": -3}, {"min_count": 0}):
        with pytest.raises(ValueError):
            golden.leadup(log, _boom_library(), boom.config.scoring, **kw)
        for call in (lambda: boom.leadup(log, **kw), lambda: boom.leadup_file(os.path.join(ROOT, "no", "such", "file"), **kw),
                     lambda: boom.leadup_stream(log.encode(), **kw), lambda: boom.leadup_resident(res, **kw),
                     lambda: boom.engine.leadup_bytes(log.encode(), **kw)):
            with pytest.raises(ValueError):
                call()
    for window in (0, 4097):
        with pytest.raises(ValueError):
            boom.leadup_accumulator(window)
    acc = boom.leadup_accumulator(5)
    for kw in ({"order": "Share"}, {"min_count": 0}):
        with pytest.raises(ValueError):
            acc.report(**kw)


def test_frequency_window_untouched():
    log = _boom_log(200, [20, 21, 90, 150], seed=11)
    cfg = Config.load(overrides={"engine.device": "cpu", "scoring.frequency.threshold": "1.0"})
    a, b = LogParser(_boom_library(), config=cfg), LogParser(_boom_library(), config=cfg)
    a.parse(log)
    b.parse(log)
    before = a.frequency_statistics()
    assert before and a.leadup(log)["events"] > 0
    assert a.leadup_stream(log.encode(), chunk_bytes=300)["events"] > 0
    assert a.leadup_resident(a.load_resident(log.encode(), chunk_bytes=2048))["events"] > 0
    assert a.frequency_statistics() == before
    sa = [(e["lineNumber"], e["score"]) for e in a.parse(log)["events"]]
    sb = [(e["lineNumber"], e["score"]) for e in b.parse(log)["events"]]
    assert sa == sb and len(sa) > 0


def test_batcher_guard():
    lp = LogParser(_boom_library(), config=Config.load(overrides=CPU))
    try:
        acc = lp.leadup_accumulator(2)
        acc.add_document("INFO fine\nBOOM\n")
        assert acc.report(min_count=1)["leadLines"] == 1 == lp.leadup_stream(b"INFO x\nBOOM\n")["leadLines"]
        res = lp.load_resident(b"INFO x\nBOOM\n")
        lp.submit("BOOM\n").result(timeout=120)
        for call in (lambda: lp.leadup(b"x\nBOOM\n"), lambda: lp.leadup_stream(b"x\nBOOM\n"), lambda: lp.leadup_resident(res),
                     lambda: lp.leadup_file(__file__), lambda: lp.leadup_accumulator(), lambda: acc.add_document("x\n"),
                     lambda: acc.add_stream(b"x\n"), lambda: acc.add_resident(res), lambda: acc.report()):
            with pytest.raises(RuntimeError, match="leadup"):
                call()
    finally:
        lp.close()


# ---- 6. command line

def _cli(*argv, code: int = 0):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "leadup", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == code, r.stderr
    return json.loads(r.stdout) if code == 0 else r.stderr


def test_cli(tmp_path):
    log = tmp_path / "app.log"
    log.write_text("starting\nWARN pool exhausted, waiting 20ms\nINFO request 7 served in 9ms\nERROR OOMKilled container app\n"
                   "INFO request 8 served in 11ms\nWARN pool exhausted, waiting 31ms\nINFO request 9 served in 11ms\n"
                   "ERROR OOMKilled container db\nINFO request 10 served in 7ms\n")
    one = _cli(str(log), "--window", "2")
    assert set(one) == KEYS and one["totalLines"] == 9 and one["eventLines"] == 2 and one["leadLines"] == 4
    assert one["window"] == 2 and one["templates"] == 2 and len(one["top"]) == 2
    assert {"count": 2, "total": 2, "share": 1.0, "lift": 2.25, "firstLine": 2,
            "template": "WARN pool exhausted, waiting 0"}.items() <= one["top"][0].items()
    assert {"count": 2, "total": 4, "share": 0.5, "firstLine": 3}.items() <= one["top"][1].items()
    assert _cli(str(log), "--window", "2", "--stream", "--chunk-bytes", "32") == one
    first = _cli(str(log), "--window", "3", "--order", "first", "--min-count", "1", "--top", "5")
    assert [g["firstLine"] for g in first["top"]] == [1, 2, 3] and first["leadLines"] == 6
    assert "window" in _cli(str(log), "--window", "0", code=2)
