"""Log timeline on the CPU engine: the timestamp grammar (golden.line_timestamp, the host twin of
k_ts_parse), the report against golden.timeline, edge documents, the stream and resident forms
against the one-piece report, side effects and the command line."""
import json
import os
import random
import subprocess
import sys
import threading

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.parallel.stream import StreamAnalyzer, _eff_end
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import make_library, make_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
CPU = {"engine.device": "cpu"}

B = 1758283200000                       # 2025-09-19T12:00:00Z
S = b"2025-09-19T12:00:00"
LEAP = (19723 + 31 + 28) * 86400000     # 2024-01-01 is day 19723; 2024-02-29

# (line, epoch milliseconds or None), worked out by hand
GRAMMAR = [
    (S + b".000Z", B),
    (S, B),
    (b"2024-02-29T00:00:00Z", LEAP),
    (b"2023-02-29T00:00:00Z", None),
    (b"2100-02-29T00:00:00Z", None),                         # 2100 is no leap year
    (b"2000-02-29T00:00:00Z", 951782400000),                 # 2000 is one
    (b"2025-13-19T12:00:00", None),
    (b"2025-00-19T12:00:00", None),
    (b"2025-09-31T12:00:00", None),
    (b"2025-09-00T12:00:00", None),
    (b"2025-09-19T24:00:00", None),
    (b"2025-09-19T12:60:00", None),
    (b"2025-09-19T12:00:60", None),
    (b"1969-12-31T23:59:59Z", None),
    (b"1970-01-01T00:00:00+01:00", -3600000),
    (b"1970-01-01T00:00:00Z", 0),
    (S + b".1", B + 100),
    (S + b".123", B + 123),
    (S + b".123456789", B + 123),
    (S + b".1234567891Z", B + 123),
    (S + b".1234567891+02:00", B + 123),                     # the zone behind a tenth digit is not seen
    (S + b".123456789+02:00", B + 123 - 7200000),
    (S + b",123", B + 123),
    (S + b",999 INFO logback", B + 999),
    (S + b". next", B),                                      # a mark without a digit is no fraction
    (b"2025/09/19 12:00:00", B),
    (b"2025/09/19 12:00:00 [error] 7#7: nginx", B),
    (b"2025-09/19 12:00:00", B),                             # the grammar does not pair the separators
    (S + b"+0530", B - 19800000),
    (S + b"-01:30", B + 5400000),
    (S + b"+24:00", None),
    (S + b"+23:60", None),
    (S + b"+05:3", B),                                       # no whole zone: UTC
    (S + b"+05", B),
    (S + b" +05:30", B),                                     # the zone must follow immediately
    (S + b".5-0800 stdout F hello", B + 500 + 28800000),
    (b"x" + S, None),
    (b"9" + S, None),
    (b"[" + S + b"] boot", B),
    (b'"' + S + b'Z"', B),
    (b'time="' + S + b'Z" level=info', B),
    (b'{"ts":"' + S + b'.25Z","msg":"x"}', B + 250),
    (S[:18], None),                                          # the line ends inside the stamp
    (S[:10], None),
    (b"", None),
    (b"2025-13-19T12:00:00 " + S, None),                     # an invalid leftmost match: later ones are not tried
    (b"2025-09 " + S, B),                                    # no match at all at offset 0: the next start is
    (b"2025-2025-09-19T12:00:00", B),
    (b"E0919 12:00:00.000000 1 klog.go:1] x", None),
    (b"Sep 19 12:00:00 host app[1]: x", None),
    (b"19/Sep/2025:12:00:00 +0000", None),
    (b"1758283200 epoch", None),
]
GRAMMAR += [(b"." * k + S + b"Z", B) for k in range(32)]
GRAMMAR += [(b"." * 32 + S + b"Z", None), (b"\xc3\xa9" * 15 + b" " + S, B), (b"\xc3\xa9" * 16 + S, None)]


def _index(lines):
    """(text, ls, ll) of the lines joined with "\\n" (CPU tensors)."""
    data = b"\n".join(lines) + b"\n"
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    ls, o = [], 0
    for l in lines:
        ls.append(o)
        o += len(l) + 1
    return text, torch.tensor(ls, dtype=torch.int64), torch.tensor([len(l) for l in lines], dtype=torch.int32)


def _twin(lines):
    return [None if t == K.TS_NONE else t for t in K.line_timestamps(*_index(lines)).tolist()]


def test_grammar_table():
    for line, want in GRAMMAR:
        assert golden.line_timestamp(line) == want, line
    assert _twin([l for l, _ in GRAMMAR]) == [w for _, w in GRAMMAR]
    assert golden.iso_ms(B + 7) == "2025-09-19T12:00:00.007Z" and golden.iso_ms(-1) == "1969-12-31T23:59:59.999Z"


def _random_stamp(rng):
    out = "%04d%s%02d%s%02d%s%02d:%02d:%02d" % (
        rng.choice([1969, 1970, 1999, 2000, 2023, 2024, 2025, 2100, 9999]), rng.choice("-/"), rng.randrange(0, 14),
        rng.choice("-/"), rng.randrange(0, 33), rng.choice("T "), rng.randrange(0, 26), rng.randrange(0, 62),
        rng.randrange(0, 62))
    if rng.random() < .6:
        out += rng.choice(".,") + "".join(rng.choice("0123456789") for _ in range(rng.randrange(0, 12)))
    r = rng.random()
    if r < .3:
        out += "Z"
    elif r < .7:
        out += "%s%02d%s%02d" % (rng.choice("+-"), rng.randrange(0, 26), rng.choice([":", ""]), rng.randrange(0, 62))
    return out


def test_twin_fuzz():
    rng = random.Random(1)
    alpha = "0123456789-/:T .,Z+-xA[\"= \xe9"
    lines = []
    for _ in range(6000):
        pre = "".join(rng.choice(alpha) for _ in range(rng.randrange(0, 36)))
        if rng.random() < .5:
            pre = rng.choice(["", "[", "\"", "time=\"", "{\"ts\":\"", "x", " "])
        s = list(pre + _random_stamp(rng) + rng.choice(["", " INFO foo", "Z", "+01:00 x", _random_stamp(rng)]))
        for _ in range(rng.choice([0, 0, 1, 2, 3])):
            k, r = rng.randrange(len(s) + 1), rng.random()
            if r < .33 and k < len(s):
                s[k] = rng.choice(alpha)
            elif r < .66 and k < len(s):
                del s[k]
            else:
                s.insert(k, rng.choice(alpha))
        if rng.random() < .1:
            s = s[:rng.randrange(len(s) + 1)]
        lines.append("".join(s).encode("utf-8"))
    want = [golden.line_timestamp(l) for l in lines]
    assert 500 < sum(w is not None for w in want) < 5500            # both outcomes are well represented
    assert _twin(lines) == want


def _fill_reference(ts, carry_last, carry_top):
    eff, n, last, top = [], 0, carry_last, carry_top
    for t in ts:
        if t != K.TS_NONE:
            n += t < top
            last, top = t, max(top, t)
        eff.append(last)
    return eff, n


def _fill_cases():
    """(stamps, carry_last, carry_top) around the tile edges of k_tl_fill (8 lines a lane, 2048 a
    block)."""
    rng = random.Random(5)
    NONE = K.TS_NONE
    for L in (1, 7, 8, 9, 2047, 2048, 2049, 4097):
        for ts in ([NONE] * L,                                                    # nothing stamped
                   [B + rng.randrange(-500, 500) * 1000 if rng.random() < .7 else NONE for _ in range(L)],
                   [B - i if i % 97 == 0 else NONE for i in range(L)]):           # sparse, every stamp runs backwards
            yield ts, NONE, NONE
            yield ts, B - 77, B + 100000


def test_fill_twin():
    for ts, carry_last, carry_top in _fill_cases():
        eff, n = K.timeline_fill(torch.tensor(ts, dtype=torch.int64), carry_last, carry_top)
        want = _fill_reference(ts, carry_last, carry_top)
        assert (eff.tolist(), n.item()) == want, (len(ts), carry_last)
    eff, n = K.timeline_fill(torch.empty(0, dtype=torch.int64))
    assert eff.numel() == 0 and n.item() == 0


# ---- the report against golden.timeline

@pytest.fixture(scope="module")
def synth():
    sets, trig = make_library(64, seed=1)
    log = "no stamp yet\n\tat x.Y(Z.java:1)\n" + make_log(20000, trig, seed=3, stack_rate=0.05, crlf_rate=0.1)
    return sets, log, LogParser(sets, config=Config.load(overrides=CPU))


@pytest.mark.parametrize("bucket", [1, 60, 3600])
def test_report_equals_golden(synth, bucket):
    sets, log, lp = synth
    want = golden.timeline(log, sets, lp.config.scoring, bucket)
    assert 0 < want["stampedLines"] < want["totalLines"] == 20002
    assert want["outOfOrderLines"] > 0 and want["undatedLines"] > 0 and want["events"] > 0
    assert len({k for b in want["buckets"] for k in b["severity"]}) >= 2
    assert sum(b["lines"] for b in want["buckets"]) == want["totalLines"] - want["undatedLines"]
    assert lp.engine.timeline_bytes(log.encode(), bucket) == want
    assert lp.timeline(log, bucket_seconds=bucket) == want
    assert lp.timeline_stream(log.encode(), chunk_bytes=1 << 16, bucket_seconds=bucket) == want


# ---- a small library and a planted log for everything else

def _library():
    return [PatternSet.model_validate({"metadata": {"library_id": "tl"}, "patterns": [
        {"id": "oom", "name": "oom", "severity": "CRITICAL",
         "primary_pattern": {"regex": r"OutOfMemoryError", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "quota", "name": "quota", "severity": "high",
         "primary_pattern": {"regex": r"disk quota exceeded", "confidence": 0.8}},
        {"id": "heap", "name": "heap", "primary_pattern": {"regex": r"heap space", "confidence": 0.5}},
        {"id": "dup", "name": "backref", "severity": "LOW",
         "primary_pattern": {"regex": r"(\w+)Dup \1", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


def _planted_log() -> str:
    """Undated leading lines with an event and an error line among them, events of four severities
    (one null), two events on one line, continuation lines behind stamped lines, a stamp that
    jumps back, a zone, a stamp before 1970 UTC (a negative bucket is not reached: year >= 1970
    holds for the local date), the last line unstamped."""
    return "\n".join([
        "starting up", "ERROR fooDup foo before any stamp", "java.lang.OutOfMemoryError: early",
        "2025-09-19T12:00:00.100Z INFO boot ok",
        "2025-09-19T12:00:01Z ERROR widget 1 jammed",
        "java.lang.OutOfMemoryError: Java heap space", "\tat x.Y(Z.java:1)", "\tat x.Y(Z.java:2)",
        "2025-09-19T12:00:59,999 WARN slow disk",
        "[2025-09-19 12:01:00] ERROR disk quota exceeded on /data",
        "2025-09-19T12:05:30+02:00 INFO a stamp two hours back",
        "continuation of the line two hours back", "FATAL shard 3 lost",
        "2025-09-19T12:05:31Z ERROR barDup bar happened",
        "2025/09/19 12:07:00 ERROR widget 2 jammed",
        "2025-09-19T12:07:00.5Z INFO same bucket",
        "2025-13-19T12:07:01Z ERROR an invalid month takes the time above",
        "java.lang.OutOfMemoryError: late", "the end"]) + "\n"


@pytest.fixture(scope="module")
def parser():
    lp = LogParser(_library(), config=Config.load(overrides=CPU))
    assert lp.library.summary()["host_fallback"] == 1         # the backreference: host side path
    return lp


def _golden(lp, data, bucket_seconds=60, max_buckets=65536):
    return golden.timeline(data, _library(), lp.config.scoring, bucket_seconds, max_buckets)


def test_planted_report(parser):
    log = _planted_log()
    rep = parser.timeline(log)
    assert rep == _golden(parser, log)
    assert (rep["totalLines"], rep["stampedLines"], rep["undatedLines"], rep["outOfOrderLines"]) == (19, 8, 3, 1)
    assert (rep["events"], rep["undatedEvents"]) == (7, 2)
    assert rep["firstTimestamp"] == "2025-09-19T10:05:30.000Z" and rep["lastTimestamp"] == "2025-09-19T12:07:00.500Z"
    assert rep["firstErrorLine"] == {"lineNumber": 5, "timestamp": "2025-09-19T12:00:01.000Z"}
    assert rep["firstEvent"] == {"lineNumber": 6, "patternId": "oom", "timestamp": "2025-09-19T12:00:01.000Z"}
    assert rep["lastEvent"] == {"lineNumber": 18, "patternId": "oom", "timestamp": "2025-09-19T12:07:00.500Z"}
    assert rep["buckets"][0] == {"start": "2025-09-19T10:05:00.000Z", "lines": 3, "errorLines": 1, "events": 0,
                                 "severity": {}}
    assert rep["buckets"][1] == {"start": "2025-09-19T12:00:00.000Z", "lines": 6, "errorLines": 2, "events": 2,
                                 "severity": {"CRITICAL": 1, "": 1}}
    assert [b["start"][11:16] for b in rep["buckets"]] == ["10:05", "12:00", "12:01", "12:05", "12:07"]
    for bucket in (1, 7, 3600, 86400):
        assert parser.timeline(log, bucket_seconds=bucket) == _golden(parser, log, bucket)


def test_edge_documents(parser):
    none = {"firstTimestamp": None, "lastTimestamp": None, "firstErrorLine": None, "firstEvent": None,
            "lastEvent": None, "buckets": []}
    for doc in ("", "\n", "ERROR no stamp\njava.lang.OutOfMemoryError: x\nplain\n", "ERROR one line, no stamp"):
        rep = parser.timeline(doc)
        assert rep == _golden(parser, doc) and none.items() <= rep.items()
        assert rep["undatedLines"] == rep["totalLines"] and rep["undatedEvents"] == rep["events"]
    assert parser.timeline("ERROR no stamp\njava.lang.OutOfMemoryError: x\nplain\n")["events"] == 1
    one = "2025-09-19T12:00:00Z java.lang.OutOfMemoryError: Java heap space"
    rep = parser.timeline(one)
    assert rep == _golden(parser, one) and rep["events"] == 2
    assert rep["buckets"] == [{"start": "2025-09-19T12:00:00.000Z", "lines": 1, "errorLines": 1, "events": 2,
                               "severity": {"CRITICAL": 1, "": 1}}]
    assert (rep["firstEvent"]["patternId"], rep["lastEvent"]["patternId"]) == ("oom", "heap")
    same = "".join("2025-09-19T12:00:%02dZ ERROR widget %d jammed\n" % (i % 60, i) for i in range(300))
    rep = parser.timeline(same)
    assert rep == _golden(parser, same) and len(rep["buckets"]) == 1 and rep["buckets"][0]["errorLines"] == 300
    early = "1970-01-01T00:30:00+01:00 ERROR before the epoch\n1970-01-01T00:00:00Z INFO at it\n"
    rep = parser.timeline(early)
    assert rep == _golden(parser, early) and rep["buckets"][0]["start"] == "1969-12-31T23:30:00.000Z"
    for bad in (0, -5, 1.5, True, "60"):
        with pytest.raises(ValueError):
            parser.timeline(one, bucket_seconds=bad)
        with pytest.raises(ValueError):
            _golden(parser, one, bad)


def test_span_over_max_buckets(parser):
    doc = ("2025-09-19T12:00:00Z INFO a\n" + "INFO filler\n" * 40 + "1999-01-01T00:00:00Z ERROR a stray old date\n"
           + "INFO filler\n" * 40 + "2025-09-19T12:00:01Z INFO b\n")
    for call in (lambda **kw: _golden(parser, doc, **kw), lambda **kw: parser.timeline(doc, **kw),
                 lambda **kw: parser.timeline_stream(doc.encode(), **kw),
                 lambda **kw: parser.timeline_stream(doc.encode(), chunk_bytes=64, **kw)):
        with pytest.raises(ValueError, match="larger bucket"):
            call()
        assert len(call(bucket_seconds=86400)["buckets"]) == 2
        with pytest.raises(ValueError):
            call(bucket_seconds=86400, max_buckets=9758)              # days 10592 .. 20350: 9759 buckets
        assert call(bucket_seconds=86400, max_buckets=9759)["outOfOrderLines"] == 1


def test_span_error_from_a_path_in_many_chunks(parser, tmp_path):
    """The error leaves in the middle of a mapped file with more chunks waiting than the producer's
    queue holds: it still comes out as the ValueError (the mapping can be closed), no producer
    thread stays behind, and the command line turns it into its message and exit status 2."""
    doc = ("2025-09-19T12:00:00Z INFO a\n" + "INFO filler\n" * 40 + "1999-01-01T00:00:00Z ERROR a stray old date\n"
           + "INFO filler\n" * 400 + "2025-09-19T12:00:01Z INFO b\n")
    f = tmp_path / "stray.log"
    f.write_text(doc)
    threads = threading.active_count()
    for c in (64, 300, None):
        with pytest.raises(ValueError, match="larger bucket"):
            parser.timeline_stream(str(f), chunk_bytes=c)
        with pytest.raises(ValueError, match="larger bucket"):
            parser.timeline_stream(doc.encode(), chunk_bytes=c)
    assert threading.active_count() == threads
    assert parser.timeline_stream(str(f), chunk_bytes=64, bucket_seconds=86400) == parser.timeline(doc, 86400)
    cmd = [sys.executable, "-m", "log_parser_amd", "timeline", str(f), "--stream", "--patterns", PAT, "--device", "cpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT,
                       timeout=300)
    assert r.returncode == 2 and "larger bucket" in r.stderr and "Traceback" not in r.stderr and r.stdout == ""


def test_line_index_tensors_are_checked():
    text, ls, ll = _index([S + b"Z", b"x"])
    assert K.line_timestamps(text, ls, ll).tolist() == [B, K.TS_NONE]
    for bad in ((text, ls.int(), ll), (text, ls, ll.long()), (text, ls, ll[:1]), (text, ls.repeat(2)[::2], ll),
                (text.long(), ls, ll)):
        with pytest.raises(ValueError):
            K.line_timestamps(*bad)


# ---- stream and resident forms

def test_stream_equals_document(parser):
    data = _planted_log().encode()
    for bucket in (60, 1):
        want = parser.timeline(data, bucket_seconds=bucket)
        for c in (1, 2, 64, 300, 4096, 1 << 20):
            assert parser.timeline_stream(data, chunk_bytes=c, bucket_seconds=bucket) == want, (c, bucket)


W = 64              # bytes per line, line end included: 10 lines fill a 640-byte chunk exactly


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_border_cases(parser, eol):
    """Chunks of 10 * W bytes begin at the lines 0, 10, 20, 30.
    boundary 10: line 9 is stamped, the lines 10..12 are its continuation (the fill carry);
    boundary 20: line 19 holds the running maximum, line 20 is stamped below it (the other carry),
    and line 21 is stamped below line 19 but above line 20 (line 29 is below line 19 as well);
    boundary 30: an event on the unstamped line 30 takes the time of line 29."""
    lines = ["INFO filler %d" % i for i in range(40)]
    lines[3] = "2025-09-19T12:00:00Z INFO first"
    lines[9] = "2025-09-19T12:03:00Z ERROR widget 9 jammed"
    lines[10] = "java.lang.OutOfMemoryError: Java heap space"
    lines[19] = "2025-09-19T12:30:00Z ERROR the running maximum"
    lines[20] = "2025-09-19T12:10:00Z INFO back"
    lines[21] = "2025-09-19T12:20:00Z INFO still behind line 19"
    lines[29] = "2025-09-19T12:21:00Z INFO before the border"
    lines[30] = "ERROR disk quota exceeded"
    data = "".join(x.ljust(W - len(eol)) + eol for x in lines).encode()
    plan = list(StreamAnalyzer(parser.engine, chunk_bytes=10 * W)._plan(data, _eff_end(data)))
    assert [data[:pos].count(b"\n") for _, pos, _, _, _, _ in plan] == [0, 10, 20, 30]
    want = parser.timeline(data)
    assert want == _golden(parser, data)
    assert (want["undatedLines"], want["outOfOrderLines"], want["events"]) == (3, 3, 3)
    assert want["lastEvent"] == {"lineNumber": 31, "patternId": "quota", "timestamp": "2025-09-19T12:21:00.000Z"}
    for c in (10 * W, 1, W, 3 * W + 1, 25 * W):
        assert parser.timeline_stream(data, chunk_bytes=c) == want, c


def test_resident_equals_stream(parser):
    data = (_planted_log() * 40).encode()
    res = parser.load_resident(data, chunk_bytes=8192)
    assert len(res.chunks) > 3
    for bucket in (60, 5):
        want = parser.timeline(data, bucket_seconds=bucket)
        assert parser.timeline_resident(res, bucket_seconds=bucket) == want
        assert parser.timeline_stream(data, chunk_bytes=8192, bucket_seconds=bucket) == want
    assert want["outOfOrderLines"] > 40


def test_paths_and_empty_sources(parser, tmp_path):
    data = _planted_log().encode()
    f = tmp_path / "app.log"
    f.write_bytes(data)
    assert parser.timeline_stream(str(f), chunk_bytes=300) == parser.timeline_file(str(f)) == parser.timeline(data)
    e = tmp_path / "empty.log"
    e.write_bytes(b"")
    assert parser.timeline_stream(str(e)) == parser.timeline_file(str(e)) == parser.timeline(b"")
    for src in (b"", b"\n", b"INFO all good\nDEBUG nothing 1 to see\n"):
        for c in (None, 2):
            rep = parser.timeline_stream(src, chunk_bytes=c)
            assert rep == parser.timeline(src) == _golden(parser, src)
            assert rep["totalLines"] == (0 if src == b"\n" else len(golden.split_lines(src.decode())))


# ---- side effects and interface

def test_frequency_window_untouched():
    log = _planted_log()
    cfg = Config.load(overrides={**CPU, "scoring.frequency.threshold": "1.0"})
    a, b = LogParser(_library(), config=cfg), LogParser(_library(), config=cfg)
    a.parse(log)
    b.parse(log)
    before = a.frequency_statistics()
    assert before and a.timeline(log)["events"] == 7
    assert a.frequency_statistics() == before
    assert a.timeline_stream(log.encode(), chunk_bytes=300)["events"] == 7
    assert a.frequency_statistics() == before
    sa = [(e["lineNumber"], e["score"]) for e in a.parse(log)["events"]]
    sb = [(e["lineNumber"], e["score"]) for e in b.parse(log)["events"]]
    assert sa == sb and len(sa) == 7


def test_batcher_guard():
    lp = LogParser(_library(), config=Config.load(overrides=CPU))
    try:
        assert lp.timeline(b"ERROR x\n")["totalLines"] == 1
        res = lp.load_resident(b"ERROR x\n")
        lp.submit("ERROR x\n").result(timeout=120)
        for call in (lambda: lp.timeline(b"ERROR x\n"), lambda: lp.timeline_stream(b"ERROR x\n"),
                     lambda: lp.timeline_resident(res)):
            with pytest.raises(RuntimeError, match="timeline"):
                call()
    finally:
        lp.close()


def _cli(*argv):
    cmd = [sys.executable, "-m", "log_parser_amd", "timeline", *argv, "--patterns", PAT, "--device", "cpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_cli(tmp_path):
    f = tmp_path / "a.log"
    f.write_text("starting\n2025-09-19T12:00:00Z boot\n2025-09-19T12:00:07Z ERROR OOMKilled container app\n"
                 "  continued\n2025-09-19T12:01:02Z ERROR widget 17 jammed\n")
    lp = LogParser.from_directory(PAT, config=Config.load(overrides=CPU))
    one = _cli(str(f))
    assert one == lp.timeline_file(str(f)) and one["events"] >= 1 and len(one["buckets"]) == 2
    five = _cli(str(f), "--stream", "--bucket", "5")
    assert five == lp.timeline_stream(str(f), bucket_seconds=5) == lp.timeline_file(str(f), bucket_seconds=5)
    assert [b["start"] for b in five["buckets"]] == ["2025-09-19T12:00:00.000Z", "2025-09-19T12:00:05.000Z",
                                                     "2025-09-19T12:01:00.000Z"]
