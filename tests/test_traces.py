"""Trace report on the CPU engine (log_parser_amd/traces.py, csrc/kernels/traces.hip host twins):
the report against ``golden.traces`` for documents, streams in chunks that traces straddle and
resident logs, the edge cases of the line classes and of runs, the arguments, side effects and the
command line."""
import json
import os
import random
import subprocess
import sys

import pytest

from log_parser_amd import golden
from log_parser_amd import traces as TR
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.native import N
from log_parser_amd.ops import kernels as K
from log_parser_amd.pieces import stream_pieces
from log_parser_amd.utils.config import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
KEYS = {"totalLines", "events", "traces", "traceLines", "frameLines", "groups", "unexplainedTraces",
        "unexplainedGroups", "top"}
GROUP_KEYS = {"count", "eventTraces", "firstLine", "signature", "lines", "frames", "causes", "head", "exception",
              "topFrame", "rootCause"}


def _library():
    """An event on heads, one on a frame, and a backreference on the host side path."""
    return [PatternSet.model_validate({"metadata": {"library_id": "traces"}, "patterns": [
        {"id": "oom", "name": "oom", "severity": "CRITICAL",
         "primary_pattern": {"regex": r"OutOfMemoryError", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "pool", "name": "pool", "severity": "HIGH",
         "primary_pattern": {"regex": r"Pool\.grow", "confidence": 0.8}},
        {"id": "dup", "name": "backref", "severity": "LOW",
         "primary_pattern": {"regex": r"(\w+)Dup \1", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


PLAIN = ["INFO request %d served in %dms", "DEBUG cache shard %d hit ratio 0.%d", "WARN slow disk sd%d latency %dms",
         "ERROR fooDup foo after %d retries", ""]


def _site(rng, k: int):
    """Trace site ``k``: (head template, run templates) -- frames, cause chains, ``... n more``."""
    exc = ["java.lang.IllegalStateException", "java.lang.OutOfMemoryError", "com.acme.db.TimeoutException",
           "java.io.IOException"][k % 4]
    run = ["\tat com.acme.S%d.run%d(S%d.java:%%d)" % (k, j, k) for j in range(1 + k % 5)]
    if k % 3 == 0:
        run.append("\tat com.acme.Pool.grow(Pool.java:%d)")
    if k % 2:
        run += ["Caused by: java.net.SocketException: reset %d", "\tat java.net.Socket.read(Socket.java:%d)", "\t... %d more"]
    if k % 4 == 3:
        run += ["  Suppressed: com.acme.CloseFailed%d" % k, "    at com.acme.Closer.close(Closer.java:%d)",
                "Caused by: com.acme.Root%d: no route %%d" % k, "\t... %d common frames omitted"]
    return "%%d ERROR [w-%%d] %s: site %d failed" % (exc, k), run


def _fill(rng, t: str) -> str:
    return t % tuple(rng.randrange(1000) for _ in range(t.count("%d")))


def _log(n_plain: int, n_traces: int, seed: int, eol: str = "\n", long_run: int = 0) -> str:
    """Plain lines with ``n_traces`` traces of a dozen sites planted among them (some back to
    back: the line between them is the second one's head); ``long_run``: one trace of that many
    frames more."""
    rng = random.Random(seed)
    sites = [_site(rng, k) for k in range(12)]
    blocks = [[_fill(rng, rng.choice(PLAIN))] for _ in range(n_plain)]
    for _ in range(n_traces):
        head, run = rng.choice(sites)
        blocks.insert(rng.randrange(len(blocks) + 1), [_fill(rng, head)] + [_fill(rng, x) for x in run])
    if long_run:
        blocks.insert(len(blocks) // 2, ["java.lang.StackOverflowError"] +
                      ["\tat com.acme.Rec.down(Rec.java:%d)" % (j % 7) for j in range(long_run)])
    lines = [x for b in blocks for x in b] + ["INFO done"]
    return eol.join(lines) + eol


@pytest.fixture(scope="module")
def parser():
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    assert lp.library.summary()["host_fallback"] == 1
    return lp


@pytest.fixture(scope="module")
def case(parser):
    """(log with a 320-frame trace, golden report with every group)."""
    log = _log(600, 90, seed=2, long_run=320)
    want = golden.traces(log, _library(), parser.config.scoring, None)
    assert want["traces"] == 91 and 8 <= want["groups"] <= 13 and want["events"] > 0
    assert 0 < want["unexplainedGroups"] < want["groups"] and 0 < want["unexplainedTraces"] < want["traces"]
    assert max(g["lines"] for g in want["top"]) == 321 and any(g["causes"] == 3 for g in want["top"])
    assert any(g["rootCause"] and g["rootCause"].startswith("Caused by: com.acme.Root") for g in want["top"])
    return log, want


def test_constants_match_the_native_side():
    assert K.TR_TILE == N.trace_tile() and K.TR_TILE % 256 == 0
    assert (K.TR_OTHER, K.TR_FRAME, K.TR_MORE, K.TR_CAUSE) == (golden.TR_OTHER, golden.TR_FRAME, golden.TR_MORE,
                                                               golden.TR_CAUSE)


# ---- 1. the report against golden.traces

@pytest.mark.parametrize("order", ["count", "first"])
@pytest.mark.parametrize("unexplained_only", [False, True])
def test_report_equals_golden(parser, case, order, unexplained_only):
    log, full = case
    for top in (0, 3, None):
        want = golden.traces(log, _library(), parser.config.scoring, top, order, unexplained_only)
        got = parser.traces(log, top=top, order=order, unexplained_only=unexplained_only)
        assert got == want and set(got) == KEYS
        assert all(set(g) == GROUP_KEYS for g in got["top"])
        assert {k: v for k, v in got.items() if k != "top"} == {k: v for k, v in full.items() if k != "top"}
    assert len(got["top"]) == (full["unexplainedGroups"] if unexplained_only else full["groups"])
    firsts = [g["firstLine"] for g in got["top"]]
    if order == "first":
        assert firsts == sorted(firsts)
    else:
        assert [(-g["count"], g["firstLine"]) for g in got["top"]] == sorted((-g["count"], g["firstLine"]) for g in got["top"])
    if unexplained_only:
        assert all(g["eventTraces"] == 0 for g in got["top"])
    assert sum(g["count"] for g in parser.traces(log, top=None)["top"]) == full["traces"]


def test_bad_order_raises(parser, case):
    log, _ = case
    with pytest.raises(ValueError):
        golden.traces(log, _library(), parser.config.scoring, order="line")
    for call in (lambda: parser.traces(log, order="line"),
                 lambda: parser.traces_stream(log.encode(), order="line"),
                 lambda: parser.traces_resident(parser.load_resident(log.encode()), order=""),
                 lambda: TR.TraceAccumulator(parser.engine).report(order="Count")):
        with pytest.raises(ValueError):
            call()


# ---- 2. sources and chunking

@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_stream_equals_document(parser, eol):
    """Chunks so small that traces straddle them -- the 320-line trace covers several whole chunks
    of 4096 bytes -- and chunks of 65536 bytes."""
    log = _log(300, 60, seed=5, eol=eol, long_run=320)
    data = log.encode()
    want = golden.traces(log, _library(), parser.config.scoring, None)
    assert parser.traces(data, top=None) == want and want["traces"] == 61
    for c in (256, 4096, 65536):
        with stream_pieces(parser.engine, data, c) as pieces:
            n = sum(1 for _ in pieces)
        assert n > 1 or c == 65536
        for order in ("count", "first"):
            assert parser.traces_stream(data, chunk_bytes=c, top=None, order=order) == \
                parser.traces(data, top=None, order=order), (c, order)
        assert parser.traces_stream(data, chunk_bytes=c, top=2, unexplained_only=True) == \
            golden.traces(log, _library(), parser.config.scoring, 2, "count", True), c


def test_one_line_chunks(parser):
    """Every line a chunk of its own: every trace straddles chunks, every head is the previous
    chunk's last line."""
    W = 96
    rng = random.Random(9)
    lines = []
    for k in range(8):
        head, run = _site(rng, k)
        lines += [_fill(rng, "INFO request %d served in %dms"), _fill(rng, head)] + [_fill(rng, x) for x in run]
    data = "".join(x.ljust(W - 1) + "\n" for x in ["\tat com.acme.Pool.grow(Pool.java:1)"] + lines).encode()
    assert max(len(x) for x in lines) < W
    want = golden.traces(data, _library(), parser.config.scoring, None)
    assert want["traces"] == 9 and any(g["head"] is None for g in want["top"])
    for c in (W, 2 * W, 3 * W, 5 * W):
        assert parser.traces_stream(data, chunk_bytes=c, top=None) == want, c


def test_resident_and_path_equal_document(parser, case, tmp_path):
    log, want = case
    data = log.encode()
    res = parser.load_resident(data, chunk_bytes=2048)
    assert len(res.chunks) > 3
    assert parser.traces_resident(res, top=None) == want
    assert parser.traces_resident(res, top=3, order="first") == parser.traces(data, top=3, order="first")
    f = tmp_path / "app.log"
    f.write_bytes(data)
    assert parser.traces_stream(str(f), chunk_bytes=300, top=None) == want
    assert parser.traces_file(str(f), top=None) == want


def test_accumulator_continues_line_numbers(parser, case):
    """A further source continues the log's line numbers (cut between traces: a source ends its open run)."""
    log, want = case
    lines = log.split("\n")[:-1]
    cuts = [i for i, x in enumerate(lines) if x.startswith("INFO") and lines[i - 1].startswith("INFO")]
    a, b = cuts[len(cuts) // 3], cuts[2 * len(cuts) // 3]
    parts = ["\n".join(x) + "\n" for x in (lines[:a], lines[a:b], lines[b:])]
    acc = TR.TraceAccumulator(parser.engine)
    acc.add_document(parts[0])
    acc.add_stream(parts[1].encode(), chunk_bytes=512)
    acc.add_resident(parser.load_resident(parts[2].encode(), chunk_bytes=1024))
    assert acc.report(top=None) == want


# ---- 3. edge cases, each against golden

def _check(parser, data: bytes, **expect):
    want = golden.traces(data, _library(), parser.config.scoring, None)
    assert parser.traces(data, top=None) == want, data
    for c in (1, 16, 64):
        assert parser.traces_stream(data, chunk_bytes=c, top=None) == want, (data, c)
    for k, v in expect.items():
        assert want[k] == v, (k, want)
    return want


F1, F2 = b"\tat com.acme.A.f(A.java:10)", b"\tat com.acme.B.g(B.java:20)"


def test_headless_trace_at_line_0(parser):
    w = _check(parser, F1 + b"\n" + F2 + b"\nINFO after\n", traces=1, traceLines=2, frameLines=2)
    assert w["top"][0]["head"] is None and w["top"][0]["firstLine"] == 1 and w["top"][0]["exception"] is None


def test_trace_ends_the_document_without_newline(parser):
    w = _check(parser, b"java.lang.RuntimeException: x\n" + F1 + b"\n" + F2, traces=1, traceLines=3)
    assert w["top"][0]["exception"] == "java.lang.RuntimeException" and w["top"][0]["firstLine"] == 1


def test_two_traces_one_line_apart(parser):
    w = _check(parser, b"first.BadError: 1\n" + F1 + b"\nsecond.WorseException\n" + F2 + b"\n", traces=2, traceLines=4, groups=2)
    assert [g["firstLine"] for g in w["top"]] == [1, 3] and w["top"][1]["head"] == "second.WorseException"


def test_runs_without_a_frame_are_no_traces(parser):
    _check(parser, b"x\nCaused by: a.B: c\n\t... 3 more\ny\n\t... 4 more\nSuppressed: q\nz\n", traces=0, groups=0, traceLines=0)


def test_leading_blanks_64_and_65(parser):
    data = b"h\n" + b" " * 64 + b"at a.B.c(B.java:1)\nh\n" + b" " * 65 + b"at a.B.c(B.java:1)\nh\n" + \
        b"\t" * 64 + b"... 2 more\n" + b"\t" * 65 + b"at x\n" + b" " * 64 + b"Caused by: q.R\n" + b" " * 65 + b"Caused by: q.R\n"
    _check(parser, data, traces=1, frameLines=1, traceLines=2)
    assert [golden.trace_class(x)[0] for x in data.split(b"\n")[:-1]] == [0, 1, 0, 0, 0, 2, 0, 3, 0]


def test_line_that_is_exactly_tab_at(parser):
    _check(parser, b"head\n\tat\n", traces=0)
    _check(parser, b"head\n\tat\n" + F1, traces=1, traceLines=2, frameLines=1)        # (... so the frame's head is "\tat")
    _check(parser, b"head\n\tat \n", traces=1)


def test_crlf_line_ends(parser):
    w = _check(parser, b"a.b.CrashError: boom\r\n" + F1 + b"\r\nCaused by: x.Y: z\r\n" + F2 + b"\r\n\t... 1 more\r\nend\r\n",
               traces=1, traceLines=5, frameLines=2, totalLines=6)
    assert w["top"][0]["rootCause"] == "Caused by: x.Y: z" and w["top"][0]["causes"] == 1


def test_cause_tokens_of_0_256_and_257_bytes(parser):
    def doc(token: bytes) -> bytes:
        return b"head\n" + F1 + b"\nCaused by: " + token + b"\n" + F2 + b"\n"
    sig = {n: _check(parser, doc(b"T" * n), traces=1)["top"][0]["signature"] for n in (0, 255, 256, 257, 300)}
    assert sig[256] == sig[257] == sig[300] and len({sig[0], sig[255], sig[256]}) == 3      # cut after 256 bytes
    assert _check(parser, b"head\n" + F1 + b"\nCaused by:\n" + F2 + b"\n")["top"][0]["signature"] == sig[0]
    # the token ends at a colon or a blank, and at most 8 blanks before it are skipped
    a = _check(parser, doc(b"x.Y: one"))["top"][0]["signature"]
    assert a == _check(parser, doc(b"       x.Y two"))["top"][0]["signature"]
    assert a != _check(parser, doc(b"        x.Y"))["top"][0]["signature"] == sig[0]        # (the 9th blank: an empty token)


def test_same_frames_other_line_numbers_are_one_group(parser):
    one = b"e.E: 1\n\tat a.B.c(B.java:10)\n\tat a.D.e(D.java:200)\n"
    two = b"f.F: 2\n\tat a.B.c(B.java:11)\n\tat  a.D.e(D.java:7)\n"
    other = b"g.G: 3\n\tat a.D.e(D.java:200)\n\tat a.B.c(B.java:10)\n"                      # the same frames, another order
    w = _check(parser, one + b"INFO x\n" + two + b"INFO y\n" + other, traces=3, groups=2)
    assert w["top"][0]["count"] == 2 and w["top"][0]["head"] == "e.E: 1" and w["top"][0]["firstLine"] == 1


def test_event_on_the_head_only_and_on_a_frame_only(parser):
    head = _check(parser, b"java.lang.OutOfMemoryError: heap\n" + F1 + b"\n", events=1, traces=1, unexplainedTraces=0)
    assert head["top"][0]["eventTraces"] == 1
    frame = _check(parser, b"quiet head\n" + F1 + b"\n\tat com.acme.Pool.grow(Pool.java:12)\n", events=1, unexplainedTraces=0)
    assert frame["top"][0]["eventTraces"] == 1 and frame["unexplainedGroups"] == 0
    # an event two lines before the run, or right after it, explains nothing
    _check(parser, b"java.lang.OutOfMemoryError: heap\nhead\n" + F1 + b"\nPool.grow again\n", events=2, unexplainedTraces=1)


def test_empty_logs(parser):
    zero = {"events": 0, "traces": 0, "traceLines": 0, "frameLines": 0, "groups": 0, "unexplainedTraces": 0,
            "unexplainedGroups": 0, "top": []}
    for call in (parser.traces, parser.traces_stream, lambda d: parser.traces_stream(d, chunk_bytes=2)):
        assert call(b"") == {"totalLines": 1, **zero} == golden.traces("", _library(), parser.config.scoring)
        assert call(b"\n") == {"totalLines": 0, **zero} == golden.traces("\n", _library(), parser.config.scoring)


# ---- 4. side effects, guard, command line

def test_frequency_window_untouched(case):
    log, _ = case
    cfg = Config.load(overrides={"engine.device": "cpu", "scoring.frequency.threshold": "1.0"})
    a = LogParser(_library(), config=cfg)
    a.parse(log)
    before = a.frequency_statistics()
    assert before and a.traces(log)["events"] > 0
    assert a.traces_stream(log.encode(), chunk_bytes=300)["events"] > 0
    assert a.traces_resident(a.load_resident(log.encode(), chunk_bytes=2048))["events"] > 0
    assert a.frequency_statistics() == before


def test_batcher_guard():
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    try:
        res = lp.load_resident(b"x\n" + F1 + b"\n")
        assert lp.traces_resident(res)["traces"] == 1
        lp.submit("ERROR x\n").result(timeout=120)
        for call in (lambda: lp.traces(b"x\n"), lambda: lp.traces_stream(b"x\n"), lambda: lp.traces_resident(res),
                     lambda: lp.traces_file(__file__)):
            with pytest.raises(RuntimeError, match="traces"):
                call()
    finally:
        lp.close()


def _cli(*argv):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "traces", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_cli(tmp_path):
    log = tmp_path / "app.log"
    log.write_text("starting\njava.lang.IllegalStateException: pool 1 closed\n\tat com.acme.Pool.grow(Pool.java:12)\n"
                   "\tat com.acme.Main.run(Main.java:3)\nCaused by: java.io.IOException: disk\n\t... 2 more\nINFO ok\n"
                   "other.KindError\n\tat com.acme.Other.go(Other.java:1)\n"
                   "java.lang.IllegalStateException: pool 2 closed\n\tat com.acme.Pool.grow(Pool.java:13)\n"
                   "\tat com.acme.Main.run(Main.java:4)\nCaused by: java.io.IOException: net\n\t... 9 more\n")
    one = _cli(str(log), "--top", "5")
    assert set(one) == KEYS and one["totalLines"] == 14 and one["traces"] == 3 and one["groups"] == 2
    assert one["traceLines"] == 12 and one["frameLines"] == 5
    assert {"count": 2, "firstLine": 2, "lines": 5, "frames": 2, "causes": 1, "exception": "java.lang.IllegalStateException",
            "topFrame": "at com.acme.Pool.grow(Pool.java:12)",
            "rootCause": "Caused by: java.io.IOException: disk"}.items() <= one["top"][0].items()
    assert _cli(str(log), "--top", "5", "--stream", "--chunk-bytes", "32") == one
    first = _cli(str(log), "--order", "first", "--unexplained-only", "--top", "1")
    assert [g["firstLine"] for g in first["top"]] == [2] and first["groups"] == 2
