"""Coverage-gap report of streams, resident logs and corpora on the CPU engine
(log_parser_amd/gapreport.py): a stream in chunks of any size reports exactly what the one-document
``gaps`` reports, a corpus reports what ``golden.gaps_corpus`` specifies."""
import json
import mmap
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
from log_parser_amd.parallel.stream import StreamAnalyzer, _eff_end
from log_parser_amd.pieces import document_piece, gather_lines, stream_pieces
from log_parser_amd.utils.config import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
KEYS = {"totalLines", "events", "errorLines", "uncoveredErrorLines", "templates", "top"}
ZERO = {"events": 0, "errorLines": 0, "uncoveredErrorLines": 0, "templates": 0, "top": []}


def _library():
    """A window after the match (2 lines), a window before it (1 line), a pattern without context
    rules, and a backreference that runs on the host side path."""
    return [PatternSet.model_validate({"metadata": {"library_id": "gaps"}, "patterns": [
        {"id": "oom", "name": "oom", "severity": "CRITICAL",
         "primary_pattern": {"regex": r"OutOfMemoryError", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "quota", "name": "quota", "severity": "HIGH",
         "primary_pattern": {"regex": r"disk quota exceeded", "confidence": 0.8}},
        {"id": "dup", "name": "backref", "severity": "LOW",
         "primary_pattern": {"regex": r"(\w+)Dup \1", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


def _planted_log() -> str:
    """Uncovered templates with uneven counts between filler lines, an ERROR line inside the oom
    window, an ERROR line before the backreference match (inside its window), one behind the
    null-rules match (not covered), a stack frame (no candidate)."""
    rng = random.Random(9)
    out = ["INFO boot %d ok" % i for i in range(5)]

    def put(line):
        out.append(line)
        out.extend("INFO tick %d WARN-free" % rng.randrange(1000) for _ in range(rng.randrange(1, 4)))

    for k, t in enumerate("AABACBCABCA"):
        if t == "A":
            put("ERROR [worker-%d] connection to 10.0.%d.%d:5432 refused at 2024-01-0%dT10:0%d:00"
                % (rng.randrange(100), rng.randrange(256), rng.randrange(256), 1 + k % 9, k % 10))
        elif t == "B":
            put("FATAL cache shard %d lost quorum" % rng.randrange(64))
        else:
            put("request %08x1 failed: TimeoutException after %dms" % (rng.randrange(1 << 32), rng.randrange(9000)))
    out += ["java.lang.OutOfMemoryError: Java heap space", "\tat x.Y(Z.java:1)", "ERROR cleanup after oom",
            "ERROR cleanup after oom", "WARN slow disk", "ERROR disk quota exceeded on /data",
            "ERROR retry scheduled in 30s", "\tat com.acme.MyException.raise(MyException.java:9)",
            "ERROR before the dup", "ERROR fooDup foo happened", "ERROR cleanup after oom"]
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def parser():
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    assert lp.library.summary()["host_fallback"] == 1         # the backreference: host side path
    return lp


# ---- 1. a stream in chunks == the one-document report

@pytest.mark.parametrize("cover", ["context", "events"])
def test_stream_equals_document(parser, cover):
    data = _planted_log().encode()
    full = parser.gaps(data, top=None, cover=cover)
    assert full == golden.gaps(data, _library(), parser.config.scoring, None, cover)
    assert full["events"] == 3 and full["templates"] >= 5 and full["errorLines"] > full["uncoveredErrorLines"] > 0
    for top in (20, None):
        want = parser.gaps(data, top=top, cover=cover)
        for c in (2, 64, 300, 4096, 1 << 20):
            assert parser.gaps_stream(data, chunk_bytes=c, top=top, cover=cover) == want, (c, top)
    assert parser.gaps_stream(data, chunk_bytes=64, top=1, cover=cover)["top"] == full["top"][:1]
    with pytest.raises(ValueError):
        parser.gaps_stream(data, cover="lines")


# ---- 2. every border case at a chunk boundary

W = 64              # bytes per line, line end included: 10 lines fill a 640-byte chunk exactly


def _border_log(eol: str) -> bytes:
    """60 lines of W bytes. Chunks of 10 * W bytes begin at the lines 0, 10, 20, ...
    boundary 10: the oom match on line 9 covers the candidates on lines 10 and 11 (lines_after 2);
    boundary 20: the dup match on line 20 covers the candidate on line 19 (lines_before 1);
    boundary 30: the candidates on lines 29 and 30 are covered by nothing;
    boundary 40: the candidate on line 38 is out of the dup match's reach on line 40 (held back,
    then released)."""
    lines = ["INFO filler %d" % i for i in range(60)]
    lines[9] = "java.lang.OutOfMemoryError: Java heap space"
    lines[10] = "ERROR widget 10 jammed"
    lines[11] = "ERROR widget 11 jammed"
    lines[12] = "ERROR widget 12 jammed"            # past the window
    lines[19] = "ERROR widget 19 jammed"
    lines[20] = "ERROR barDup bar happened"
    lines[29] = "ERROR widget 29 jammed"
    lines[30] = "FATAL shard 30 lost"
    lines[38] = "FATAL shard 38 lost"
    lines[40] = "ERROR bazDup baz happened"
    lines[59] = "FATAL shard 59 lost"
    return "".join(x.ljust(W - len(eol)) + eol for x in lines).encode()


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_border_cases(parser, eol):
    data = _border_log(eol)
    plan = list(StreamAnalyzer(parser.engine, chunk_bytes=10 * W)._plan(data, _eff_end(data)))
    starts = [data[:pos].count(b"\n") for _, pos, _, _, _, _ in plan]
    assert starts == [0, 10, 20, 30, 40, 50]                  # the cases straddle the boundaries 10, 20, 30, 40
    want = parser.gaps(data, top=None)
    assert want == golden.gaps(data, _library(), parser.config.scoring, None, "context")
    # candidates: 9 10 11 12 19 20 29 30 38 40 59; covered: 9 10 11 (oom), 19 20 (dup), 40 (dup)
    assert (want["events"], want["errorLines"], want["uncoveredErrorLines"], want["templates"]) == (3, 11, 5, 2)
    assert [(g["count"], g["firstLine"]) for g in want["top"]] == [(3, 31), (2, 13)]      # lines 30 38 59; 12 29
    for c in (10 * W, 2, W, 3 * W + 1, 25 * W):
        assert parser.gaps_stream(data, chunk_bytes=c, top=None) == want, c
    ev = parser.gaps(data, top=None, cover="events")
    assert ev["uncoveredErrorLines"] == 8
    assert parser.gaps_stream(data, chunk_bytes=10 * W, top=None, cover="events") == ev


# ---- 3. a resident log

def test_resident_equals_document(parser):
    data = (_planted_log() * 40).encode()
    res = parser.load_resident(data, chunk_bytes=8192)
    assert len(res.chunks) > 3
    for cover in ("context", "events"):
        assert parser.gaps_resident(res, cover=cover) == parser.gaps(data, cover=cover)
    assert parser.gaps_resident(res, top=None) == parser.gaps_stream(data, chunk_bytes=8192, top=None)


# ---- 4. empty sources

def test_empty_sources(parser):
    assert parser.gaps_stream(b"\n") == {"totalLines": 0, **ZERO} == parser.gaps(b"\n")
    for src in (b"", b"INFO all good\nDEBUG nothing 1 to see\n"):
        for c in (None, 2):
            rep = parser.gaps_stream(src, chunk_bytes=c)
            assert rep == parser.gaps(src) == {"totalLines": len(golden.split_lines(src.decode())), **ZERO}


def test_stream_from_a_path(parser, tmp_path):
    data = _planted_log().encode()
    f = tmp_path / "app.log"
    f.write_bytes(data)
    assert parser.gaps_stream(str(f), chunk_bytes=300) == parser.gaps(data)
    e = tmp_path / "empty.log"
    e.write_bytes(b"")
    assert parser.gaps_stream(str(e)) == parser.gaps(b"")


# ---- 4b. the walker itself (log_parser_amd/pieces.py)

def test_walker_leaves_nothing_behind(parser, tmp_path):
    """``stream_pieces`` over a mapped file with more chunks than the producer's queue holds, left
    by an exception after the second piece, by ``break`` there, and at its end: no producer thread
    stays behind and the mapping can be closed (no exported buffer is left). Exactly the final
    piece is ``last`` and the pieces' line numbers add up to the document's."""
    doc = ("2025-09-19T12:00:00Z INFO a\n" + "INFO filler\n" * 40 + "1999-01-01T00:00:00Z ERROR a stray old date\n"
           + "INFO filler\n" * 400 + "2025-09-19T12:00:01Z INFO b\n")
    f = tmp_path / "stray.log"
    f.write_text(doc)
    threads = threading.active_count()
    for how in ("raise", "break", "end"):
        with open(f, "rb") as fh:
            mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
            seen = []
            try:
                with stream_pieces(parser.engine, mm, 64) as pieces:
                    for piece in pieces:
                        seen.append((piece.line_base, piece.ls.numel(), piece.last))
                        if len(seen) == 2 and how == "raise":
                            raise KeyError("leave in the middle")
                        if len(seen) == 2 and how == "break":
                            break
            except KeyError:
                assert how == "raise"
            assert threading.active_count() == threads, how
            mm.close()                                        # BufferError if the producer's view were alive
        assert how == "end" or len(seen) == 2
    assert len(seen) > 8                                      # (the queue holds 2, one more is fetched ahead)
    assert [last for _, _, last in seen] == [False] * (len(seen) - 1) + [True]
    at = 0
    for base, n, _ in seen:
        assert base == at
        at += n
    assert at == len(golden.split_lines(doc)) == 443
    assert parser.gaps_stream(str(f), chunk_bytes=64) == parser.gaps(doc)


def test_raw_lines_host_and_device_agree(parser):
    """A piece's lines cut from the host bytes == gathered from the staged text."""
    data = _planted_log().encode()
    piece = document_piece(parser.engine, *parser.engine.stage_text(data), data)
    idx = torch.tensor([0, 7, 7, piece.ls.numel() - 1])
    want = [data.split(b"\n")[i] for i in idx.tolist()]
    assert piece.raw_lines(idx) == gather_lines(piece.text, piece.ls[idx], piece.ll[idx]) == want
    assert piece.raw_lines(idx[:0]) == gather_lines(piece.text, piece.ls[:0], piece.ll[:0]) == []


# ---- 5. the frequency window is not touched

def test_frequency_window_untouched():
    log = _planted_log()
    cfg = Config.load(overrides={"engine.device": "cpu", "scoring.frequency.threshold": "1.0"})
    a, b = LogParser(_library(), config=cfg), LogParser(_library(), config=cfg)
    a.parse(log)
    b.parse(log)
    before = a.frequency_statistics()
    assert before and a.gaps_stream(log.encode(), chunk_bytes=300)["events"] == 3
    assert a.frequency_statistics() == before
    assert a.gaps_corpus([log, log])["events"] == 6
    assert a.frequency_statistics() == before
    sa = [(e["lineNumber"], e["score"]) for e in a.parse(log)["events"]]
    sb = [(e["lineNumber"], e["score"]) for e in b.parse(log)["events"]]
    assert sa == sb and len(sa) == 3


# ---- 6. the batcher owns the engine after submit()

def test_batcher_guard():
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    try:
        acc = lp.gap_accumulator()
        acc.add_document("ERROR x\n")
        assert lp.gaps_stream(b"ERROR x\n")["uncoveredErrorLines"] == 1
        res = lp.load_resident(b"ERROR x\n")
        lp.submit("ERROR x\n").result(timeout=120)
        for call in (lambda: lp.gaps_stream(b"ERROR x\n"), lambda: lp.gaps_resident(res),
                     lambda: lp.gaps_corpus(["ERROR x\n"]), lambda: lp.gap_accumulator(),
                     lambda: acc.add_document("ERROR y\n"), lambda: acc.report()):
            with pytest.raises(RuntimeError):
                call()
    finally:
        lp.close()


# ---- 7. a corpus

def _corpus():
    """Five documents: template W (widget) in every document that has lines, S (shard) in two, the
    third document empty; R and Q occur once each, R in the earlier document (the tie order)."""
    return ["INFO a\nERROR widget 1 jammed\nFATAL shard 1 lost\nERROR widget 2 jammed\n",
            "ERROR widget 3 jammed\nERROR rare thing R happened\n",
            "",
            "INFO b\nINFO c\nERROR queue Q overflow\nERROR widget 4 jammed\n",
            "FATAL shard 2 lost\nFATAL shard 3 lost\nERROR widget 5 jammed\nFATAL shard 4 lost\nFATAL shard 5 lost\n"]


def test_corpus_equals_golden(parser):
    docs = _corpus()
    sets, p = _library(), parser.config.scoring
    for cover in ("context", "events"):
        for top in (20, None, 2):
            assert parser.gaps_corpus(docs, top=top, cover=cover) == golden.gaps_corpus(docs, sets, p, top, cover)
    rep = parser.gaps_corpus(docs)
    assert set(rep) == KEYS | {"documents"} and rep["documents"] == 5
    assert rep["totalLines"] == sum(len(golden.split_lines(d)) for d in docs)
    assert (rep["errorLines"], rep["uncoveredErrorLines"], rep["templates"]) == (12, 12, 4)
    got = [(g["template"], g["count"], g["documents"], g["firstDocument"], g["firstLine"]) for g in rep["top"]]
    assert got == [("ERROR widget 0 jammed", 5, 4, 0, 2), ("FATAL shard 0 lost", 5, 2, 0, 3),     # a tie: first line
                   ("ERROR rare thing R happened", 1, 1, 1, 2), ("ERROR queue Q overflow", 1, 1, 3, 3)]
    assert parser.gaps_corpus(d.encode() for d in docs) == rep            # bytes, from a generator
    empty = parser.gaps_corpus([])
    assert empty == golden.gaps_corpus([], sets, p) == {"totalLines": 0, **ZERO, "documents": 0}


def test_corpus_of_one_is_the_document(parser):
    log = _planted_log()
    assert parser.gaps_corpus([log]) == parser.gaps(log)
    assert parser.gaps_corpus([log], top=None, cover="events") == parser.gaps(log, top=None, cover="events")
    assert golden.gaps_corpus([log], _library(), parser.config.scoring) == parser.gaps(log)


def test_corpus_documents_do_not_interact(parser):
    """The last line of document k and the window of an event on the first line of document k + 1
    (and the other way round) do not meet."""
    docs = ["INFO a\nERROR widget 1 jammed\n",                               # a candidate on the last line
            "ERROR fooDup foo happened\nINFO b\njava.lang.OutOfMemoryError: x\n",   # windows reach out of both ends
            "ERROR widget 2 jammed\nERROR widget 3 jammed\n"]
    rep = parser.gaps_corpus(docs)
    assert rep == golden.gaps_corpus(docs, _library(), parser.config.scoring)
    assert (rep["events"], rep["uncoveredErrorLines"]) == (2, 3)
    assert [(g["count"], g["documents"], g["firstDocument"], g["firstLine"]) for g in rep["top"]] == [(3, 2, 0, 2)]
    joined = parser.gaps("".join(docs))                                       # one document: the windows do cover
    assert joined["uncoveredErrorLines"] == 0


def test_accumulator_over_time(parser):
    docs = _corpus()
    acc = parser.gap_accumulator()
    acc.add_document(docs[0])
    assert acc.report() == parser.gaps(docs[0])
    acc.add_stream(docs[1].encode(), chunk_bytes=2)                           # a streamed document among whole ones
    for d in docs[2:]:
        acc.add_document(d)
    assert acc.report() == golden.gaps_corpus(docs, _library(), parser.config.scoring)


# ---- 8. command line

def _cli(*argv):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "gaps", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_cli_files_and_stream(tmp_path):
    a, b = tmp_path / "a.log", tmp_path / "b.log"
    a.write_text("starting\nERROR OOMKilled container app\nERROR widget 17 jammed\nERROR widget 23 jammed\n")
    b.write_text("ERROR widget 5 jammed\nFATAL shard 2 lost\n")
    one = _cli(str(a), "--top", "5", "--cover", "events")
    assert set(one) == KEYS and one["totalLines"] == 4
    assert {"count": 2, "firstLine": 3, "template": "ERROR widget 0 jammed"}.items() <= one["top"][0].items()
    assert _cli(str(a), "--top", "5", "--cover", "events", "--stream") == one
    two = _cli(str(a), str(b), "--cover", "events")
    assert set(two) == KEYS | {"documents"} and two["documents"] == 2 and two["totalLines"] == 6
    assert {"count": 3, "documents": 2, "firstDocument": 0, "firstLine": 3,
            "template": "ERROR widget 0 jammed"}.items() <= two["top"][0].items()
