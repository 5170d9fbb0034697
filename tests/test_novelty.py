"""Novelty report on the CPU engine (log_parser_amd/novelty.py, csrc/kernels/novelty.hip host twins):
the one-pass sign / probe / compact kernel against ``golden.line_signature`` membership, the report
against ``golden.novelty`` for documents, streams in chunks of any size and resident logs, the
baseline's sources and its file format, side effects, guards and the command line."""
import json
import mmap
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from log_parser_amd import golden
from log_parser_amd import novelty as NV
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.pieces import stream_pieces
from log_parser_amd.utils.config import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
KEYS = {"totalLines", "events", "errorLines", "novelLines", "novelErrorLines", "templates", "errorTemplates",
        "baseline", "top"}
GROUP_KEYS = {"count", "errorLines", "eventLines", "firstLine", "signature", "template", "example"}


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


def _library():
    """An event with a context window, one without rules, and a backreference on the host side path."""
    return [PatternSet.model_validate({"metadata": {"library_id": "novelty"}, "patterns": [
        {"id": "oom", "name": "oom", "severity": "CRITICAL",
         "primary_pattern": {"regex": r"OutOfMemoryError", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "quota", "name": "quota", "severity": "HIGH",
         "primary_pattern": {"regex": r"disk quota exceeded", "confidence": 0.8}},
        {"id": "dup", "name": "backref", "severity": "LOW",
         "primary_pattern": {"regex": r"(\w+)Dup \1", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


# the healthy templates, and the ones only the failing log shows: error lines, plain lines, lines
# with an event on them (two patterns on one line too), an event line the baseline knows
HEALTHY = ["INFO request %d served in %dms", "DEBUG cache shard %d hit ratio 0.%d", "WARN slow disk sd%d \t latency %dms",
           "INFO héartbeat from node-%d", "", "ERROR transient glitch %d recovered", "WARN disk quota exceeded on /data%d"]
HELD_OUT = ["ERROR [worker-%d] connection to 10.0.%d.7:5432 refused", "FATAL cache shard %d lost quorum",
            "INFO leader election %d started", "java.lang.OutOfMemoryError: Java heap space %d",
            "\tat com.acme.Pool.grow(Pool.java:%d)", "ERROR fooDup foo after disk quota exceeded %d",
            "request %d failed: TimeoutException"]


def _fill(rng, t: str) -> str:
    return t % tuple(rng.randrange(1000) for _ in range(t.count("%d")))


def _log(templates, n: int, seed: int, eol: str = "\n") -> str:
    """``n`` lines of ``templates``, with uneven counts; ends with a line that is not empty."""
    rng = random.Random(seed)
    w = [1.0 / (k + 1) for k in range(len(templates))]
    lines = [_fill(rng, t) for t in rng.choices(templates, weights=w, k=n)] + [_fill(rng, templates[0])]
    return eol.join(lines) + eol


@pytest.fixture(scope="module")
def parser():
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    assert lp.library.summary()["host_fallback"] == 1
    return lp


@pytest.fixture(scope="module")
def case(parser):
    """(healthy document, failing log, the baseline of the healthy document, golden report with every group)."""
    healthy = _log(HEALTHY, 200, seed=1)
    log = _log(HEALTHY + HELD_OUT, 400, seed=2)
    base = parser.baseline()
    base.add_document(healthy)
    want = golden.novelty(log, [healthy], _library(), parser.config.scoring, None)
    # by construction: exactly the held-out templates are novel (every one occurs in 400 lines)
    assert want["templates"] == len(HELD_OUT) and want["baseline"]["templates"] == len(HEALTHY)
    assert want["events"] > 0 and 0 < want["errorTemplates"] < want["templates"]
    assert any(g["eventLines"] for g in want["top"]) and any(not g["eventLines"] for g in want["top"])
    assert want["errorLines"] > want["novelErrorLines"] > 0      # (a healthy template is an error line too)
    return healthy, log, base, want


# ---- 1. the host twin against golden.line_signature membership

def _crafted_lines():
    rng = random.Random(3)
    lines = [bytes(rng.choice(b"ab1 9\tZ-.:") for _ in range(n)) for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 5000)]
    lines += [b"a \t\t  b\t \tc", b"a b c", b"\t\tlead and trail  ", b" lead and trail\t"]   # runs of tabs / spaces
    lines += [b"caf\xc3\xa9 \xff\xfe 42 \x80\x80abc1\x80", bytes(range(128, 256)) * 3]       # bytes >= 0x80
    lines += [b"retry in 30", b"retry in 7", b"code=x9f", b"id 12345678901234567890"]         # digit tokens at the end
    lines += [b"x" * 1020 + b" tail AAAA", b"x" * 1020 + b" tail BBBB"]                       # differ after byte 1024
    lines += [b"", b"plain words only", b"plain words only"]
    return lines


def _stage(data: bytes) -> torch.Tensor:
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return text


def test_host_twin_matches_golden():
    lines = _crafted_lines()
    data = b"\n".join(lines) + b"\nend"
    lines.append(b"end")
    text = _stage(data)
    ls, ll = K.split_lines(text, len(data))
    L = len(lines)
    assert ls.numel() == L
    sigs = [golden.line_signature(x) for x in lines]
    a, b = lines.index(b"x" * 1020 + b" tail AAAA"), lines.index(b"x" * 1020 + b" tail BBBB")
    assert sigs[a] == sigs[b] and sigs[lines.index(b"a \t\t  b\t \tc")] == sigs[lines.index(b"a b c")]
    rng = random.Random(5)
    feat = torch.tensor([rng.choice((0, 1, 2, 4, 5, 8, 9, 12)) for _ in range(L)], dtype=torch.uint8)
    evm = torch.tensor([rng.random() < 0.3 for _ in range(L)], dtype=torch.uint8)
    cand = [(f & 9) != 0 and (f & 4) == 0 for f in feat.tolist()]
    held = {a, lines.index(b"a b c"), lines.index(b"retry in 30"), 0, 3, 8}     # lines whose signature the baseline holds
    base = {sigs[i] for i in held}
    table = K.GapTable.from_signatures("cpu", torch.tensor(sorted(_signed(s) for s in base), dtype=torch.int64))
    want = [(i, _signed(sigs[i])) for i in range(L) if sigs[i] not in base]
    assert b not in [i for i, _ in want] and lines.index(b"retry in 7") not in [i for i, _ in want]
    for f, e in ((feat, evm), (feat, None), (None, evm), (None, None)):
        flags = [(1 if f is not None and cand[i] else 0) | (2 if e is not None and evm[i] else 0) for i, _ in want]
        counts = (sum(cand) if f is not None else 0, len(want),
                  sum(cand[i] for i, _ in want) if f is not None else 0)
        for cap in (None, L, 1, 0):                               # cap below the count: the re-run
            line, sig, flag, cnt = K.novel_lines(text, ls, ll, table, f, e, cap=cap)
            assert line.dtype == torch.int32 and sig.dtype == torch.int64 and flag.dtype == torch.uint8
            assert list(zip(line.tolist(), sig.tolist())) == want          # (the twin appends in line order)
            assert flag.tolist() == flags and cnt == counts
    # an empty table: every line; a table that holds everything: none
    line, _, _, cnt = K.novel_lines(text, ls, ll, K.GapTable("cpu"), feat, evm)
    assert line.tolist() == list(range(L)) and cnt == (sum(cand), L, sum(cand))
    full = K.GapTable.from_signatures("cpu", torch.tensor(sorted({_signed(s) for s in sigs}), dtype=torch.int64))
    line, _, _, cnt = K.novel_lines(text, ls, ll, full, feat, evm)
    assert line.numel() == 0 and cnt == (sum(cand), 0, 0)
    with pytest.raises(ValueError):
        K.novel_lines(text, ls, ll, table, feat.long(), None)
    with pytest.raises(ValueError):
        K.novel_lines(text, ls, ll, table, None, evm[:3])


# ---- 2. the report against golden.novelty

@pytest.mark.parametrize("order", ["count", "first"])
@pytest.mark.parametrize("errors_only", [False, True])
def test_report_equals_golden(parser, case, order, errors_only):
    healthy, log, base, full = case
    for top in (0, 3, None):
        want = golden.novelty(log, [healthy], _library(), parser.config.scoring, top, order, errors_only)
        got = parser.novelty(log, base, top=top, order=order, errors_only=errors_only)
        assert got == want and set(got) == KEYS
        assert all(set(g) == GROUP_KEYS for g in got["top"])
        assert {k: v for k, v in got.items() if k != "top"} == {k: v for k, v in full.items() if k != "top"}
    assert len(got["top"]) == (full["errorTemplates"] if errors_only else full["templates"])     # top=None: every group
    firsts = [g["firstLine"] for g in got["top"]]
    if order == "first":
        assert firsts == sorted(firsts)
    else:
        assert [(-g["count"], g["firstLine"]) for g in got["top"]] == sorted((-g["count"], g["firstLine"]) for g in got["top"])
    assert sum(g["count"] for g in parser.novelty(log, base, top=None)["top"]) == full["novelLines"]


def test_bad_order_raises(parser, case):
    healthy, log, base, _ = case
    with pytest.raises(ValueError):
        golden.novelty(log, [healthy], _library(), parser.config.scoring, order="line")
    for call in (lambda: parser.novelty(log, base, order="line"),
                 lambda: parser.novelty_stream(log.encode(), base, order="line"),
                 lambda: parser.novelty_resident(parser.load_resident(log.encode()), base, order=""),
                 lambda: NV.NoveltyAccumulator(parser.engine, base).report(order="Count")):
        with pytest.raises(ValueError):
            call()


# ---- 3. sources and chunking

W = 96              # bytes per line, line end included


def _padded_log(eol: str, templates, n: int, seed: int) -> bytes:
    """``n`` lines of W bytes each: chunks of k * W bytes hold k lines."""
    rng = random.Random(seed)
    lines = [_fill(rng, t) for t in rng.choices(templates, k=n)]
    return "".join(x.ljust(W - len(eol)) + eol for x in lines).encode()


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_stream_equals_document(parser, case, eol):
    healthy = _padded_log(eol, HEALTHY, 40, seed=12)             # (padded: the trailing blanks are part of a template)
    data = _padded_log(eol, HEALTHY + HELD_OUT, 60, seed=11)
    base = parser.baseline()
    base.add_document(healthy)
    want = parser.novelty(data, base, top=None)
    assert want == golden.novelty(data, [healthy], _library(), parser.config.scoring, None)
    assert want["totalLines"] == 60 and 10 < want["novelLines"] < 50 and want["events"] > 0
    for c, per_chunk in ((W, 1), (3 * W, 3), (25 * W, 25), (1 << 20, 60)):
        with stream_pieces(parser.engine, data, c) as pieces:
            assert max(p.ls.numel() for p in pieces) == per_chunk          # 1-line, 3-line and many-line chunks
        for order in ("count", "first"):
            got = parser.novelty_stream(data, base, chunk_bytes=c, top=None, order=order)
            assert got == parser.novelty(data, base, top=None, order=order), (c, order)
        assert parser.novelty_stream(data, base, chunk_bytes=c, top=2, errors_only=True) == \
            parser.novelty(data, base, top=2, errors_only=True), c


def test_resident_and_path_equal_document(parser, case, tmp_path):
    _, log, base, want = case
    data = log.encode()
    res = parser.load_resident(data, chunk_bytes=2048)
    assert len(res.chunks) > 3
    assert parser.novelty_resident(res, base, top=None) == want
    assert parser.novelty_resident(res, base, top=3, order="first") == parser.novelty(data, base, top=3, order="first")
    f = tmp_path / "app.log"
    f.write_bytes(data)
    assert parser.novelty_stream(str(f), base, chunk_bytes=300, top=None) == want
    assert parser.novelty_file(str(f), base, top=None) == want
    e = tmp_path / "empty.log"
    e.write_bytes(b"")
    assert parser.novelty_stream(str(e), base) == parser.novelty(b"", base)


def test_accumulator_continues_one_log(parser, case):
    """Further sources continue the same log: document + stream + resident == the whole document."""
    _, log, base, want = case
    lines = log.split("\n")[:-1]
    a, b, c = ("\n".join(x) + "\n" for x in (lines[:100], lines[100:250], lines[250:]))
    acc = NV.NoveltyAccumulator(parser.engine, base)
    acc.add_document(a)
    acc.add_stream(b.encode(), chunk_bytes=128)
    acc.add_resident(parser.load_resident(c.encode(), chunk_bytes=1024))
    assert acc.report(top=None) == want


def test_empty_targets_and_baselines(parser, case):
    healthy, log, base, _ = case
    sets, p = _library(), parser.config.scoring
    zero = {"events": 0, "errorLines": 0, "novelLines": 0, "novelErrorLines": 0, "templates": 0, "errorTemplates": 0,
            "baseline": {"documents": 1, "lines": 201, "templates": len(HEALTHY)}, "top": []}
    for call in (lambda d: parser.novelty(d, base), lambda d: parser.novelty_stream(d, base),
                 lambda d: parser.novelty_stream(d, base, chunk_bytes=2)):
        assert call(b"\n") == {"totalLines": 0, **zero} == golden.novelty("\n", [healthy], sets, p)
        assert call(b"") == {"totalLines": 1, **zero} == golden.novelty("", [healthy], sets, p)    # the empty line is known
    # an empty baseline: every line is novel
    none = parser.baseline()
    for src in (b"", log.encode()):
        want = golden.novelty(src, [], sets, p, None)
        assert want["novelLines"] == want["totalLines"] > 0 and want["baseline"] == {"documents": 0, "lines": 0, "templates": 0}
        assert parser.novelty(src, none, top=None) == want == parser.novelty_stream(src, none, chunk_bytes=256, top=None)
    # a baseline that holds the target: nothing is novel
    both = parser.baseline()
    both.add_document(healthy)
    both.add_document(log)
    rep = parser.novelty(log, both)
    assert rep == golden.novelty(log, [healthy, log], sets, p)
    assert rep["novelLines"] == 0 and rep["top"] == [] and rep["errorLines"] > 0 and rep["baseline"]["documents"] == 2


def test_baseline_sources_agree(parser, case, tmp_path):
    healthy, log, base, _ = case
    docs = [healthy, log.replace("\n", "\r\n"), "", "\n", "one line without an end"]
    sigs, n_lines, n_docs = golden.baseline_signatures(docs)
    assert golden.baseline_signatures(d.encode() for d in docs) == (sigs, n_lines, n_docs)
    want = sorted(_signed(s) for s in sigs)
    whole = parser.baseline()
    for d in docs:
        whole.add_document(d)
    assert (whole.lines, whole.documents, whole.templates) == (n_lines, n_docs, len(sigs))
    assert whole.signatures().tolist() == want
    for c in (2, 64, 300, 1 << 20):
        b = parser.baseline()
        for k, d in enumerate(docs):
            if k == 1:
                b.add_resident(parser.load_resident(d.encode(), chunk_bytes=max(c, 512)))
            else:
                b.add_stream(d.encode(), chunk_bytes=c)
        assert (b.lines, b.documents, b.templates) == (n_lines, n_docs, len(sigs)), c
        assert b.signatures().tolist() == want, c
    f = tmp_path / "healthy.log"
    f.write_text(healthy)
    b = parser.baseline()
    b.add_file(str(f))
    assert b.signatures().tolist() == base.signatures().tolist() and b.lines == base.lines == 201
    with pytest.raises(ValueError):
        NV.Baseline("cpu").add_document(healthy)                  # a device alone stages nothing


def test_baseline_table_follows_the_templates(parser):
    """Many lines, few templates: the table stays small (it is sized by the folds' pairs, and
    after the first chunk next to nothing is folded)."""
    doc = _log(HEALTHY, 20000, seed=4)
    b = parser.baseline()
    b.add_stream(doc.encode(), chunk_bytes=1 << 16)
    assert b.lines == 20001 and b.templates == len(HEALTHY)
    assert b.table.cap <= 1 << 13                                 # the first chunk's ~1000 lines, not 20000


def test_wrong_device_raises(parser, case):
    class Elsewhere:
        device = torch.device("meta")
    with pytest.raises(ValueError):
        NV.NoveltyAccumulator(parser.engine, Elsewhere())
    with pytest.raises(ValueError):
        K.novel_lines(_stage(b"a"), torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32), Elsewhere())


# ---- 4. persistence

def test_baseline_save_load(parser, case, tmp_path):
    healthy, log, base, want = case
    path = tmp_path / "base.npz"
    base.save(str(path))
    with np.load(str(path), allow_pickle=False) as z:
        assert set(z.files) == {"format", "sig_max_bytes", "lines", "documents", "sig"}
        assert int(z["format"]) == 1 and int(z["sig_max_bytes"]) == golden.SIG_MAX_BYTES
        assert (int(z["lines"]), int(z["documents"])) == (201, 1)
        assert z["sig"].dtype == np.int64 and z["sig"].tolist() == sorted(z["sig"].tolist()) == base.signatures().tolist()
    got = parser.load_baseline(str(path))
    assert (got.lines, got.documents, got.templates) == (201, 1, len(HEALTHY))
    assert parser.novelty(log, got, top=None) == want
    assert NV.Baseline.load(str(path), "cpu").signatures().tolist() == base.signatures().tolist()
    # continued: the held-out templates join the set
    got.add_document(log)
    sigs, n_lines, _ = golden.baseline_signatures([healthy, log])
    assert (got.lines, got.documents, got.templates) == (n_lines, 2, len(sigs))
    assert got.signatures().tolist() == sorted(_signed(s) for s in sigs)
    assert parser.novelty(log, got)["novelLines"] == 0


def test_baseline_load_refuses(tmp_path):
    good = {"format": np.int64(1), "sig_max_bytes": np.int64(golden.SIG_MAX_BYTES), "lines": np.int64(3),
            "documents": np.int64(1), "sig": np.array([-5, 7, 9], dtype=np.int64)}
    path = str(tmp_path / "b.npz")

    def write(**kw):
        with open(path, "wb") as f:
            np.savez(f, **{k: v for k, v in {**good, **kw}.items() if v is not None})

    write()
    assert NV.Baseline.load(path, "cpu").signatures().tolist() == [-5, 7, 9]
    for bad in ({"format": np.int64(2)}, {"sig_max_bytes": np.int64(512)}, {"sig": np.array([1.0, 2.0])},
                {"sig": np.array([1, 2], dtype=np.int32)}, {"sig": np.zeros((2, 2), dtype=np.int64)},
                {"sig": np.array([7, 9, 7], dtype=np.int64)}, {"lines": None}):
        write(**bad)
        with pytest.raises(ValueError):
            NV.Baseline.load(path, "cpu")


def test_table_from_signatures_and_contains():
    E = K.GT_EMPTY
    sig = torch.tensor([5, -9, 1 << 40, 123456789], dtype=torch.int64)
    with pytest.raises(ValueError):
        K.GapTable.from_signatures("cpu", torch.tensor([5, 7, 5], dtype=torch.int64))
    with pytest.raises(ValueError):
        K.GapTable.from_signatures("cpu", sig, cap=2)
    ask = torch.tensor([5, 6, E, -9, 0, 123456789, 1 << 40, E], dtype=torch.int64)
    for cap in (None, 4, 8):                                      # 4: a full table, every probe chain wraps or ends at cap
        t = K.GapTable.from_signatures("cpu", sig, cap=cap)
        assert t.used == 4 and sorted(t.rows()[0].tolist()) == sorted(sig.tolist())
        got = t.contains(ask)
        assert got.dtype == torch.bool and got.tolist() == [True, False, False, True, False, True, True, False]
        assert t.contains(ask[:0]).numel() == 0
    t = K.GapTable.from_signatures("cpu", torch.cat([sig, torch.tensor([E])]))     # the marker's bit pattern as a signature
    assert t.used == 5 and t.contains(ask).tolist() == [True, False, True, True, False, True, True, True]
    # ... and it can be folded into afterwards
    t.fold(torch.tensor([77, 5], dtype=torch.int64), torch.tensor([3, 4], dtype=torch.int64))
    assert t.used == 6 and t.contains(torch.tensor([77, 78])).tolist() == [True, False]
    empty = K.GapTable.from_signatures("cpu", sig[:0])
    assert empty.used == 0 and empty.contains(ask).tolist() == [False] * 8


def test_baseline_contains(parser, case):
    _, _, base, _ = case
    rng = random.Random(0)
    known = golden.line_signature(_fill(rng, HEALTHY[0]).encode())
    new = golden.line_signature(_fill(rng, HELD_OUT[0]).encode())
    assert base.contains([known, new, _signed(known), golden.line_signature(b"")]).tolist() == [True, False, True, True]
    assert base.contains(torch.tensor([_signed(new), K.GT_EMPTY])).tolist() == [False, False]


# ---- 5. side effects and guards

def test_frequency_window_untouched(case):
    healthy, log, _, _ = case
    cfg = Config.load(overrides={"engine.device": "cpu", "scoring.frequency.threshold": "1.0"})
    a, b = LogParser(_library(), config=cfg), LogParser(_library(), config=cfg)
    a.parse(log)
    b.parse(log)
    before = a.frequency_statistics()
    base = a.baseline()
    base.add_document(healthy)
    base.add_stream(healthy.encode(), chunk_bytes=300)
    assert before and a.novelty(log, base)["events"] > 0
    assert a.novelty_stream(log.encode(), base, chunk_bytes=300)["events"] > 0
    assert a.novelty_resident(a.load_resident(log.encode(), chunk_bytes=2048), base)["events"] > 0
    assert a.frequency_statistics() == before
    sa = [(e["lineNumber"], e["score"]) for e in a.parse(log)["events"]]
    sb = [(e["lineNumber"], e["score"]) for e in b.parse(log)["events"]]
    assert sa == sb and len(sa) > 0


def test_batcher_guard():
    lp = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    try:
        base = lp.baseline()
        base.add_document("INFO fine\n")
        assert lp.novelty_stream(b"ERROR x\n", base)["novelLines"] == 1
        res = lp.load_resident(b"ERROR x\n")
        lp.submit("ERROR x\n").result(timeout=120)
        for call in (lambda: lp.novelty(b"ERROR x\n", base), lambda: lp.novelty_stream(b"ERROR x\n", base),
                     lambda: lp.novelty_resident(res, base), lambda: lp.novelty_file(__file__, base),
                     lambda: lp.baseline(), lambda: base.add_document("INFO y\n"),
                     lambda: base.add_stream(b"INFO y\n"), lambda: base.contains([1])):
            with pytest.raises(RuntimeError, match="novelty"):
                call()
    finally:
        lp.close()


def test_abandoned_streams_leave_nothing_behind(parser, case, tmp_path, monkeypatch):
    """A baseline stream and a report stream over a mapped file, left by an exception after the
    second chunk: no producer thread stays behind and the mapping can be closed."""
    _, _, base, _ = case
    f = tmp_path / "big.log"
    f.write_text("INFO filler line\n" * 600)
    real = K.novel_lines
    threads = threading.active_count()
    for run in (lambda mm: parser.baseline().add_stream(mm, chunk_bytes=64),
                lambda mm: parser.novelty_stream(mm, base, chunk_bytes=64)):
        calls = []

        def failing(*a, **kw):
            calls.append(1)
            if len(calls) == 2:
                raise KeyError("leave in the middle")
            return real(*a, **kw)

        monkeypatch.setattr(K, "novel_lines", failing)
        with open(f, "rb") as fh:
            mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
            with pytest.raises(KeyError):
                run(mm)
            assert len(calls) == 2 and threading.active_count() == threads
            mm.close()                                            # BufferError if the producer's view were alive
        monkeypatch.setattr(K, "novel_lines", real)
    assert parser.novelty_stream(str(f), base, chunk_bytes=64)["totalLines"] == 600       # the parser's lock was released


# ---- 6. command line

def _cli(*argv):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "novel", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_cli(tmp_path):
    h1, h2, log, npz = (tmp_path / n for n in ("h1.log", "h2.log", "app.log", "base.npz"))
    h1.write_text("starting\nINFO request 1 served in 20ms\nINFO request 2 served in 31ms\n")
    h2.write_text("INFO héartbeat from node-3\r\nERROR transient glitch 4 recovered\r\n")
    log.write_text("starting\nINFO request 7 served in 9ms\nERROR widget 17 jammed\nINFO leader election 2 started\n"
                   "ERROR OOMKilled container app\nERROR widget 23 jammed\nERROR transient glitch 9 recovered\n")
    one = _cli(str(log), "--baseline", str(h1), str(h2), "--save-baseline", str(npz), "--top", "5")
    assert set(one) == KEYS and one["totalLines"] == 7 and one["novelLines"] == 4 and one["templates"] == 3
    assert one["baseline"] == {"documents": 2, "lines": 5, "templates": 4}
    assert {"count": 2, "errorLines": 2, "firstLine": 3, "template": "ERROR widget 0 jammed"}.items() <= one["top"][0].items()
    assert _cli(str(log), "--baseline-file", str(npz), "--top", "5") == one
    assert _cli(str(log), "--baseline-file", str(npz), "--top", "5", "--stream", "--chunk-bytes", "32") == one
    first = _cli(str(log), "--baseline-file", str(npz), "--order", "first", "--errors-only")
    assert [g["firstLine"] for g in first["top"]] == [3, 5] and first["templates"] == 3 and first["errorTemplates"] == 2
