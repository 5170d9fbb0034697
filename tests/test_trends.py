"""Trends report on the CPU engine (log_parser_amd/trends.py, csrc/kernels/trends.hip host twins): the
stamp-and-signature twin against ``golden.line_signature`` / ``golden.line_timestamp``, the cell table
against a ``collections.Counter``, the report against ``golden.trends`` and against what
``synth.trend_log`` plants, for documents, streams in chunks of any size, resident logs and an
accumulator fed in parts, edge logs, arguments and the command line.

Mutations, each made once by hand and undone, and the tests of this file that failed on them:

* fill ignored (the cell fold fed the stamps instead of the effective times): test_report_matches_golden,
  test_first_event_pivot, test_streams_and_parts_give_the_document_report, test_planted_facts, test_edges,
  test_cli;
* the carry between runs dropped (``timeline_fill`` without it): test_streams_and_parts_give_the_document_report,
  test_edges, test_cli (the stream forms only: a document is one run);
* truncating instead of floor division in ``cell_bucket``: test_cell_table[bucket edges], test_edges (the
  stamp before 1970);
* ``<=`` at the pivot (the pivot's own bucket counted as before): test_report_matches_golden,
  test_first_event_pivot, test_streams_and_parts_give_the_document_report, test_planted_facts, test_edges,
  test_cli;
* min line dropped in the host fold (the first arrival kept): test_cell_table[two folds, the later lines
  first] and [empty marker as a key] -- one thread folds in line order, so only a later fold with smaller
  line numbers shows it; on the GPU the arrival order is arbitrary and every repeated cell does;
* LDS overflow dropped: the host twin has no LDS table. test_gpu_trends.py test_cell_table_gpu[3000
  distinct cells-2048] is built for it (more distinct cells in one tile than LDS slots); that mutation
  was not run.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, trend_log
from trends_cases import W, cell_cases, cells_of, check_cells, fold_all, growth_folds, late_errors, rows_of, signed, stamp_lines
from values_cases import index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
CPU = {"engine.device": "cpu"}
KEYS = {"totalLines", "datedLines", "undatedLines", "templates", "cells", "bucketSeconds", "firstBucket", "lastBucket",
        "buckets", "pivot", "pivotSource", "bucketsBefore", "bucketsAfter", "kinds", "top"}
ROW_KEYS = {"signature", "kind", "lift", "lines", "datedLines", "before", "after", "firstSeen", "lastSeen",
            "activeBuckets", "peakBucket", "peakCount", "firstLine", "template", "example"}
CASES = cell_cases()


# ---- 1. the host twin against the specification

@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_host_twin_matches_golden(L):
    lines = stamp_lines(L, seed=L)
    sigs = [signed(golden.line_signature(x)) for x in lines]
    stamps = [K.TS_NONE if t is None else t for t in map(golden.line_timestamp, lines)]
    assert L < 63 or (any(t != K.TS_NONE for t in stamps) and any(t == K.TS_NONE for t in stamps))
    for shift in (0, 1, 15):
        idx = index(lines, shift)
        sig, ts = K.line_stamps(*idx)
        assert (sig.dtype, ts.dtype) == (torch.int64, torch.int64)
        assert sig.tolist() == sigs and ts.tolist() == stamps, shift
        assert torch.equal(sig, K.line_signatures(*idx)) and torch.equal(ts, K.line_timestamps(*idx)), shift


def test_line_stamps_arguments():
    text, ls, ll = index([b"2025-09-19T12:01:02 x"], 0)
    none = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int32)
    sig, ts = K.line_stamps(text, *none)
    assert sig.numel() == ts.numel() == 0
    for bad in (lambda: K.line_stamps(text, ls, ll, per_block=4096), lambda: K.line_stamps(text, ls.int(), ll),
                lambda: K.line_stamps(text, ls, ll.long())):
        with pytest.raises(ValueError):
            bad()


# ---- 2. the cell table against a Counter

def test_cell_key_is_invertible():
    for sig in (0, 1, (1 << 64) - 1, golden.line_signature(b"served in 12ms")):
        for b in (0, 1, -1, 175828320, golden.TREND_UNDATED):
            k = golden.trend_cell_key(sig, b)
            assert 0 <= k < 1 << 64 and golden.trend_cell_sig(k, b) == sig
            assert k == (sig + b * 0x9E3779B97F4A7C15) % (1 << 64)
    assert len({golden.trend_cell_key(7, b) for b in range(-50, 50)}) == 100


@pytest.mark.parametrize("tile", [256, 2048])
@pytest.mark.parametrize("name", list(CASES))
def test_cell_table(name, tile):
    check_cells("cpu", tile, CASES[name])


def test_cell_table_grows_from_two_slots():
    table = K.CellTable("cpu", cap=2)
    caps, folds = [table.cap], growth_folds()
    for k in range(len(folds)):
        fold_all(table, folds[k:k + 1], "cpu")
        caps.append(table.cap)
        assert rows_of(table) == cells_of(folds[:k + 1]) and 2 * table.used <= table.cap
    assert len(set(caps)) >= 4 and caps == sorted(caps)         # at least three regrowths


def test_cell_table_arguments():
    table = K.CellTable("cpu")
    one = torch.zeros(1, dtype=torch.int64)
    for bad in (lambda: table.fold(one, one, 0, 0), lambda: table.fold(one, torch.zeros(2, dtype=torch.int64), 0, W),
                lambda: table.fold(one, one, -1, W), lambda: K.CellTable("cpu", cap=6), lambda: K.CellTable("cpu", tile=100)):
        with pytest.raises(ValueError):
            bad()
    table.fold(one[:0], one[:0], 0, W)
    assert table.used == 0 and all(c.numel() == 0 for c in table.rows())


# ---- 3. the report

@pytest.fixture(scope="module")
def cpu():
    return LogParser([], config=Config.load(overrides=CPU))


@pytest.fixture(scope="module")
def logs():
    """seed -> (text, planted, the stamp of line 3000 in epoch ms)."""
    out = {}
    for seed in (1, 2, 3):
        text, planted = trend_log(4000, log_templates(30, 1), seed)
        out[seed] = (text, planted, golden.line_timestamp(text.split("\n")[3000].encode()))
    return out


def parameter_sets(at_ms: int):
    sets = [{"order": o} for o in ("change", "count", "first")]
    sets += [{"kind": k, "top": None} for k in golden.TREND_KINDS + ("all",)]
    sets += [{"ratio": 2, "top": None}, {"ratio": 4, "top": 2}, {"at": at_ms}, {"at": golden.iso_ms(at_ms), "min_count": 20},
             {"at": golden.iso_ms(at_ms).replace("T", " ").replace(".000Z", ",000+00:00"), "kind": "all", "order": "first"},
             {"at": "first-error", "top": None, "kind": "all"}, {"min_count": 1, "top": None, "kind": "all"}]
    return [dict(kw, bucket_seconds=10) for kw in sets]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_report_matches_golden(cpu, logs, seed):
    text, planted, at_ms = logs[seed]
    before = cpu.frequency_statistics()
    for kw in parameter_sets(at_ms):
        if kw.get("at") == "first-error":       # (the bulk has error lines from the first bucket on: no pivot there)
            with pytest.raises(ValueError, match="first-error"):
                golden.trends(text, **kw)
            with pytest.raises(ValueError, match="first-error"):
                cpu.trends(text, **kw)
            text = late_errors(text)
        want = golden.trends(text, **kw)
        assert cpu.trends(text, **kw) == want, kw
        assert set(want) == KEYS and all(set(r) == ROW_KEYS for r in want["top"]) and want["totalLines"] == 4000
        assert want["datedLines"] == 4000 and want["buckets"] == 40 and want["bucketsBefore"] + want["bucketsAfter"] == 40
        if kw.get("kind") == "all" and kw.get("top", 20) is None:
            assert sum(want["kinds"].values()) == len(want["top"])
            assert sum(r["lines"] for r in want["top"]) <= 4000
    rep = golden.trends(late_errors(text), bucket_seconds=10, at="first-error")
    assert rep["pivotSource"] == "first-error" and rep["bucketsBefore"] >= 10
    assert cpu.frequency_statistics() == before


def test_first_event_pivot():
    lp = LogParser.from_directory(PAT, config=Config.load(overrides=CPU))
    text, _ = trend_log(1200, log_templates(10, 2), seed=5, change_at=0.5)
    lines = text.split("\n")
    for i in (700, 701, 900):
        lines[i] = lines[i][:25] + "ERROR OOMKilled container app"
    text = "\n".join(lines)
    kw = {"bucket_seconds": 10, "at": "first-event", "kind": "all", "top": None, "min_count": 1}
    want = golden.trends(text, lp.library.pattern_sets, lp.engine.lib.params, **kw)
    assert want["pivotSource"] == "first-event" and want["pivot"] == "2025-09-19T12:01:10.000Z"
    before = lp.frequency_statistics()
    assert lp.trends(text, **kw) == want
    assert lp.trends_stream(text.encode(), chunk_bytes=4096, **kw) == want
    assert lp.trends_resident(lp.load_resident(text.encode(), chunk_bytes=32768), **kw) == want
    assert lp.frequency_statistics() == before
    quiet = "\n".join(l for l in lines if "OOMKilled" not in l)
    for call in (lambda: golden.trends(quiet, lp.library.pattern_sets, lp.engine.lib.params, **kw), lambda: lp.trends(quiet, **kw),
                 lambda: lp.trends_stream(quiet.encode(), **kw), lambda: lp.trend_accumulator(10).report(at="first-event")):
        with pytest.raises(ValueError):
            call()


def test_streams_and_parts_give_the_document_report(cpu, logs):
    text, planted, at_ms = logs[2]
    text = late_errors(text)
    data = text.encode()
    for kw in ({"bucket_seconds": 10, "kind": "all", "top": None, "min_count": 1},
               {"bucket_seconds": 10, "at": at_ms, "min_count": 20}, {"bucket_seconds": 10, "at": "first-error", "order": "count"}):
        want = golden.trends(text, **kw)
        for c in (4096, 1 << 22):
            assert cpu.trends_stream(data, chunk_bytes=c, **kw) == want, (kw, c)
        res = cpu.load_resident(data, chunk_bytes=32768)
        assert len(res.chunks) > 3 and cpu.trends_resident(res, **kw) == want
        if kw.get("at") == "first-error":
            continue
        acc = cpu.trend_accumulator(10)                                             # one log in two parts
        cut = data.index(b"\n", len(data) // 2) + 1
        acc.add_document(data[:cut])
        acc.add_stream(data[cut:], 50000)
        assert acc.report(**{k: v for k, v in kw.items() if k != "bucket_seconds"}) == want
    # one-line chunks: unstamped lines at chunk heads take the carried time
    head = "".join(text.splitlines(keepends=True)[:400])
    assert sum(1 for l in head.split("\n") if l.startswith("\tat")) > 5
    kw = {"bucket_seconds": 10, "kind": "all", "top": None, "min_count": 1}
    assert cpu.trends_stream(head.encode(), chunk_bytes=64, **kw) == golden.trends(head, **kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_facts(cpu, logs, seed):
    text, (stopped, started, surged), at_ms = logs[seed]
    rep = golden.trends(text, bucket_seconds=10, at=at_ms, min_count=20, order="change")
    assert rep["pivot"] == "2025-09-19T12:05:00.000Z" and (rep["bucketsBefore"], rep["bucketsAfter"]) == (30, 10)
    rows = rep["top"]
    assert [r["kind"] for r in rows[:3]] == ["started", "stopped", "surged"]
    for r, planted in zip(rows, (started, stopped, surged)):
        assert planted.split("%d")[0] in r["example"]
    change = [max(r["lift"], 1 / r["lift"]) for r in rows]
    # by construction: about 50 error lines after the change ((n + 1) * 30 / 10), 150 heartbeats before
    # it (151 * 10 / 30), the surging line on 1 % and then 10 % of the lines
    assert 120 <= change[0] <= 200 and rows[0]["before"] == 0 and rows[0]["firstSeen"] == rep["pivot"]
    assert change[1] == pytest.approx(151 / 3) and (rows[1]["before"], rows[1]["after"]) == (150, 0)
    assert rows[1]["lastSeen"] == "2025-09-19T12:04:50.000Z" and rows[1]["activeBuckets"] == 30 and rows[1]["peakCount"] == 5
    assert 6 <= change[2] <= 16 and all(c < 4 for c in change[3:])
    assert cpu.trends(text, bucket_seconds=10, at=at_ms, min_count=20) == rep
    # the pivot matters: from the middle of the log the heartbeat is steady (100 lines before, 50 after)
    mid = golden.trends(text, bucket_seconds=10, min_count=20, kind="all", top=None)
    beat = [r for r in mid["top"] if stopped.split("%d")[0] in r["example"]]
    assert mid["pivotSource"] == "middle" and [(r["kind"], r["before"], r["after"]) for r in beat] == [("steady", 100, 50)]


# ---- 4. edges

def test_edges(cpu):
    S = "2025-09-19T12:00:%02d "
    all_kw = {"bucket_seconds": 10, "kind": "all", "top": None, "min_count": 1}
    logs = {
        "empty": "", "blank": "\n", "no stamp": "a 1\nb 2\na 3\n", "one bucket": "".join(S % i + "x %d\n" % i for i in range(10)),
        "undated head": "head 1\nhead 2\n" + "".join(S % i + "x %d\n" % i for i in range(0, 60, 3)) + "\tat tail\n",
        "crlf": "".join((S % i + "x %d\r\n" % i) + ("\tat frame %d\r\n" % i) for i in range(0, 60, 2)),
        "before 1970": "1970-01-01T00:00:00+05:00 early\n" * 3 + "1970-01-01T00:00:05+05:00 early\n1970-01-01T04:59:59.999+05:00 late 1\n"
                       + "1970-01-01T05:00:00+05:00 late 2\n" * 2,
        "out of order": "".join(S % i + "x\n" for i in (50, 10, 30, 10, 59, 0)),
    }
    for name, text in logs.items():
        kw = dict(all_kw, max_buckets=1 << 20)
        want = golden.trends(text, **kw)
        assert cpu.trends(text, **kw) == want, name
        assert cpu.trends_stream(text.encode(), chunk_bytes=64, **kw) == want, name
        assert set(want) == KEYS and want["totalLines"] == len(golden.split_lines(text))
    for name in ("empty", "blank", "no stamp", "one bucket"):
        rep = golden.trends(logs[name], **all_kw)
        assert rep["pivot"] is None and rep["top"] == [] and rep["pivotSource"] is None, name
        if name != "one bucket":                # (without a dated line the named pivots are not looked up)
            assert rep == golden.trends(logs[name], **dict(all_kw, at="first-event"))
            assert rep == cpu.trends(logs[name], **dict(all_kw, at="first-error"))
    rep = golden.trends(logs["no stamp"], **all_kw)
    assert (rep["totalLines"], rep["datedLines"], rep["undatedLines"], rep["templates"], rep["cells"], rep["buckets"]) == (3, 0, 3, 2, 2, 0)
    assert golden.trends(logs["one bucket"], **all_kw)["buckets"] == 1
    rep = golden.trends(logs["undated head"], **all_kw)
    assert (rep["undatedLines"], rep["datedLines"], rep["cells"]) == (2, 21, 8) and rep["templates"] == 3
    # (the template of the two head lines has no dated line: counted, never listed)
    assert [(r["example"], r["lines"], r["kind"]) for r in rep["top"]] == [("\tat tail", 1, "started"), (S % 0 + "x 0", 20, "steady")]
    rep = golden.trends(logs["before 1970"], **dict(all_kw, max_buckets=1 << 20))
    assert rep["firstBucket"] == "1969-12-31T19:00:00.000Z" and rep["lastBucket"] == "1970-01-01T00:00:00.000Z"
    assert rep["buckets"] == 1801 and sorted((r["before"], r["after"], r["firstSeen"]) for r in rep["top"]) == \
        [(0, 1, "1969-12-31T23:59:50.000Z"), (0, 2, "1970-01-01T00:00:00.000Z"), (4, 0, "1969-12-31T19:00:00.000Z")]
    # the pivot: outside the span, on the first bucket, unparsable; the span against max_buckets
    text = logs["undated head"]
    for at in ("2025-09-19T12:00:00", "2025-09-19T12:00:09.999Z", "2025-09-19T12:01:00", 0, "yesterday", "x2025-09-19T12:00:30",
               " 2025-09-19T12:00:30", "2025-13-19T12:00:30", "", 1.5, True, "first-event"):
        for call in (lambda: golden.trends(text, **dict(all_kw, at=at)), lambda: cpu.trends(text, **dict(all_kw, at=at)),
                     lambda: cpu.trends_stream(text.encode(), **dict(all_kw, at=at))):
            with pytest.raises(ValueError):
                call()
    assert golden.trends(text, **dict(all_kw, at="2025-09-19T12:00:10"))["bucketsBefore"] == 1
    assert cpu.trends(text, **dict(all_kw, at="2025-09-19T12:00:59.999"))["bucketsAfter"] == 1
    for call in (lambda: golden.trends(text, **dict(all_kw, max_buckets=5)), lambda: cpu.trends(text, **dict(all_kw, max_buckets=5)),
                 lambda: cpu.trends_stream(text.encode(), chunk_bytes=64, **dict(all_kw, max_buckets=5))):
        with pytest.raises(ValueError, match="max_buckets=5"):
            call()
    assert cpu.trends(text, **dict(all_kw, max_buckets=6))["buckets"] == 6


def test_bad_arguments_raise(cpu):
    log = "2025-09-19T12:00:00 a\n2025-09-19T12:01:00 a\n"
    res = cpu.load_resident(log.encode())
    for kw in ({"ratio": 1}, {"ratio": 2.5}, {"ratio": True}, {"order": "peak"}, {"order": ""}, {"kind": "new"}, {"kind": ""},
               {"min_count": 0}, {"min_count": 2.5}, {"bucket_seconds": 0}, {"bucket_seconds": 1.5}, {"max_buckets": 0}):
        with pytest.raises(ValueError):
            golden.trends(log, **kw)
        acc_kw = {k: v for k, v in kw.items() if k != "bucket_seconds"}
        for call in (lambda: cpu.trends(log, **kw), lambda: cpu.trends_file(os.path.join(ROOT, "no", "such", "file"), **kw),
                     lambda: cpu.trends_stream(log.encode(), **kw), lambda: cpu.trends_resident(res, **kw),
                     lambda: cpu.engine.trends_bytes(log.encode(), **kw),
                     lambda: cpu.trend_accumulator(kw.get("bucket_seconds", 60)).report(**acc_kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="does not have the template"):
        golden.trends_row(1, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0, b"a line", 1000, "started", golden.trends_lift(0, 1, 1, 1))


def _cli(*argv, code: int = 0):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "trends", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == code, r.stderr
    return json.loads(r.stdout) if code == 0 else r.stderr


def test_cli(tmp_path, logs):
    text, planted, at_ms = logs[1]
    log = tmp_path / "app.log"
    log.write_text(text)
    one = _cli(str(log), "--bucket", "10", "--at", golden.iso_ms(at_ms), "--min-count", "20")
    assert one == golden.trends(text, bucket_seconds=10, at=at_ms, min_count=20) and one["top"][0]["kind"] == "started"
    other = _cli(str(log), "--stream", "--chunk-bytes", "4096", "--bucket", "10", "--at", str(at_ms), "--ratio", "2", "--kind", "all",
                 "--order", "count", "--top", "3")
    assert other == golden.trends(text, bucket_seconds=10, at=at_ms, ratio=2, kind="all", order="count", top=3)
    assert "pivot" in _cli(str(log), "--at", "2020-01-01T00:00:00", code=2)
