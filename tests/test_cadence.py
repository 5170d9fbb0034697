"""Cadence report on the CPU engine (log_parser_amd/cadence.py, csrc/kernels/cadence.hip host twins):
the beat scan against a plain Python loop, the state across runs, the report against
``golden.cadence`` and against what ``synth.cadence_log`` plants, for documents, streams in chunks of
any size, resident logs and an accumulator fed in parts, edge logs, arguments and the command line.
The device kernels share ``cd_join`` / ``cd_step`` / ``cd_bucket`` with the twins; their sort, their
scans and their block borders are test_gpu_cadence.py's.

Mutations, each made once by hand in csrc/kernels/cadence.hip and undone, and the tests of this file
that failed on them:

* the border beat wins a tie against an earlier maximum (``beat >= r.mx`` in ``cd_join``):
  test_beat_scan[equal maxima inside a tile], [equal maxima, the border beat second], [equal stamps], [one
  signature on every line], [one row per tile, 300 tiles], [rows past every link block], [borders only;
  first and last lines of tiles], test_edges;
* a later maximum wins a tie (``b.mx >= r.mx``): test_beat_scan[equal maxima, one the border beat], [equal
  maxima, the border beat second], [one signature on every line], test_edges;
* the link twin joins a signature's rows in the wrong order (``cd_join(mine, cur)``): 15 test_beat_scan
  cases, among them every case of several tiles or runs, the six multi-run cases of
  test_state_of_split_runs_is_the_state_of_the_joined_run, test_small_capacity_reruns,
  test_report_matches_golden, test_streams_and_parts_give_the_document_report, test_edges, test_cli."""
import json
import os

import pytest
import torch

from cadence_cases import (NONE, TILE, expected, joined, parameter_sets, report_log, run_case, run_runs, scan_cases,
                           wanted)
from log_parser_amd import golden
from log_parser_amd.__main__ import main
from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import CADENCE_HOLE, CADENCE_HOLE_MS, CADENCE_STEADY, CADENCE_STOPPED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
CPU = {"engine.device": "cpu"}
HEAD_KEYS = {"totalLines", "stampedLines", "templates", "periodic", "missed", "stopped", "firstTimestamp",
             "lastTimestamp", "top"}
ROW_KEYS = {"signature", "missed", "stopped", "lines", "beats", "backwardBeats", "typicalMs", "regularity", "sumMs",
            "minMs", "maxMs", "fromLine", "toLine", "from", "to", "missedBeats", "overdueMs", "firstLine", "lastLine",
            "lastTimestamp", "intervals", "template", "example"}


# ---- 1. the host twins against a loop

@pytest.mark.parametrize("name", list(scan_cases()))
def test_beat_scan(name):
    assert run_case(name, "cpu") == expected(name)


@pytest.mark.parametrize("name", [n for n, runs in scan_cases().items() if len(runs) > 1])
def test_state_of_split_runs_is_the_state_of_the_joined_run(name):
    split, one = run_case(name, "cpu"), run_runs(joined(name), "cpu")
    assert split[2] == one[2]
    assert sum(split[0], []) == one[0][0] and sum(split[1], []) == one[1][0]


def test_cases_hold_what_they_are_for():
    want = {name: expected(name) for name in scan_cases()}
    col = lambda name, c: [r[c] for r in want[name][2]]
    assert len(want["rows past every link block"][2]) == 30_000 > 100 * K.CDL_ROWS
    assert want["one row per tile, 300 tiles"][2] == [(5, 300, 299, 0, 299 * TILE, TILE, TILE, 0, TILE, 0, 299 * TILE,
                                                        want["one row per tile, 300 tiles"][2][0][11], 1_758_283_200_000,
                                                        1_758_283_200_000 + TILE)]
    assert col("one signature on every line", K.CD_BEATS) == [2 * TILE + 4]
    assert len(want["all signatures distinct"][2]) == 2 * TILE and set(want["all signatures distinct"][0][0]) == {NONE}
    by_sig = {r[0]: r for r in want["borders only; first and last lines of tiles"][2]}
    assert by_sig[1][K.CD_BEATS] == 3 and by_sig[1][K.CD_MIN] == by_sig[1][K.CD_MAX] == 11 * TILE
    assert by_sig[2][K.CD_LINES] == 6 and by_sig[2][K.CD_MIN] == 11 and by_sig[2][K.CD_MAX_TO] == 3 * TILE - 1
    assert sorted(col("a tile without a stamp between", K.CD_MAX)) == [TILE + 1, TILE + 4, TILE + 4]
    assert want["no stamp at all"][2] == [] and set(want["no stamp at all"][1][0]) == {NONE}
    assert col("equal stamps", K.CD_SUM) == [0, 0] and set(want["equal stamps"][1][0]) == {NONE, 0}
    assert col("backward beats", K.CD_BACKWARD) == [201, 199, 199] and col("backward beats", K.CD_BEATS) == [1, 0, 0]
    bkt = want["bucket edges"][1][0]
    assert bkt == [NONE] + [b for k in range(1, 61) for b in (k, k + 1)]
    assert want["widest beat"][0] == [[NONE, NONE, 1 << 62], [0, -(1 << 62)]] and want["widest beat"][1][0][2] == 63
    assert want["equal maxima inside a tile"][2][0][K.CD_MAX_FROM:K.CD_MAX_TO + 1] == (1, 2)
    assert want["equal maxima, one the border beat"][2][0][K.CD_MAX_FROM:K.CD_MAX_TO + 1] == (TILE - 1, TILE)
    assert want["equal maxima, the border beat second"][2][0][K.CD_MAX_FROM:K.CD_MAX_TO + 1] == (3, 5)
    assert col("empty marker as a signature", K.CD_SIG) == [K.GT_EMPTY, 3]
    assert want["cut between the lines of a beat"][0] == [[NONE, 70], [4000, 10]]
    assert set(want["a middle run without a stamp"][0][1]) == {NONE} and len(want["a middle run without a stamp"][0]) == 3
    absent = {r[0]: r for r in want["a template absent from a middle run"][2]}[12345]
    assert absent[K.CD_MAX_FROM] < 1500 and absent[K.CD_MAX_TO] >= 3800
    unstamped = want["skewed mix"][0][0].count(NONE) / len(want["skewed mix"][0][0])
    assert 0.18 < unstamped < 0.25


def test_small_capacity_reruns():
    for name in ("skewed mix", "all signatures distinct", "many small runs"):
        for cap in (0, 1, 7):
            assert run_case(name, "cpu", cap=cap) == expected(name), (name, cap)


def test_beat_scan_arguments():
    one = torch.zeros(1, dtype=torch.int64)
    beat, bkt, state = K.beat_scan(one[:0], one[:0], 5)
    assert beat.numel() == bkt.numel() == 0 and tuple(state.shape) == (K.CD_COLS, 0)
    _, _, state = K.beat_scan(torch.zeros(2, dtype=torch.int64), torch.tensor([4, 2]))
    assert state[K.CD_SIG].tolist() == [2, 4]
    assert K.beat_scan(one[:0], one[:0], 1, state)[2] is state
    for bad in (lambda: K.beat_scan(one.int(), one), lambda: K.beat_scan(one, torch.zeros(2, dtype=torch.int64)),
                lambda: K.beat_scan(one, one.int()), lambda: K.beat_scan(torch.zeros(2, 2, dtype=torch.int64)[:, 0], one),
                lambda: K.beat_scan(one, one, -1), lambda: K.beat_scan(one, one, 1.5), lambda: K.beat_scan(one, one, True),
                lambda: K.beat_scan(one, one, 1, torch.zeros(3, 1, dtype=torch.int64)),
                lambda: K.beat_scan(one, one, 1, state.int()), lambda: K.beat_scan(one, one, 1, state.t().contiguous().t()),
                lambda: K.beat_scan(one, one, 0, state), lambda: K.beat_scan(one, one, 1, state, cap=-1),
                lambda: K.beat_scan(one, one, 1, state, cap=2.0)):
        with pytest.raises(ValueError, match="beat_scan: "):
            bad()


# ---- 2. the report

@pytest.fixture(scope="module")
def cpu():
    return LogParser([], config=Config.load(overrides=CPU))


def _crlf(text: str) -> str:
    return "".join(l + ("\r\n" if i % 3 == 0 else "\n") for i, l in enumerate(text.split("\n")[:-1]))


def test_planted_facts():
    text, known = report_log()
    hole, stopped, steady = known["hole"], known["stopped"], known["steady"]
    rep = golden.cadence(text)
    assert set(rep) == HEAD_KEYS and all(set(r) == ROW_KEYS for r in rep["top"])
    assert (rep["totalLines"], rep["periodic"], rep["missed"], rep["stopped"]) == (4000, 3, 1, 1) and len(rep["top"]) == 2
    assert 0.02 < 1 - rep["stampedLines"] / 4000 < 0.04
    row = rep["top"][0]                     # the planted hole, with its exact numbers
    assert CADENCE_HOLE.split("%d")[0] in row["example"] and row["missed"] and not row["stopped"]
    assert (row["maxMs"], row["fromLine"] - 1, row["toLine"] - 1, row["missedBeats"]) == \
        (hole["maxMs"], hole["fromLine"], hole["toLine"], hole["missedBeats"])
    assert CADENCE_HOLE_MS <= row["maxMs"] < CADENCE_HOLE_MS + 6000 and row["missedBeats"] >= 16
    assert (row["lines"], row["beats"], row["sumMs"], row["typicalMs"]) == (hole["lines"], hole["beats"], hole["sumMs"], hole["typicalMs"])
    assert golden.line_timestamp(row["to"].encode()) - golden.line_timestamp(row["from"].encode()) == row["maxMs"]
    assert sum(c["count"] for c in row["intervals"]) == row["beats"] and row["regularity"] > 0.95
    gone = rep["top"][1]                    # the one that stopped, with its exact last line
    assert CADENCE_STOPPED.split("%d")[0] in gone["example"] and gone["stopped"] and not gone["missed"]
    assert gone["lastLine"] - 1 == stopped["lastLine"] < 11 * 4000 // 20 and gone["missedBeats"] == 0
    assert gone["overdueMs"] == golden.line_timestamp(rep["lastTimestamp"].encode()) - stopped["lastMs"] > 10 * gone["typicalMs"]
    assert [r["signature"] for r in golden.cadence(text, kind="missed")["top"]] == [row["signature"]]
    assert [r["signature"] for r in golden.cadence(text, kind="stopped")["top"]] == [gone["signature"]]
    # the steady one: only under kind="all"; no bulk template is periodic at the defaults
    every = golden.cadence(text, kind="all")["top"]
    assert len(every) == 3 and CADENCE_STEADY.split("%d")[0] in every[2]["example"]
    assert not every[2]["missed"] and not every[2]["stopped"] and every[2]["lastLine"] - 1 == steady["lastLine"]
    loose = golden.cadence(text, kind="all", min_regularity=0, top=None)
    assert loose["periodic"] > 20 and sorted(r["regularity"] for r in loose["top"])[-4] < 0.75


def test_report_matches_golden(cpu):
    text, _ = report_log()
    before = cpu.frequency_statistics()
    for kw, want in zip(parameter_sets(), wanted()):
        assert cpu.cadence(text, **kw) == want, kw
        assert set(want) == HEAD_KEYS and all(set(r) == ROW_KEYS for r in want["top"])
    assert [len(w["top"]) for w in wanted()][:6] == [2, 3, 1, 1, wanted()[4]["periodic"], 7]
    for kw in ({}, {"kind": "all", "min_regularity": 0, "top": None}):
        assert cpu.cadence(_crlf(text), **kw) == golden.cadence(_crlf(text), **kw)
    assert golden.cadence(_crlf(text))["top"][0]["maxMs"] == wanted()[0]["top"][0]["maxMs"]
    assert cpu.frequency_statistics() == before


def test_streams_and_parts_give_the_document_report(cpu, tmp_path):
    text, known = report_log()
    data = text.encode()
    sets, wants = parameter_sets(), wanted()
    lines = text.splitlines(keepends=True)
    cut = len("".join(lines[:(known["hole"]["fromLine"] + known["hole"]["toLine"]) // 2]).encode())    # inside the hole
    res = cpu.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3
    path = tmp_path / "app.log"
    path.write_bytes(data)
    for kw, want in ((sets[k], wants[k]) for k in (0, 1, 4, 7)):
        assert cpu.engine.cadence_bytes(data, **kw) == want and cpu.cadence_file(str(path), **kw) == want, kw
        for c in (4096, 1 << 22):                                                   # ~40-line chunks; one chunk
            assert cpu.cadence_stream(data, chunk_bytes=c, **kw) == want, (kw, c)
        assert cpu.cadence_stream(str(path), chunk_bytes=10_000, **kw) == want, kw
        assert cpu.cadence_resident(res, **kw) == want, kw
        acc = cpu.cadence_accumulator()                                             # one log in two parts
        acc.add_document(data[:cut])
        acc.add_stream(data[cut:], 50000)
        assert acc.report(**kw) == want, kw
        assert acc.report(**sets[3]) == wants[3]                                    # (the parameters belong to the report)
    # one-line chunks: every beat crosses a run border
    head = "".join(lines[:150])
    for kw in ({"kind": "all", "min_regularity": 0, "min_count": 1, "top": None}, {"kind": "all", "min_ms": 1}):
        want = golden.cadence(head, **kw)
        assert want["periodic"] >= 1 and cpu.cadence_stream(head.encode(), chunk_bytes=64, **kw) == want
    assert cpu.cadence_accumulator().report() == dict(golden.cadence(""), totalLines=0, templates=0)      # (nothing added: not even "")


def test_edges(cpu):
    S = "2025-09-19T12:00:%02d "
    logs = {
        "empty": "", "blank": "\n", "no stamp": "a 1\nb 2\na 3\n", "one stamp": "head\n" + S % 5 + "x\n\tat tail\n",
        "two beats": "".join(S % i + "tick %d\n" % i for i in (0, 5, 10)),
        "a hole": "".join(S % i + "tick %d\n" % i + "noise\n" for i in (0, 2, 4, 6, 8, 10, 30, 32, 34)) + S % 59 + "end\n",
        "equal holes": "".join(S % i + "tick\n" for i in (0, 1, 2, 12, 13, 14, 24, 25, 26)),
        "out of order": "".join(S % i + "x\n" for i in (50, 10, 30, 10, 59, 0, 20, 40)),
        "all at once": "".join(S % 7 + "x %d\n" % i for i in range(9)),
        "crlf": "".join((S % i + "x %d\r\n" % i) + ("\tat frame %d\r\n" % i) for i in range(0, 60, 2)),
    }
    for name, text in logs.items():
        for kw in ({"kind": "all", "top": None}, {"min_count": 1, "min_ms": 1, "ratio": 1, "min_regularity": 0, "kind": "all"},
                   {"min_count": 2, "order": "first", "min_regularity": 0.5}):
            want = golden.cadence(text, **kw)
            assert cpu.cadence(text, **kw) == want, (name, kw)
            assert cpu.cadence_stream(text.encode(), chunk_bytes=64, **kw) == want, (name, kw)
            assert set(want) == HEAD_KEYS and want["totalLines"] == len(golden.split_lines(text))
    loose = {"min_count": 2, "min_regularity": 0, "kind": "all"}
    for name in ("empty", "blank", "no stamp", "one stamp"):
        rep = golden.cadence(logs[name], **loose)
        assert (rep["periodic"], rep["top"]) == (0, []) and rep["stampedLines"] == (name == "one stamp")
    assert golden.cadence(logs["no stamp"])["templates"] == 2 and golden.cadence(logs["one stamp"])["lastTimestamp"] is not None
    (row,) = golden.cadence(logs["two beats"], **loose)["top"]
    assert (row["beats"], row["typicalMs"], row["maxMs"], row["regularity"], row["missed"]) == (2, 5000, 5000, 1.0, False)
    rep = golden.cadence(logs["a hole"])
    (row,) = rep["top"]
    assert (row["beats"], row["typicalMs"], row["maxMs"], row["fromLine"], row["toLine"], row["missedBeats"]) == (8, 2000, 20000, 11, 13, 9)
    assert row["missed"] and row["stopped"] and row["overdueMs"] == 25000 and rep["templates"] == 3
    assert golden.cadence(logs["a hole"], ratio=13)["top"] == [] and golden.cadence(logs["a hole"], ratio=13)["periodic"] == 1
    (row,) = golden.cadence(logs["equal holes"], min_regularity=0.5)["top"]
    assert (row["maxMs"], row["fromLine"], row["toLine"], row["typicalMs"], row["missedBeats"]) == (10000, 3, 4, 2285, 3)
    (row,) = golden.cadence(logs["out of order"], min_count=1, min_regularity=0, kind="all")["top"]
    assert (row["beats"], row["backwardBeats"], row["sumMs"], row["minMs"], row["maxMs"]) == (4, 3, 109000, 20000, 49000)
    assert golden.cadence(logs["all at once"], min_regularity=0, kind="all")["top"] == []          # typicalMs 0: not periodic


def test_bad_arguments_raise(cpu):
    log = "2025-09-19T12:00:00 a\n2025-09-19T12:01:00 a\n"
    res = cpu.load_resident(log.encode())
    for kw in ({"min_ms": 0}, {"min_ms": 2.5}, {"min_ms": True}, {"ratio": 0}, {"ratio": 1.5}, {"min_count": 0},
               {"min_count": True}, {"min_regularity": 1.5}, {"min_regularity": -0.1}, {"min_regularity": "0.8"},
               {"min_regularity": float("nan")}, {"kind": "steady"}, {"kind": ""}, {"order": "max"}, {"order": ""},
               {"top": 1.5}, {"top": "3"}):
        calls = [lambda: cpu.cadence(log, **kw), lambda: cpu.cadence_file(os.path.join(ROOT, "no", "such", "file"), **kw),
                 lambda: cpu.cadence_stream(log.encode(), **kw), lambda: cpu.cadence_resident(res, **kw),
                 lambda: cpu.engine.cadence_bytes(log.encode(), **kw), lambda: cpu.cadence_accumulator().report(**kw)]
        if "top" not in kw:
            calls.append(lambda: golden.cadence(log, **kw))
        for call in calls:
            with pytest.raises(ValueError, match="cadence: "):
                call()
    with pytest.raises(ValueError, match="does not have the template"):
        golden.cadence_row(1, 2, 1, 0, 5, 5, 5, 0, 1, 5, 0, 1, 5, [0] * 64, {}, b"a line")
    assert cpu.cadence(log, top=0)["top"] == [] and cpu.cadence(log, top=-1) == golden.cadence(log, top=-1)


def _cli(capsys, *argv, code: int = 0):
    assert main(["cadence", *argv, "--patterns", PAT, "--device", "cpu"]) == code
    out = capsys.readouterr()
    return json.loads(out.out) if code == 0 else out.err


def test_cli(tmp_path, capsys):
    text, _ = report_log()
    log = tmp_path / "app.log"
    log.write_text(text)
    one = _cli(capsys, str(log))
    assert one == wanted()[0] and one["top"][0]["missedBeats"] >= 16
    other = _cli(capsys, str(log), "--stream", "--chunk-bytes", "4096", "--min-ms", "1", "--ratio", "12", "--min-count", "30",
                 "--min-regularity", "0.5", "--kind", "all", "--order", "overdue", "--top", "2")
    assert other == golden.cadence(text, min_ms=1, ratio=12, min_count=30, min_regularity=0.5, kind="all", order="overdue",
                                   top=2) and len(other["top"]) == 2
    assert "min_ms" in _cli(capsys, str(log), "--min-ms", "0", code=2)
