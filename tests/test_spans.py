"""Spans report on the CPU engine (log_parser_amd/spans.py, the host twins of
csrc/kernels/spans.hip): the host twin of ``span_keys`` against ``golden.line_keys`` /
``line_signature`` / ``line_timestamp`` on hand-written and random lines, the report against
``golden.spans`` and against what ``synth.span_log`` plants -- as a document, a stream at chunk
sizes that cut the planted spans, a resident log and an accumulator fed in two and three parts,
every order and filter -- the kinds' usual ends by hand, the sample rule at ``max_ids=16``, the
arguments and the command line.

Mutations that were made, one at a time, and the tests that failed with each (the host twins share
their source with the kernels, so a mutation of span_table.h or of ``span_end_pair`` is one of both):

* spans.hip ``span_fold_host`` takes ``tmin`` from the span's first line and ``tmax`` from its last
  (not min and max): test_start_is_the_smallest_time_not_the_first_lines, test_planted_spans,
  test_unstamped_prefix_and_log_without_stamps, test_small_random_logs,
  test_every_way_gives_the_document_report, 14 of the 15 cases of test_report_equals_golden, and seven
  tests of test_span_table.py (test_last_line_three_folds_after_the_first and
  test_untimed_line_as_the_only_line among them);
* spans.hip ``span_end_pair`` writes ``closes`` only while it is still 0 (a later piece does not
  rewrite it): test_closes_is_rewritten_by_a_later_piece, test_every_way_gives_the_document_report,
  test_sampling, test_small_random_logs, test_token_comes_from_the_first_line, test_cli,
  test_start_is_the_smallest_time_not_the_first_lines (its stream at 64-byte chunks), and six tests
  of test_span_table.py (test_last_line_three_folds_after_the_first among them);
* span_table.h ``span_level`` counts the LOW zero bits of the hash (the sample test on the bits the
  slot uses): test_hand_lines (all three), test_twin_on_random_lines, test_sampling,
  test_small_random_logs, test_cli, and test_fold_purge_fold / test_purge_then_fold_of_a_sibling of
  test_span_table.py;
* spans.hip ``span_end_pair`` cuts the token in the span's LAST line, at that line's own place:
  NOTHING fails, and nothing can -- the key is the hash of the lowered token, so every line of a span
  spells the same lowered bytes (64-bit collisions aside); the mutant is equivalent. What the first
  line decides is WHERE the bytes are read, which the next mutation covers;
* spans.hip ``span_end_pair`` ignores the token's offset (reads at the line's start): 34 of the 42
  tests here and in test_span_table.py, most through the report's own cross-check (the token does not
  hash to the key); test_token_comes_from_the_first_line and every table test that compares bytes;
* spans.py ``count < max_share * total`` instead of ``<=``: test_max_share_boundary,
  test_planted_spans, test_start_is_the_smallest_time_not_the_first_lines,
  test_closes_is_rewritten_by_a_later_piece, test_token_comes_from_the_first_line;
* spans.py never runs the sample rule (``sampleShift`` stays 0): test_sampling, test_small_random_logs
  (its ``max_ids=16`` case), test_cli.
"""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.spans import SpanAccumulator
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import SPAN_HOST, span_log
from spans_cases import SPAN_HAND, sorted_triples, span_index, want_span_keys
from values_cases import index, random_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
CPU = {"engine.device": "cpu"}
KEYS = {"totalLines", "timedLines", "idLines", "pairs", "ids", "listed", "minLength", "maxIds", "sampleShift", "durations",
        "kinds", "top"}
EVERY = {"top": None, "kinds": None, "min_lines": 1, "max_share": 1.0}


@pytest.fixture(scope="module")
def lp():
    return LogParser([], config=Config.load(overrides=CPU))


@pytest.fixture(scope="module")
def planted():
    """The 3,000-line span log behind an unstamped prefix, some of its lines ending in CR LF; its
    default golden report, computed once."""
    text, facts = span_log(3000, seed=1, crlf_rate=0.05)
    text = "starting up on %s\nconfig loaded for %s\n" % (SPAN_HOST, SPAN_HOST) + text
    return text, facts, golden.spans(text)


# ---- the text kernel's host twin

@pytest.mark.parametrize("min_len", [4, 8, 64])
def test_hand_lines(min_len):
    idx = span_index(SPAN_HAND)
    for shift in (0, 1, 3):
        sigs, ts, triples, held, levels = want_span_keys(SPAN_HAND, min_len, shift)
        got_levels = torch.zeros(K.SPAN_LEVELS, dtype=torch.int64)
        sig, stamp, line, key, tok, cnt = K.span_keys(*idx, min_len=min_len, shift=shift, levels=got_levels)
        assert sig.tolist() == sigs and stamp.tolist() == ts, (min_len, shift)
        assert list(zip(line.tolist(), key.tolist(), tok.tolist())) == triples and cnt == (len(triples), held)
        assert got_levels.tolist() == levels and sum(levels) == held
    if min_len == 8:
        per = {i: [(k, p) for j, k, p in want_span_keys(SPAN_HAND)[2] if j == i] for i in range(len(SPAN_HAND))}
        assert per[0] == [(per[0][0][0], 22 | 8 << 10)]                           # ends with the line
        assert per[1][0][1] == 1010 | 14 << 10 and per[2] == []                     # cut at byte 1,024
        assert per[3][0][1] == 8 | 15 << 10                                         # straddles a block
        assert len(per[4]) == 8 and len(per[5]) == 1 and per[5][0][1] == 4 | 8 << 10
        assert [p >> 10 for _, p in per[6]] == [64] and per[7] == per[9] == per[10] == []
        assert len(per[8]) == 1 and len(per[13]) == 1 and per[13][0][0] == per[0][0][0]
        assert K.span_keys(*idx)[1].tolist()[10] == golden.line_timestamp(SPAN_HAND[10]) is not None


def test_twin_on_random_lines():
    lines = random_lines(400, seed=3)
    for shift_bytes in (0, 1, 15):
        idx = index(lines, shift_bytes)
        for min_len, shift in ((8, 0), (4, 2), (16, 1)):
            sigs, ts, triples, held, levels = want_span_keys(lines, min_len, shift)
            sig, stamp, line, key, tok, cnt = K.span_keys(*idx, min_len=min_len, shift=shift)
            assert sig.tolist() == sigs and stamp.tolist() == ts and cnt == (len(triples), held) and held > 0
            assert list(zip(line.tolist(), key.tolist(), tok.tolist())) == triples
            for cap in (0, len(triples) - 1, len(triples)):                         # the re-run protocol
                again = K.span_keys(*idx, min_len=min_len, shift=shift, cap=cap)
                assert sorted_triples(*again[2:5]) == sorted(triples) and again[5] == cnt
    lsig, lts = K.line_stamps(*index(lines, 0))
    sig, stamp = K.span_keys(*index(lines, 0))[:2]
    assert torch.equal(sig, lsig) and torch.equal(stamp, lts)


def test_span_keys_arguments():
    idx = span_index([b"rid=abc12345"])
    for kw in ({"min_len": 3}, {"min_len": 65}, {"shift": -1}, {"shift": 65}, {"per_block": 4096},
               {"levels": torch.zeros(3, dtype=torch.int64)}):
        with pytest.raises(ValueError):
            K.span_keys(*idx, **kw)
    none = K.span_keys(idx[0], idx[1][:0], idx[2][:0])
    assert [t.numel() for t in none[:5]] == [0] * 5 and none[5] == (0, 0)


# ---- the report

PARAMS = [{}, {"order": "lines", "top": 7}, {"order": "first", "top": None}, {"unfinished_only": True},
          {"min_ms": 300}, {"min_ms": 300, "unfinished_only": True, "order": "lines"}, {"min_lines": 5, "kinds": 1},
          {"max_share": 1.0, "min_lines": 1}, {"max_share": 0.001}, {"top": 0}, {"top": 1, "kinds": 0},
          {"kind_min_spans": 300}, {"close_share": 1.0}, {"min_len": 4, "top": 5}, {"min_len": 11}]


@pytest.mark.parametrize("kw", PARAMS, ids=[json.dumps(p) for p in PARAMS])
def test_report_equals_golden(lp, planted, kw):
    text = planted[0]
    got = lp.spans(text, **kw)
    assert got == golden.spans(text, **kw) and set(got) == KEYS and got["totalLines"] == 3002
    if kw.get("top", 20) is not None:
        assert len(got["top"]) <= kw.get("top", 20)


def test_planted_spans(lp, planted):
    text, facts, want = planted
    got = lp.spans(text)
    assert got == want and got["timedLines"] < got["totalLines"] and got["ids"] == facts["ids"] + 1
    assert got["listed"] == facts["ids"]                                            # the host token is on every line
    assert got["top"][0]["key"] == facts["long"] and got["top"][0]["durationMs"] > 3 * got["top"][1]["durationMs"]
    assert not got["top"][0]["unfinished"] and got["top"][0]["closes"] == got["top"][0]["usualEnd"]
    assert all(r["key"] != SPAN_HOST for r in lp.spans(text, top=None)["top"])
    assert any(r["key"] == SPAN_HOST for r in lp.spans(text, top=None, max_share=1.0)["top"])
    kind = got["kinds"][0]                                                          # the kind with the unfinished span first
    assert kind["unfinished"] == 1 and "request" in kind["template"] and kind["usualEnd"] is not None
    assert [k["unfinished"] for k in got["kinds"][1:]] == [0, 0] and len(got["kinds"]) == facts["kinds"]
    only = lp.spans(text, unfinished_only=True)["top"]
    assert [r["key"] for r in only] == [facts["unfinished"]] and only[0]["unfinished"]
    assert only[0]["opens"] == kind["opens"] and only[0]["closes"] != only[0]["usualEnd"] == kind["usualEnd"]
    assert "completed" in [c for c in kind["closes"] if c["signature"] == kind["usualEnd"]][0]["template"]
    assert sum(d["count"] for d in got["durations"]) == got["listed"]
    assert kind["maxKey"] == facts["long"] and kind["maxMs"] == got["top"][0]["durationMs"]


def test_start_is_the_smallest_time_not_the_first_lines():
    """Out-of-order stamps: ``start`` / ``end`` are min and max over the span's lines."""
    log = ("2025-09-19T12:00:10Z begin rid=abc12345\n"
           "2025-09-19T12:00:05Z work rid=abc12345\n"            # a stamp in the past
           "   continued rid=abc12345\n"                         # unstamped: the time of the line before
           "2025-09-19T12:00:30Z work rid=abc12345\n"
           "2025-09-19T12:00:20Z end rid=abc12345\n")
    lp = LogParser([], config=Config.load(overrides=CPU))
    got = lp.spans(log, max_share=1.0)
    assert got == golden.spans(log, max_share=1.0)
    row = got["top"][0]
    assert (row["start"], row["end"], row["durationMs"]) == ("2025-09-19T12:00:05.000Z", "2025-09-19T12:00:30.000Z", 25000)
    assert row["lines"] == 5 and (row["firstLine"], row["lastLine"]) == (1, 5)
    for cb in (64, 100):
        assert lp.spans_stream(log.encode(), cb, max_share=1.0) == got


def test_unstamped_prefix_and_log_without_stamps(lp):
    body = "".join("step %d for job1234567\n" % i for i in range(6))
    log = body + "2025-09-19T12:00:00Z late stamp job1234567 and req7654321\nmore req7654321\n"
    got = lp.spans(log, max_share=1.0)
    assert got == golden.spans(log, max_share=1.0) and got["timedLines"] == 2
    rows = {r["key"]: r for r in got["top"]}
    assert rows["job1234567"]["durationMs"] == 0 == rows["req7654321"]["durationMs"] and rows["job1234567"]["lines"] == 7
    # no stamp at all: every duration is null, and min_ms = 1 lists nothing
    none = lp.spans(body + "x job1234567 req7654321\ny req7654321\n", max_share=1.0)
    assert none == golden.spans(body + "x job1234567 req7654321\ny req7654321\n", max_share=1.0)
    assert none["timedLines"] == 0 and [r["durationMs"] for r in none["top"]] == [None, None] and none["durations"] == []
    assert [r["start"] for r in none["top"]] == [None, None] and none["kinds"][0]["maxMs"] is None
    empty = lp.spans(body, max_share=1.0, min_ms=1)
    assert empty == golden.spans(body, max_share=1.0, min_ms=1) and empty["listed"] == 0 and empty["ids"] == 1
    assert lp.spans("") == golden.spans("") and lp.spans("no id here\n")["ids"] == 0


def _kind_log(closes, opening="opened session"):
    """One kind: span i opens on ``opening`` and closes on the template ``closes[i]``."""
    out = []
    for i, c in enumerate(closes):
        sid = "%s%07d" % (opening[:2], i)
        out += ["2025-09-19T12:00:%02dZ %s %s" % (i, opening, sid), "2025-09-19T12:00:%02dZ %s %s" % (i + 1, c, sid)]
    return out


def test_usual_end_by_hand(lp):
    x, y = "closed fine", "gave up on"
    sx, sy = (golden.line_signature(("2025-09-19T12:00:00Z %s ab0000001" % c).encode()) for c in (x, y))
    # a tie of closing templates: the smaller unsigned signature wins
    tie = "\n".join(_kind_log([x, y, x, y, x, y])) + "\n"
    got = lp.spans(tie, close_share=0.5, max_share=1.0)
    assert got == golden.spans(tie, close_share=0.5, max_share=1.0)
    assert got["kinds"][0]["usualEnd"] == "%016x" % min(sx, sy) and got["kinds"][0]["unfinished"] == 3
    assert lp.spans(tie, close_share=0.51, max_share=1.0)["kinds"][0]["usualEnd"] is None
    # a share of exactly close_share passes: 4 of 5 at 0.8
    exact = "\n".join(_kind_log([x, x, y, x, x])) + "\n"
    got = lp.spans(exact, max_share=1.0)
    assert got == golden.spans(exact, max_share=1.0) and got["kinds"][0]["usualEnd"] == "%016x" % sx
    assert [r["key"] for r in got["top"] if r["unfinished"]] == ["op0000002"] and got["kinds"][0]["unfinished"] == 1
    assert lp.spans(exact, max_share=1.0, close_share=0.81)["kinds"][0]["usualEnd"] is None
    # kind_min_spans - 1 spans: no usual end, nothing unfinished
    few = "\n".join(_kind_log([x, x, x, y])) + "\n"
    got = lp.spans(few, max_share=1.0, close_share=0.7)
    assert got == golden.spans(few, max_share=1.0, close_share=0.7)
    assert got["kinds"][0]["usualEnd"] is None and not any(r["unfinished"] or "usualEnd" in r for r in got["top"])
    assert lp.spans(few, max_share=1.0, close_share=0.7, kind_min_spans=4)["kinds"][0]["usualEnd"] == "%016x" % sx
    # two kinds: the one with unfinished spans comes first although the other is larger
    both = "\n".join(_kind_log([x] * 9, "started batch") + _kind_log([x, x, x, x, y, x])) + "\n"
    got = lp.spans(both, max_share=1.0)
    assert got == golden.spans(both, max_share=1.0)
    assert [(k["spans"], k["unfinished"]) for k in got["kinds"]] == [(6, 1), (9, 0)]


def test_max_share_boundary(lp):
    """``lines <= max_share * totalLines``: an id on exactly that many lines stays."""
    log = "a rid=abc12345\nb rid=abc12345\n" + "filler line\n" * 6
    for share, listed in ((0.25, 1), (0.2499, 0), (0.26, 1)):
        got = lp.spans(log, max_share=share)
        assert got == golden.spans(log, max_share=share) and got["listed"] == listed and got["ids"] == 1, share
    assert lp.spans(log, min_lines=3)["listed"] == 0 and lp.spans(log, min_lines=2)["listed"] == 1


def test_small_random_logs(lp):
    for seed in range(6):
        rng = random.Random(seed)
        lines = [x.decode("latin-1") for x in random_lines(rng.randrange(5, 120), seed)]
        log = ("\r\n" if seed % 2 else "\n").join(lines) + "\n"
        for kw in (EVERY, dict(EVERY, order="lines", min_len=4), dict(EVERY, order="first", max_ids=16),
                   {"min_lines": 2, "max_share": 0.5, "kind_min_spans": 2, "close_share": 0.5, "top": 3}):
            got = lp.spans(log, **kw)
            assert got == golden.spans(log, **kw), (seed, kw)
            assert got == lp.spans_stream(log.encode("latin-1").decode("latin-1").encode(), 256, **kw), (seed, kw)


# ---- chunk independence and the sample rule

def _ways(lp, text, **kw):
    """The report of ``text`` as a document, as a stream at chunk sizes that cut the planted spans,
    as a resident log and from an accumulator fed in two and in three parts."""
    data = text.encode()
    acc_kw = {k: kw[k] for k in ("min_len", "max_ids") if k in kw}
    rep_kw = {k: v for k, v in kw.items() if k not in acc_kw}
    yield "document", lp.spans(text, **kw)
    for c in (4096, 30000, 1 << 20):
        yield "stream %d" % c, lp.spans_stream(data, chunk_bytes=c, **kw)
    res = lp.load_resident(data, chunk_bytes=16384)
    assert len(res.chunks) > 3
    yield "resident", lp.spans_resident(res, **kw)
    cut = [data.index(b"\n", len(data) * k // 3) + 1 for k in (1, 2)]
    two = lp.span_accumulator(**acc_kw)
    two.add_document(data[:cut[1]])
    two.add_stream(data[cut[1]:], 50000)
    yield "two parts", two.report(**rep_kw)
    three = lp.span_accumulator(**acc_kw)
    three.add_document(data[:cut[0]])
    three.add_document(data[cut[0]:cut[1]])
    three.add_stream(data[cut[1]:], 8192)
    yield "three parts", three.report(**rep_kw)


def test_every_way_gives_the_document_report(lp, planted):
    text, facts, want = planted
    # (the long span's first line is in the first third, its last in the last: the three-part case
    # puts an id's last line in a later part than its first)
    long_row = want["top"][0]
    assert long_row["firstLine"] < 3002 // 3 and long_row["lastLine"] > 2 * 3002 // 3
    for name, got in _ways(lp, text):
        assert got == want, name
    kw = {"order": "lines", "top": None, "kinds": None, "min_ms": 10, "unfinished_only": False}
    want = golden.spans(text, **kw)
    for name, got in _ways(lp, text, **kw):
        assert got == want, name


def test_closes_is_rewritten_by_a_later_piece(lp):
    """The two-fold ``closes`` test at the level of the report."""
    a = "2025-09-19T12:00:00Z opened rid=abc12345\n2025-09-19T12:00:01Z working on rid=abc12345\n"
    b = "2025-09-19T12:00:02Z still working on rid=abc12345 now\n2025-09-19T12:00:09Z closed rid=abc12345 ok\n"
    acc = lp.span_accumulator()
    acc.add_document(a)
    first = acc.report(max_share=1.0)
    acc.add_document(b)
    got = acc.report(max_share=1.0)
    assert got == golden.spans(a + b, max_share=1.0) and first == golden.spans(a, max_share=1.0)
    assert first["top"][0]["closesExample"].endswith("working on rid=abc12345")
    assert got["top"][0]["closesExample"].endswith("closed rid=abc12345 ok") and got["top"][0]["durationMs"] == 9000
    assert got["top"][0]["opens"] == first["top"][0]["opens"] and got["top"][0]["key"] == "abc12345"


def test_token_comes_from_the_first_line(lp):
    log = "open RID=ABC12345x\nwork rid=abc12345X\nclose Rid=Abc12345X done\n"
    got = lp.spans(log, max_share=1.0)
    assert got == golden.spans(log, max_share=1.0) and got["top"][0]["key"] == "abc12345x" and got["top"][0]["lines"] == 3
    # the places differ from line to line: the bytes are cut from the first line's place
    acc = lp.span_accumulator()
    acc.add_document("  open   RID=ABC12345x\n")
    acc.add_document("rid=abc12345X and a long tail that moves nothing\n")
    assert acc.report(max_share=1.0) == golden.spans("  open   RID=ABC12345x\nrid=abc12345X and a long tail that moves nothing\n",
                                                     max_share=1.0)


SAMPLE_SEED = 2


@pytest.fixture(scope="module")
def sampled():
    """A log of about 200 ids whose golden report at ``max_ids=16`` holds between 4 and 16 ids: the
    cap is not met by an empty sample (the seed was picked on the CPU for that)."""
    text, facts = span_log(1000, seed=SAMPLE_SEED)
    want = golden.spans(text, max_ids=16, top=None, kinds=None)
    assert 150 <= facts["ids"] <= 260 and 4 <= want["ids"] <= 16 and want["sampleShift"] > 0
    return text, facts, want


def test_sampling(lp, sampled):
    text, facts, want = sampled
    kw = {"max_ids": 16, "top": None, "kinds": None}
    for name, got in _ways(lp, text, **kw):
        assert got == want, name
    assert want["pairs"] == sum(r["lines"] for r in lp.spans(text, max_ids=16, top=None, min_lines=1, max_share=1.0)["top"])
    assert 0 < want["idLines"] < want["totalLines"] and want["maxIds"] == 16
    # the smallest shift whose sample fits: one less holds more than 16 ids
    levels = [golden.span_level(k) for k in {k for x in text.encode().split(b"\n") for k in golden.line_keys(x)}]
    s = want["sampleShift"]
    assert sum(v >= s for v in levels) == want["ids"] and sum(v >= s - 1 for v in levels) > 16
    # between the pieces the table never holds more than max_ids
    acc = SpanAccumulator(lp.engine, max_ids=16)
    for part in text.encode().split(b"\n2025-09-19T12:00:03")[:2]:
        acc.add_document(part + b"\n")
        assert acc.table.used <= 16
    # a max_ids above the id count: shift 0, the exact report
    full = lp.spans(text, max_ids=1024, top=None)
    assert full == golden.spans(text, max_ids=1024, top=None) == dict(golden.spans(text, top=None), maxIds=1024)
    assert full["sampleShift"] == 0 and full["ids"] == facts["ids"] + 1


# ---- arguments and the command line

def test_arguments(lp):
    for kw in ({"min_len": 3}, {"min_len": 65}, {"max_ids": 15}, {"max_ids": (1 << 26) + 1}, {"max_ids": 16.0},
               {"order": "size"}, {"min_lines": 0}, {"max_share": 0.0}, {"max_share": 1.5}, {"min_ms": -1},
               {"kind_min_spans": 0}, {"close_share": 0}, {"close_share": 1.1}, {"top": 2.5}, {"kinds": "all"}):
        for call in (lambda: lp.spans("x\n", **kw), lambda: golden.spans("x\n", **kw),
                     lambda: lp.spans_stream(b"x\n", None, **kw), lambda: lp.spans_file(os.devnull, **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        lp.span_accumulator(max_ids=3)
    assert golden.spans_check_args(close_share=0.8) == golden.Fraction(4, 5)


def _cli(*argv, code: int = 0):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "spans", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == code, r.stderr
    return json.loads(r.stdout) if code == 0 else r.stderr


def test_cli(tmp_path):
    text, facts = span_log(600, seed=4)
    log = tmp_path / "app.log"
    log.write_text(text)
    one = _cli(str(log))
    assert one == golden.spans(text) and set(one) == KEYS and one["totalLines"] == 600
    assert one["top"][0]["key"] == facts["long"] and one["kinds"][0]["unfinished"] == 1
    other = _cli(str(log), "--stream", "--chunk-bytes", "4096", "--min-length", "6", "--min-lines", "3", "--max-share", "0.5",
                 "--min-ms", "20", "--order", "lines", "--unfinished-only", "--max-ids", "64", "--top", "3", "--kinds", "2")
    assert other == golden.spans(text, min_len=6, min_lines=3, max_share=0.5, min_ms=20, order="lines", unfinished_only=True,
                                 max_ids=64, top=3, kinds=2)
    assert other["sampleShift"] > 0 and len(other["kinds"]) == 2
    # several files continue ONE log
    keep = text.splitlines(keepends=True)
    a, b = tmp_path / "a.log", tmp_path / "b.log"
    a.write_text("".join(keep[:250]))
    b.write_text("".join(keep[250:]))
    assert _cli(str(a), str(b)) == one == _cli(str(a), str(b), "--stream")
    assert "min_len" in _cli(str(log), "--min-length", "2", code=2)
    assert "max_ids" in _cli(str(log), "--max-ids", "1", code=2)
