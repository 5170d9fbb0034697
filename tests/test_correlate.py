"""Correlation report on the CPU engine (log_parser_amd/correlate.py, csrc/kernels/correlate.hip host
twin): the key rule of ``golden.line_keys`` on hand-written lines, the host twin against it pair
for pair in its three forms (plain, ``sel``, ``table``), the report against ``golden.correlate`` and
against what ``synth.correlated_log`` knows by construction, for documents, streams in chunks of
any size and resident logs, edge logs, arguments and the command line."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.pieces import stream_lines, stream_pieces
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import CORRELATED_FAIL, correlated_log, log_templates, templated_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
KEYS = {"totalLines", "events", "eventLines", "minLength", "keys", "keyLines", "top"}
ROW_KEYS = {"key", "eventLines", "lines", "share", "firstLine", "lastLine", "firstEventLine", "signature", "example"}
CPU = {"engine.device": "cpu"}
H = golden.fnv1a64


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


# ---- 1. the key rule, by hand

STAMPS = [b"2025-09-19T12:01:02.003Z INFO ready", b"2025-09-19 12:01:02,003 INFO ready", b"Sep 19 12:01:02 host1 app[4321]: ready",
          b"E0919 12:01:02.000345    4321 file.go:27] ready", b"[12345.678901] usb 1-1: ready"]


def test_key_rule_lengths_and_digits():
    for m in (4, 8, 13, 64):
        short, exact = b"a" * (m - 2) + b"7", b"a" * (m - 1) + b"7"
        assert golden.line_keys(b"x " + short + b" y", m) == []                     # min_len - 1 bytes
        assert golden.line_keys(b"x " + exact + b" y", m) == [H(exact)]             # min_len bytes
    t64, t65 = b"9" + b"b" * 63, b"9" + b"b" * 64
    assert golden.line_keys(b"blob " + t64 + b".") == [H(t64)] and golden.line_keys(b"blob " + t65 + b".") == []
    assert golden.line_keys(b"blob " + t64, 64) == [H(t64)]
    assert golden.line_keys(b"level abcdefghijklmnopqrstuvwxyz reached") == []      # a long token without a digit
    assert golden.line_keys(b"a1b2c3d4e5 middle f6g7h8i9j0") == [H(b"a1b2c3d4e5"), H(b"f6g7h8i9j0")]   # at byte 0, at the end
    assert golden.line_keys(b"") == [] and golden.line_keys(b"12345678") == [H(b"12345678")]
    assert golden.line_keys(b"caf\xc3\xa9abcd1234\xff\x80 \x80zz99zz99") == [H(b"abcd1234"), H(b"zz99zz99")]
    assert golden.line_keys(b"ab-12345678_9 1234_5678") == [H(b"12345678")]         # - and _ end a token


def test_key_rule_case_and_repeats():
    assert golden.line_keys(b"rid=ABCDEF0123 again rid=abcdef0123 and AbCdEf0123.") == [H(b"abcdef0123")]
    assert golden.line_key_tokens(b"Rid=ABCDEF0123") == [(H(b"abcdef0123"), b"abcdef0123")]
    ids = [b"id%06dxx" % i for i in range(20)]
    for n in (0, 1, 8, 9, 20):
        line = b"k " + b" ".join(ids[:n]) + b" end"
        assert golden.line_keys(line) == [H(x) for x in ids[:min(n, 8)]], n
    # a repeat does not use up a slot: the ninth DISTINCT key is the one ignored
    line = b" ".join(ids[:4] + ids[:4] + ids[4:8] + ids[:2] + ids[8:10])
    assert golden.line_keys(line) == [H(x) for x in ids[:8]]


def test_key_rule_cut_at_1024():
    tok = b"abcdefgh12345678"
    cut10 = b"x" * 1013 + b" " + tok            # 10 bytes of the token lie before byte 1024: "abcdefgh12"
    cut8 = b"x" * 1015 + b" " + tok             # 8 bytes: "abcdefgh", no digit
    cut5 = b"x" * 1018 + b" " + b"1" + tok      # 5 bytes: too short
    past = b"x" * 1023 + b" " + tok             # starts at byte 1024
    assert golden.line_keys(cut10) == [H(b"abcdefgh12")] and golden.line_keys(cut10 + b" tail9999") == [H(b"abcdefgh12")]
    assert golden.line_keys(cut8) == [] and golden.line_keys(cut5) == [] and golden.line_keys(past) == []
    long = b"7" + b"c" * 70                     # a 71-byte run that the cut shortens to 60: a blob stays a key there
    assert golden.line_keys(b"x" * 963 + b" " + long) == [H(long[:60])]
    assert golden.line_keys(b"y " + long) == []


def test_key_rule_on_real_shapes():
    for s in STAMPS:
        assert golden.line_keys(s) == [], s
    assert golden.line_keys(b"req 123e4567-e89b-12d3-a456-426614174000 done") == [H(b"123e4567"), H(b"426614174000")]
    assert golden.line_keys(b"traceId=4BF92F3577B34DA6A3CE929D0E0E4736 ok") == [H(b"4bf92f3577b34da6a3ce929d0e0e4736")]
    assert golden.line_keys(b"spanId=00f067aa0ba902b7") == [H(b"00f067aa0ba902b7")]
    assert [t for _, t in golden.line_key_tokens(b"pod web-7d4b9c6f5d-x2x9z evicted")] == [b"7d4b9c6f5d"]
    assert [t for _, t in golden.line_key_tokens(b"at 1758283262003 ptr 0x7ffdeadbeef0 since 20250919T120102Z")] == \
        [b"1758283262003", b"0x7ffdeadbeef0", b"20250919t120102z"]
    # the fields of synth.log_templates stay below 8 bytes, but for a "%dms" with six or seven digits
    toks = [t for line in templated_log(3000, log_templates(60, seed=1), seed=2).split("\n")
            for _, t in golden.line_key_tokens(line.encode())]
    assert 0 < len(toks) < 3000 and all(t.endswith(b"ms") and t[:-2].isdigit() and len(t) in (8, 9) for t in toks)


# ---- 2. the host twin against the rule, pair for pair

HAND = [b"x abcdef7 y", b"x abcdefg7 y", b"blob 9" + b"b" * 63 + b".", b"blob 9" + b"b" * 64 + b".",
        b"level abcdefghijklmnopqrstuvwxyz reached", b"a1b2c3d4e5 middle f6g7h8i9j0", b"", b"12345678",
        b"caf\xc3\xa9abcd1234\xff\x80 \x80zz99zz99", b"rid=ABCDEF0123 again rid=abcdef0123 and AbCdEf0123.",
        b"x" * 1013 + b" abcdefgh12345678", b"x" * 1015 + b" abcdefgh12345678", b"x" * 1018 + b" 1abcdefgh12345678",
        b"x" * 1023 + b" abcdefgh12345678", b"x" * 963 + b" 7" + b"c" * 70, b"y 7" + b"c" * 70,
        b"x" * 1013 + b" abcdefgh12345678 tail9999 " + b"z" * 3000] + STAMPS + \
       [b"k " + b" ".join(b"id%06dxx" % i for i in range(n)) + b" end" for n in (1, 8, 9, 20)] + \
       [b" ".join([b"id%06dxx" % i for i in (0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 8, 9)]),
        b"req 123e4567-e89b-12d3-a456-426614174000 done", b"last line ends with a key rid=00f067aa0ba902b7"]


def _random_lines(n: int, seed: int):
    """Lines of words, numbers and ids from a pool of 40 (in either letter case, some twice on a
    line, some lines with more than eight), blank and long ones among them; the last is not empty."""
    rng = random.Random(seed)
    pool = [("%016x" % rng.getrandbits(64)).encode() for _ in range(30)] + [b"node%05d" % i for i in range(10)]
    out = []
    for _ in range(n):
        words = [rng.choice([b"INFO", b"served", b"in", b"%dms" % rng.randrange(999), b"0x%x" % rng.getrandbits(rng.choice((16, 40))),
                             b"id=%d" % rng.randrange(1 << rng.choice((10, 40)))]) for _ in range(rng.randrange(0, 9))]
        for _ in range(rng.choice((0, 0, 1, 1, 2, 3, 12))):
            x = rng.choice(pool)
            words.insert(rng.randrange(len(words) + 1), rng.choice((b"rid=", b"", b"[")) + rng.choice((x, x.upper())))
        line = rng.choice((b" ", b"\t", b" - ")).join(words)
        out.append(line * rng.choice((1, 1, 1, 30)))
    return out + [b"done"], pool


def _stage(lines):
    data = b"\n".join(lines)
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    ls, ll = K.split_lines(text, len(data))
    assert ls.numel() == len(lines)
    return text, ls, ll


def _want(lines, sel=None, table=None, min_len=8):
    items = range(len(lines)) if sel is None else sel
    per = [[k for k in golden.line_keys(lines[x], min_len) if table is None or k in table] for x in items]
    return [(x, _signed(k)) for x, ks in zip(items, per) for k in ks], [int(bool(ks)) for ks in per]


def _check_twin(lines, idx, sel=None, table=None, tab=None, min_len=8):
    pairs, hit = _want(lines, sel, table, min_len)
    s = None if sel is None else torch.tensor(sel, dtype=torch.int32)
    for cap in (None, len(pairs), max(0, len(pairs) - 1), 1, 0):                    # cap below the count: the re-run
        line, key, h, (m, held) = K.line_keys(*idx, sel=s, table=tab, min_len=min_len, cap=cap)
        assert line.dtype == torch.int32 and key.dtype == torch.int64 and h.dtype == torch.uint8
        assert list(zip(line.tolist(), key.tolist())) == pairs                      # (the twin appends in item order)
        assert h.tolist() == hit and m == len(pairs) and held == sum(hit)
    return pairs


@pytest.mark.parametrize("which", ["hand", "random"])
def test_host_twin_matches_golden(which):
    lines, pool = (HAND, [b"id%06dxx" % i for i in range(20)]) if which == "hand" else _random_lines(700, 11)
    idx = _stage(lines)
    L = len(lines)
    rng = random.Random(5)
    for min_len in (8, 4, 9, 16, 64):
        assert len(_check_twin(lines, idx, min_len=min_len)) > (0 if min_len <= 16 else -1)
    for sel in ([], [0], [L - 1], [L - 1, 0, 3, 3, 3], sorted(rng.sample(range(L), L // 3)), list(range(L))[::-1]):
        _check_twin(lines, idx, sel=sel)
    # tables: the ids of half the pool plus keys no line holds; one at most half full, and two with a
    # capacity of their own -- nearly full and full, so that a probe runs around the end of the table
    held = {H(x.lower()) for x in pool[::2]}
    for n, cap in ((len(held) + 5, None), (40, 64), (31, 32), (32, 32)):
        keys = (sorted(held) + [H(b"absent%d" % i) for i in range(n)])[:n]
        tab = K.GapTable.from_signatures("cpu", torch.tensor([_signed(k) for k in keys], dtype=torch.int64), cap=cap)
        assert tab.cap == (cap or 4096) and held <= set(keys)
        got = _check_twin(lines, idx, table=set(keys), tab=tab)
        assert 0 < len(got) < len(_want(lines)[0])
        _check_twin(lines, idx, sel=sorted(rng.sample(range(L), L // 2)), table=set(keys), tab=tab, min_len=10)
    empty = K.GapTable("cpu")
    assert _check_twin(lines, idx, table=set(), tab=empty) == []


def test_line_keys_arguments():
    text, ls, ll = _stage([b"rid=abcdef0123", b"x"])
    none = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int32)
    line, key, hit, cnt = K.line_keys(text, *none)
    assert (line.numel(), key.numel(), hit.numel(), cnt) == (0, 0, 0, (0, 0))
    line, key, hit, cnt = K.line_keys(text, ls, ll, sel=torch.empty(0, dtype=torch.int32))
    assert (line.numel(), key.numel(), hit.numel(), cnt) == (0, 0, 0, (0, 0))
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)                             # noqa: E731
    for bad in (lambda: K.line_keys(text, ls, ll, min_len=3), lambda: K.line_keys(text, ls, ll, min_len=65),
                lambda: K.line_keys(text, ls, ll, sel=torch.tensor([0])), lambda: K.line_keys(text, ls, ll, sel=i32(2)),
                lambda: K.line_keys(text, ls, ll, sel=i32(-1)), lambda: K.line_keys(text, ls, ll, sel=i32(0, 1, 0, 1)[::2]),
                lambda: K.line_keys(text, *none, sel=i32(0)), lambda: K.line_keys(text, ls, ll, per_block=4096)):
        with pytest.raises(ValueError):
            bad()


# ---- 3. the report: a log of interleaved requests, some of which fail

def _library():
    return [PatternSet.model_validate({"metadata": {"library_id": "correlate"}, "patterns": [
        {"id": "aborted", "name": "request aborted", "severity": "HIGH",
         "primary_pattern": {"regex": r"request aborted:", "confidence": 0.9},
         "context_extraction": {"lines_before": 2, "lines_after": 1}}]})]


@pytest.fixture(scope="module")
def case():
    """(CPU parser, a log of 3000 lines and 120 requests, the failing ids and their lines)."""
    lp = LogParser(_library(), config=Config.load(overrides=CPU))
    log, failing = correlated_log(3000, log_templates(40, seed=5), 120, seed=7, crlf_rate=0.1)
    assert CORRELATED_FAIL in log and 15 < len(failing) < 60
    return lp, log, failing


def _golden(lp, log, **kw):
    return golden.correlate(log, _library(), lp.config.scoring, **kw)


def test_synthetic_log_is_what_it_says(case):
    _, log, failing = case
    lines = log.replace("\r\n", "\n").split("\n")
    assert len(lines) == 3001 and lines[-1] == ""
    with_id = [x for x in lines if " rid=" in x]
    assert len(with_id) > 2500 and len({x[-16:] for x in with_id}) > 100
    for rid, at in failing.items():
        assert at == [i for i, x in enumerate(lines) if x.endswith(" rid=" + rid)] and len(at) >= 2
        assert [i for i in at if CORRELATED_FAIL in lines[i]] == [at[-1]]
    assert sum(CORRELATED_FAIL in x for x in lines) == len(failing)
    spans = sorted((at[0], at[-1]) for at in failing.values())
    assert any(a2 < b1 for (_, b1), (a2, _) in zip(spans, spans[1:]))              # failing requests overlap: interleaved
    assert correlated_log(500, log_templates(10), 30, seed=3) == correlated_log(500, log_templates(10), 30, seed=3)


@pytest.mark.parametrize("order", ["events", "lines", "first"])
def test_report_equals_golden_and_construction(case, order):
    lp, log, failing = case
    want = _golden(lp, log, top=None, order=order)
    got = lp.correlate(log, top=None, order=order)
    assert got == want and set(got) == KEYS and all(set(r) == ROW_KEYS for r in got["top"])
    assert got["totalLines"] == 3000 and got["events"] == got["eventLines"] == got["keys"] == len(failing)
    assert got["minLength"] == 8 and got["keyLines"] == sum(len(at) for at in failing.values())
    # every failing id, with exactly its lines; no filter removed one
    assert len(got["top"]) == len(failing) and {r["key"] for r in got["top"]} == set(failing)
    lines = log.replace("\r\n", "\n").split("\n")
    for r in got["top"]:
        at = failing[r["key"]]
        assert (r["lines"], r["eventLines"], r["firstLine"], r["lastLine"], r["firstEventLine"]) == \
            (len(at), 1, at[0] + 1, at[-1] + 1, at[-1] + 1)
        assert r["share"] == 1 / len(at) and r["example"] == lines[at[0]]
        assert r["signature"] == "%016x" % H(r["key"].encode())
    key = {"events": lambda r: (-r["eventLines"], -r["lines"], r["firstLine"], int(r["signature"], 16)),
           "lines": lambda r: (-r["lines"], -r["eventLines"], r["firstLine"], int(r["signature"], 16)),
           "first": lambda r: (r["firstEventLine"], int(r["signature"], 16))}[order]
    assert got["top"] == sorted(got["top"], key=key)
    assert lp.correlate(log, order=order) == _golden(lp, log, order=order) and len(lp.correlate(log, order=order)["top"]) == 20
    assert lp.correlate(log, top=3, order=order)["top"] == want["top"][:3] and lp.correlate(log, top=0, order=order)["top"] == []


@pytest.mark.parametrize("kw", [{"min_len": 4}, {"min_len": 16}, {"min_len": 17}, {"min_lines": 1}, {"min_lines": 12},
                                {"max_share": 0.004}, {"max_share": 1.0}, {"min_len": 5, "min_lines": 3, "max_share": 0.01}])
def test_report_parameters(case, kw):
    lp, log, failing = case
    for order in ("events", "lines", "first"):
        want = _golden(lp, log, top=None, order=order, **kw)
        assert lp.correlate(log, top=None, order=order, **kw) == want
    n = [len(at) for at in failing.values()]
    if kw == {"min_len": 17}:
        assert want["keys"] == 0 and want["keyLines"] == 0 and want["top"] == [] and want["minLength"] == 17
    elif "min_len" not in kw:
        lo, hi = kw.get("min_lines", 2), kw.get("max_share", 0.25) * 3000
        assert len(want["top"]) == sum(lo <= c <= hi for c in n) and want["keys"] == len(failing)
        assert 0 < len(want["top"]) and (len(want["top"]) < len(failing)) == (kw != {"min_lines": 1} and kw != {"max_share": 1.0})


def test_stream_and_resident_equal_document(case, tmp_path):
    lp, log, _ = case
    data = log.encode()
    want = _golden(lp, log, top=None)
    for chunk_bytes, pieces in ((1 << 20, 1), (len(data) // 3 + 200, 3), (len(data) // 40, None)):
        with stream_lines(lp.engine, data, chunk_bytes) as walk:
            runs = [(p.ls.numel(), p.line_base) for p in walk]
        assert len(runs) == (pieces or len(runs)) and len(runs) >= (pieces or 40)
        assert sum(n for n, _ in runs) == 3000 and [b for _, b in runs] == [sum(n for n, _ in runs[:k]) for k in range(len(runs))]
        with stream_pieces(lp.engine, data, chunk_bytes) as ps:
            assert [(p.ls.numel(), p.line_base) for p in ps] == runs              # the same lines as the pieces
        assert lp.correlate_stream(data, chunk_bytes=chunk_bytes, top=None) == want, chunk_bytes
    head = "".join(log.splitlines(keepends=True)[:300])                            # one-line chunks
    with stream_lines(lp.engine, head.encode(), 64) as walk:
        assert [p.ls.numel() for p in walk] == [1] * 300
    assert lp.correlate_stream(head.encode(), chunk_bytes=64, top=None, min_lines=1) == _golden(lp, head, top=None, min_lines=1)
    for order in ("lines", "first"):
        assert lp.correlate_stream(data, chunk_bytes=5000, top=5, order=order, min_lines=4) == \
            _golden(lp, log, top=5, order=order, min_lines=4)
    res = lp.load_resident(data, chunk_bytes=20000)
    assert len(res.chunks) > 3 and lp.correlate_resident(res, top=None) == want
    assert lp.correlate_resident(res, min_len=12, order="first", max_share=0.01) == \
        _golden(lp, log, min_len=12, order="first", max_share=0.01)
    f = tmp_path / "app.log"
    f.write_bytes(data)
    assert lp.correlate_file(str(f), top=None) == want == lp.correlate_stream(str(f), chunk_bytes=3000, top=None)
    assert lp.engine.correlate_bytes(data, top=None) == want == lp.correlate(data, top=None)


# ---- 4. edge logs: a library of one word

def _boom_library():
    return [PatternSet.model_validate({"metadata": {"library_id": "correlate"}, "patterns": [
        {"id": "boom", "name": "boom", "severity": "CRITICAL", "primary_pattern": {"regex": r"BOOM", "confidence": 0.9},
         "context_extraction": {"lines_before": 2, "lines_after": 1}},
        {"id": "big", "name": "big boom", "severity": "HIGH", "primary_pattern": {"regex": r"BIG BOOM", "confidence": 0.8}}]})]


@pytest.fixture(scope="module")
def boom():
    return LogParser(_boom_library(), config=Config.load(overrides=CPU))


EDGE = {
    "empty": "",
    "only a line end": "\n",
    "no events": "start rid=abcdef0123\nwork rid=abcdef0123\n",
    "events but no keys": "start\nBOOM in worker 7\nBIG BOOM\n",
    "every line an event": "BOOM rid=aaaa1111bb\nBIG BOOM rid=AAAA1111BB trace=cccc2222dd\nBOOM trace=cccc2222dd\n",
    "an id only on its event line": "start rid=abcdef0123\nBOOM rid=ffff0000ff\nend rid=abcdef0123\n",
    "a key on every line": "host=node00042 start\nhost=node00042 BOOM rid=abcd1234\nhost=node00042 rid=abcd1234\nhost=node00042 x\n",
    "the id after the event, crlf": "BOOM rid=abcd1234\r\nwork\r\nlater RID=ABCD1234 done\r\n\r\n",
    "a ninth key on the event line": "BOOM " + " ".join("id%06dxx" % i for i in range(9)) + "\nlater id000008xx id000007xx\n",
    "bytes that are no utf-8": b"caf\xe9 BOOM \xffrid=abcd1234\xfe\nnext \x80abcd1234\x80\n",
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_logs(boom, name):
    log = EDGE[name]
    data = log if isinstance(log, bytes) else log.encode()
    for kw in ({"top": None}, {"top": None, "min_lines": 1, "max_share": 1.0}, {"order": "first", "min_len": 4}):
        want = golden.correlate(log, _boom_library(), boom.config.scoring, **kw)
        got = [boom.correlate(log, **kw), boom.correlate_stream(data, **kw), boom.correlate_stream(data, chunk_bytes=2, **kw)]
        if name != "only a line end":           # (a resident log of line ends alone holds one empty line, for every report)
            got.append(boom.correlate_resident(boom.load_resident(data, chunk_bytes=16), **kw))
        for k, g in enumerate(got):
            assert g == want, (name, kw, k)
    full = golden.correlate(log, _boom_library(), boom.config.scoring, top=None, min_lines=1, max_share=1.0)
    dflt = golden.correlate(log, _boom_library(), boom.config.scoring, top=None)
    if name in ("empty", "only a line end", "no events", "events but no keys"):
        assert full["keys"] == 0 and full["keyLines"] == 0 and full["top"] == []
        assert full["totalLines"] == {"empty": 1, "only a line end": 0}.get(name, 2 if name == "no events" else 3)
        assert (full["events"], full["eventLines"]) == ((3, 2) if name == "events but no keys" else (0, 0))
    elif name == "every line an event":
        assert (full["events"], full["eventLines"], full["keys"], full["keyLines"]) == (4, 3, 2, 3)
        assert [(r["key"], r["eventLines"], r["lines"], r["share"]) for r in full["top"]] == \
            [("aaaa1111bb", 2, 2, 1.0), ("cccc2222dd", 2, 2, 1.0)]
        assert dflt["top"] == []                                    # 2 lines of 3 are more than a quarter
    elif name == "an id only on its event line":
        assert dflt["keys"] == 1 and dflt["top"] == [] and [r["key"] for r in full["top"]] == ["ffff0000ff"]
    elif name == "a key on every line":
        assert [(r["key"], r["lines"]) for r in full["top"]] == [("node00042", 4), ("abcd1234", 2)]
        half = golden.correlate(log, _boom_library(), boom.config.scoring, max_share=0.5)
        assert [r["key"] for r in half["top"]] == ["abcd1234"] and half["keyLines"] == 4
    elif name == "the id after the event, crlf":
        assert [(r["firstLine"], r["lastLine"], r["firstEventLine"], r["example"]) for r in full["top"]] == \
            [(1, 3, 1, "BOOM rid=abcd1234")]
    elif name == "a ninth key on the event line":
        assert full["keys"] == 8 and full["keyLines"] == 2 and dflt["top"] == []
        assert (full["top"][0]["key"], full["top"][0]["lines"]) == ("id000007xx", 2)       # (the rest in the order of their hashes)
        assert sorted((r["key"], r["lines"]) for r in full["top"][1:]) == [("id%06dxx" % i, 1) for i in range(7)]
    else:
        assert [(r["key"], r["lines"]) for r in full["top"]] == [("abcd1234", 2)]


# ---- 5. arguments and the command line

def test_bad_arguments_raise(boom):
    log = "BOOM rid=abcd1234\nlater rid=abcd1234\n"
    res = boom.load_resident(log.encode())
    for kw in ({"order": "count"}, {"order": ""}, {"min_len": 3}, {"min_len": 65}, {"min_lines": 0}, {"max_share": 0.0},
               {"max_share": 1.5}, {"max_share": -0.1}):
        with pytest.raises(ValueError):
            golden.correlate(log, _boom_library(), boom.config.scoring, **kw)
        for call in (lambda: boom.correlate(log, **kw), lambda: boom.correlate_file(os.path.join(ROOT, "no", "such", "file"), **kw),
                     lambda: boom.correlate_stream(log.encode(), **kw), lambda: boom.correlate_resident(res, **kw),
                     lambda: boom.engine.correlate_bytes(log.encode(), **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="does not hold"):
        golden.correlate_row(H(b"abcd1234"), 1, 0, 1, 0, 0, b"another line 99998888", 8)


def test_frequency_window_untouched(boom):
    log = EDGE["every line an event"] * 5
    before = boom.frequency_statistics()
    assert boom.correlate(log, max_share=1.0)["events"] == 20
    assert boom.correlate_stream(log.encode(), chunk_bytes=64, max_share=1.0)["events"] == 20
    assert boom.frequency_statistics() == before


def _cli(*argv, code: int = 0):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "correlate", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == code, r.stderr
    return json.loads(r.stdout) if code == 0 else r.stderr


def test_cli(tmp_path):
    log = tmp_path / "app.log"
    log.write_text("starting\nINFO request 7 accepted trace=4bf92f3577b34da6\nINFO request 8 accepted trace=00f067aa0ba902b7\n"
                   "INFO cache warm trace=00f067aa0ba902b7\nINFO db call trace=4bf92f3577b34da6\n"
                   "ERROR OOMKilled container app trace=4BF92F3577B34DA6\nINFO request 8 served trace=00f067aa0ba902b7\n"
                   "INFO cleanup after trace=4bf92f3577b34da6\n" + "INFO idle\n" * 8)
    one = _cli(str(log), "--max-share", "0.5")
    assert set(one) == KEYS and one["totalLines"] == 16 and one["eventLines"] == 1 and one["keys"] == 1 and one["keyLines"] == 4
    assert one["top"] == [{"key": "4bf92f3577b34da6", "eventLines": 1, "lines": 4, "share": 0.25, "firstLine": 2, "lastLine": 8,
                           "firstEventLine": 6, "signature": "%016x" % H(b"4bf92f3577b34da6"),
                           "example": "INFO request 7 accepted trace=4bf92f3577b34da6"}]
    assert _cli(str(log), "--max-share", "0.5", "--stream", "--chunk-bytes", "32") == one
    other = _cli(str(log), "--min-length", "12", "--order", "first", "--top", "3", "--min-lines", "5")
    assert other["keys"] == 1 and other["minLength"] == 12 and other["top"] == []
    assert "min_len" in _cli(str(log), "--min-length", "3", code=2)
