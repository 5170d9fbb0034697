"""Variants report on the CPU engine (log_parser_amd/variants.py, the host twins of
csrc/kernels/variants.hip): the field numbering of ``golden.line_fields`` and the token hash on
hand-written lines, the host twin of ``line_vars`` against them triple for triple, the report against
``golden.variants`` and against what ``synth.variant_log`` plants -- as a document, a stream at 64 B /
4 KiB / 1 MiB chunks, a resident log and an accumulator fed in two parts, every order and filter --
the boundary at ``max_distinct``, the lines an id field brings to the host (none), the report's
cross-checks, arguments and the command line.

Mutations that were made, one at a time, and the tests that failed with each (the host twins share
their source with the kernels, so a mutation of var_core.h is one of both):

* var_core.h ``var_step`` folds ``c | 32`` (the hash lowers the case): test_fields_by_hand (the
  ``0xAB 0xab 0xAb`` and ``REQ9 req9`` lines), test_host_twin_matches_golden[hand] and [random],
  test_edge_logs[case] (the report's own cross-check raises: the token does not hash to the value);
* var_core.h ends a field without looking at ``hid`` (hidden tokens are numbered):
  test_fields_by_hand (the five lines with a stamp), test_host_twin_matches_golden[hand] and
  [random], test_planted_field, test_report_equals_golden, test_report_parameters,
  test_stream_resident_and_accumulator_equal_document, test_cli;
* variants.py ``distinct >= max_distinct`` instead of ``>``: test_boundary_at_max_distinct (every D),
  test_planted_field (the status field has exactly two values at D = 2),
  test_stream_resident_and_accumulator_equal_document, test_id_field_brings_no_line, four of
  test_edge_logs, test_cli;
* variants.hip ``var_fold_host`` keeps ``last`` with ``std::min``: every test of test_var_table.py
  that folds (test_first_and_last_are_min_and_max among them), and nearly every report test here
  (the report's cross-check raises: a value ends before it begins); the same in the kernel's
  ``vt_apply`` (``atomicMin``), run on an MI355X: all 21 tests of test_gpu_var_table.py;
* variants.hip ``k_var_fold`` without ``vt_skipped`` on the direct path, run on an MI355X (only a GPU
  test can see it: the host twin has one path): test_gpu_var_table.py test_skip_on_both_paths,
  test_hot_key_and_side_slot, test_distinct_keys_per_tile[1023 .. 3000] and test_sizes[2049-2048],
  [5000-2048] -- every case in which a tile overflows its LDS table while a skip set is in force;
* variants.py asks for the winners before the purge: test_id_field_brings_no_line.
"""
import json
import os
import subprocess
import sys
from fractions import Fraction

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, variant_log
from log_parser_amd.variants import VariantAccumulator
from values_cases import HAND, index, random_lines
from variants_cases import VAR_HAND, signed, want_triples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "patterns", "examples", "k8s")
KEYS = {"totalLines", "fieldLines", "tokens", "templates", "fields", "unboundedFields", "maxDistinct", "top"}
ROW_KEYS = {"signature", "field", "count", "lines", "fill", "distinct", "odd", "oddShare", "firstLine", "template",
            "example", "values"}
VALUE_KEYS = {"token", "count", "share", "firstLine", "lastLine"}
CPU = {"engine.device": "cpu"}
ORDERS = ("odd", "count", "distinct", "first")
EVERY = {"top": None, "min_count": 1, "min_fill": 0.0, "varying": False}


# ---- 1. the fields and the hash, by hand

def test_var_hash():
    assert golden.var_hash(b"") == 0xcbf29ce484222325 and golden.var_hash(b"a") == 0xaf63dc4c8601ec8c
    assert golden.var_hash(b"foobar") == 0x85944171f73967e8                        # (the published FNV-1a-64 vectors)
    assert golden.var_hash(b"0xAB") != golden.var_hash(b"0xab") and golden.var_hash(b"12") != golden.var_hash(b"012")


@pytest.mark.parametrize("k", range(len(VAR_HAND)))
def test_fields_by_hand(k):
    line, want = VAR_HAND[k]
    assert [(j, t) for j, _, t in golden.line_fields(line)] == want
    # ... and the twin on that one line
    text = torch.frombuffer(bytearray(line + b"\n"), dtype=torch.uint8)
    sig, ln, field, value, cnt = K.line_vars(text, torch.tensor([0]), torch.tensor([len(line)], dtype=torch.int32))
    assert cnt == (len(want), int(bool(want))) and sig.tolist() == [signed(golden.line_signature(line))]
    assert list(zip(field.tolist(), value.tolist())) == \
        [(signed(golden.val_key(golden.line_signature(line), j)), signed(golden.var_hash(t))) for j, t in want]


# ---- 2. the host twin against the rule, triple for triple

def _check_twin(lines, idx):
    sigs, triples, held = want_triples(lines)
    for cap in (None, len(triples), max(0, len(triples) - 1), 1, 0):               # cap below the count: the re-run
        sig, line, field, value, (m, h) = K.line_vars(*idx, cap=cap)
        assert (sig.dtype, line.dtype, field.dtype, value.dtype) == (torch.int64, torch.int32, torch.int64, torch.int64)
        assert sig.tolist() == sigs and (m, h) == (len(triples), held)
        assert list(zip(line.tolist(), field.tolist(), value.tolist())) == triples  # (the twin appends in line order)
    return triples


@pytest.mark.parametrize("which", ["hand", "random"])
def test_host_twin_matches_golden(which):
    # (the lines that end in CR stay with test_fields_by_hand: the splitter of a text takes a CR LF as the line end)
    lines = [x for x, _ in HAND] + [x for x, _ in VAR_HAND if not x.endswith(b"\r")] if which == "hand" else random_lines(700, 11)
    for shift in (0, 1, 15):
        idx = index(lines, shift)
        triples = _check_twin(lines, idx)
        assert len(triples) > len(lines)
        # the numbering is line_fields': where a field has a number, line_values names the same j
        vsig, vline, vkey, _, _ = K.line_values(*idx)
        assert set(zip(vline.tolist(), vkey.tolist())) <= {(i, f) for i, f, _ in triples}
    data = b"\n".join(lines)                    # ... and with the usual padding behind the text
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    _check_twin(lines, (text, *K.split_chunk_lines(text, len(data))))


def test_line_vars_arguments():
    text, ls, ll = index([b"status 503", b"x"], 0)
    none = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int32)
    sig, line, field, value, cnt = K.line_vars(text, *none)
    assert (sig.numel(), line.numel(), field.numel(), value.numel(), cnt) == (0, 0, 0, 0, (0, 0))
    for bad in (4096, -1):
        with pytest.raises(ValueError):
            K.line_vars(text, ls, ll, per_block=bad)
    # a line index that points outside the text is clipped to it, never read
    sig, line, field, value, cnt = K.line_vars(text, torch.tensor([7, 99, -3]), torch.tensor([400, 5, 10], dtype=torch.int32))
    assert cnt == (2, 2) and line.tolist() == [0, 2] and value.tolist() == [signed(golden.var_hash(b"503"))] * 2
    assert sig[1] == signed(golden.line_signature(b""))


# ---- 3. the report: a log with a planted status field, a worker field and a request id

@pytest.fixture(scope="module")
def case():
    """(CPU parser, the 4000-line variant log with some CRLF, its planted facts, golden's report of every field)."""
    lp = LogParser([], config=Config.load(overrides=CPU))
    log, facts = variant_log(4000, log_templates(30, 1), seed=2, crlf_rate=0.05)
    return lp, log, facts, golden.variants(log, **EVERY)


def _groups(log):
    """{(signature, field): {token: [lines]}} of a log, straight from ``golden.line_fields``."""
    out = {}
    for i, x in enumerate(golden.split_lines(log)):
        for j, _, t in golden.line_fields(x.encode()):
            out.setdefault(("%016x" % golden.line_signature(x.encode()), j), {}).setdefault(t.decode(), []).append(i)
    return out


def test_synthetic_log_is_what_it_says(case):
    _, log, facts, full = case
    lines = golden.split_lines(log)
    assert len(lines) == 4000 and 100 < log.count("\r\n") < 300
    ours = [(i, x.split()) for i, x in enumerate(lines) if "upstream returned status" in x]
    assert len(ours) == facts["lines"] and 300 < len(ours) < 500 and facts["template"].startswith("INFO  [proxy] upstream")
    lo, hi = facts["rareRange"]
    assert (lo, hi) == (2800, 3200) and [i for i, w in ours if w[6] == "503"] == facts["rareLines"]
    assert 3 <= len(facts["rareLines"]) <= 20 and all(lo <= i < hi for i in facts["rareLines"])
    assert all(w[6] in ("200", "503") for _, w in ours) and [int(w[9]) for _, w in ours] == [k % 8 for k in range(len(ours))]
    assert len({w[12] for _, w in ours}) == len(ours)                               # the request id never repeats
    assert variant_log(500, log_templates(10), seed=3) == variant_log(500, log_templates(10), seed=3)
    assert full["totalLines"] == 4000 and full["templates"] == 31 and full["fields"] == len(full["top"]) + full["unboundedFields"]
    assert full["tokens"] > 8000 and full["fieldLines"] == 4000


def test_planted_field(case):
    lp, log, facts, _ = case
    rep = lp.variants(log)
    assert rep == golden.variants(log) and set(rep) == KEYS and all(set(r) == ROW_KEYS for r in rep["top"])
    assert all(set(v) == VALUE_KEYS for r in rep["top"] for v in r["values"]) and rep["maxDistinct"] == 64
    top = rep["top"][0]
    assert top["template"].endswith("upstream returned status 0 to worker 0 for request 0") and top["field"] == 0
    n, rare = facts["lines"], facts["rareLines"]
    assert (top["count"], top["lines"], top["fill"], top["distinct"], top["odd"]) == (n, n, 1.0, 2, len(rare))
    assert top["oddShare"] == len(rare) / n < 0.06
    common, odd = top["values"]
    assert (common["token"], common["count"], odd["token"], odd["count"]) == ("200", n - len(rare), "503", len(rare))
    assert (odd["firstLine"], odd["lastLine"]) == (rare[0] + 1, rare[-1] + 1) and odd["share"] == len(rare) / n
    assert facts["rareRange"][0] < odd["firstLine"] <= facts["rareRange"][1]
    # the worker field is listed with its eight values, evenly spread; the request id is only counted
    mine = [r for r in rep["top"] if r["signature"] == top["signature"]]
    assert [r["field"] for r in mine] == [0, 1] and mine[1]["distinct"] == 8 and len(mine[1]["values"]) == 8
    assert sorted(v["token"] for v in mine[1]["values"]) == list("01234567") and 0.85 < mine[1]["oddShare"] < 0.9
    assert max(v["count"] for v in mine[1]["values"]) - min(v["count"] for v in mine[1]["values"]) <= 1
    every = lp.variants(log, **EVERY)
    assert not any(r["signature"] == top["signature"] and r["field"] == 2 for r in every["top"])
    assert every["unboundedFields"] >= 1 and all(r["distinct"] <= 64 for r in every["top"])
    # at D = 4 the worker field is unbounded too; at D = 2 the status field still fits
    for D, fields in ((4, [0]), (2, [0])):
        rep = lp.variants(log, max_distinct=D, **EVERY)
        assert rep == golden.variants(log, max_distinct=D, **EVERY) and rep["maxDistinct"] == D
        assert [r["field"] for r in rep["top"] if r["signature"] == top["signature"]] == fields


@pytest.mark.parametrize("order", ORDERS)
def test_report_equals_golden(case, order):
    lp, log, _, full = case
    want = golden.variants(log, top=None, order=order)
    got = lp.variants(log, top=None, order=order)
    assert got == want and {k: got[k] for k in KEYS - {"top"}} == {k: full[k] for k in KEYS - {"top"}}
    rows = got["top"]
    assert 10 < len(rows) <= full["fields"] - full["unboundedFields"]
    key = {"odd": lambda r: (Fraction(r["odd"], r["count"]), -r["count"], r["firstLine"], int(r["signature"], 16), r["field"]),
           "count": lambda r: (-r["count"], r["firstLine"], int(r["signature"], 16), r["field"]),
           "distinct": lambda r: (-r["distinct"], r["firstLine"], int(r["signature"], 16), r["field"]),
           "first": lambda r: (r["firstLine"], r["field"])}[order]
    assert rows == sorted(rows, key=key)
    lines, groups = golden.split_lines(log), _groups(log)
    for r in rows:
        vals = groups[r["signature"], r["field"]]
        assert (r["count"], r["distinct"]) == (sum(map(len, vals.values())), len(vals)) and 1 < r["distinct"] <= 64
        assert r["odd"] == r["count"] - max(map(len, vals.values())) and r["oddShare"] == r["odd"] / r["count"]
        assert r["firstLine"] == min(v[0] for v in vals.values()) + 1 and r["example"] == lines[r["firstLine"] - 1]
        assert r["fill"] == r["count"] / r["lines"] >= 0.9 and r["count"] >= 5
        order_of = sorted(vals, key=lambda t: (-len(vals[t]), vals[t][0]))
        shown = order_of if len(vals) <= 10 else order_of[:5] + order_of[-5:]
        assert [v["token"] for v in r["values"]] == shown
        for v in r["values"]:
            at = vals[v["token"]]
            assert (v["count"], v["firstLine"], v["lastLine"], v["share"]) == (len(at), at[0] + 1, at[-1] + 1, len(at) / r["count"])
    assert lp.variants(log, order=order) == golden.variants(log, order=order)
    assert lp.variants(log, top=3, order=order)["top"] == want["top"][:3] and lp.variants(log, top=0, order=order)["top"] == []
    for show in (1, 2, 40):
        assert lp.variants(log, top=None, order=order, show=show) == golden.variants(log, top=None, order=order, show=show)


@pytest.mark.parametrize("kw", [{"min_count": 1}, {"min_count": 60}, {"min_fill": 0.0}, {"min_fill": 1.0}, {"varying": False},
                                dict(EVERY, top=20), {"min_count": 2, "min_fill": 0.5}, {"show": 1}])
def test_report_parameters(case, kw):
    """The variant log with a few lines that each filter alone drops: a field that never varies, a
    field on some lines of its template only, a template with three lines."""
    lp, log, _, _ = case
    log = log + "retry 5 of 5\n" * 8 + "".join("ptr 0x%x\n" % (v % 3 << 4 | 0xf if v % 2 else 0xff) for v in range(16)) \
        + "rare %d\nlast 1\n" * 3 % (7, 8, 9)
    full = golden.variants(log, **EVERY)
    for order in ("first", "odd"):
        want = golden.variants(log, top=None, order=order, **{k: v for k, v in kw.items() if k != "top"})
        assert lp.variants(log, top=None, order=order, **{k: v for k, v in kw.items() if k != "top"}) == want
    every = full["top"]
    keep = [r for r in every if r["count"] >= kw.get("min_count", 5) and r["count"] >= kw.get("min_fill", 0.9) * r["lines"]
            and (not kw.get("varying", True) or r["distinct"] > 1)]
    assert len(want["top"]) == len(keep) > 0 and (len(keep) == len(every)) == (kw.get("varying") is False and len(kw) > 1)
    assert all(len(r["values"]) <= 2 for r in want["top"]) or kw.get("show", 5) == 5


def test_stream_resident_and_accumulator_equal_document(case, tmp_path):
    lp, log, _, _ = case
    data = log.encode()
    for D in (64, 4):
        want = golden.variants(log, max_distinct=D, top=None)
        for chunk_bytes in (4096, 1 << 20):
            assert lp.variants_stream(data, chunk_bytes=chunk_bytes, max_distinct=D, top=None) == want, chunk_bytes
        res = lp.load_resident(data, chunk_bytes=20000)
        assert len(res.chunks) > 3 and lp.variants_resident(res, max_distinct=D, top=None) == want
        # an accumulator fed in two parts, each in another form; the report in between is the first part's
        keep = log.splitlines(keepends=True)
        a, b = "".join(keep[:1700]), "".join(keep[1700:])
        acc = lp.variant_accumulator(D)
        acc.add_document(a)
        assert acc.report(top=None, order="first") == golden.variants(a, max_distinct=D, top=None, order="first")
        acc.add_stream(b.encode(), 7000)
        assert acc.report(top=None) == want
        acc = VariantAccumulator(lp.engine, D)
        acc.add_resident(lp.load_resident(a.encode(), chunk_bytes=9000))
        acc.add_document(b.encode())
        assert acc.report(top=None, order="count") == golden.variants(log, max_distinct=D, top=None, order="count")
    head = "".join(log.splitlines(keepends=True)[:150])                              # one-line chunks
    for D in (2, 64):
        assert lp.variants_stream(head.encode(), chunk_bytes=64, max_distinct=D, **EVERY) == \
            golden.variants(head, max_distinct=D, **EVERY)
    for order in ORDERS[1:]:
        assert lp.variants_stream(data, chunk_bytes=5000, top=5, order=order, min_count=9) == \
            golden.variants(log, top=5, order=order, min_count=9)
    f = tmp_path / "app.log"
    f.write_bytes(data)
    want = golden.variants(log, top=None)
    assert lp.variants_file(str(f), top=None) == want == lp.variants_stream(str(f), chunk_bytes=3000, top=None)
    assert lp.engine.variants_bytes(data, top=None) == want == lp.variants(data, top=None)


# ---- 4. the boundary at max_distinct, and what an id field costs

def _boundary_log(D: int) -> str:
    """``alpha`` has exactly D values; ``beta`` has D + 1, the last of them far behind the first;
    ``gamma`` has D + 1, the last of them on the log's last line."""
    head = "".join("alpha v%d\nbeta v%d\ngamma v%d\n" % (k, k, k) for k in range(D)) * 3
    filler = "".join("tick %d of 9\n" % (k % 2) for k in range(400))               # ~5 KiB: beta's last value is chunks away
    return head + filler + "beta v%d\n" % D + filler + "alpha v0\n" * 2 + "gamma v%d\n" % D


@pytest.mark.parametrize("D", [2, 4, 64])
def test_boundary_at_max_distinct(D):
    lp = LogParser([], config=Config.load(overrides=CPU))
    log = _boundary_log(D)
    want = golden.variants(log, max_distinct=D, **EVERY)
    names = {r["example"].split()[0]: r for r in want["top"]}
    assert set(names) == {"alpha", "tick"} and names["alpha"]["distinct"] == D and want["unboundedFields"] == 2
    assert want["fields"] == 5 and len(names["alpha"]["values"]) == min(D, 10)
    got = [lp.variants(log, max_distinct=D, **EVERY)] + \
        [lp.variants_stream(log.encode(), chunk_bytes=c, max_distinct=D, **EVERY) for c in (64, 4096, 1 << 20)]
    got.append(lp.variants_resident(lp.load_resident(log.encode(), chunk_bytes=2048), max_distinct=D, **EVERY))
    for k, g in enumerate(got):
        assert g == want, k
    if D < golden.VAR_MAX_DISTINCT:
        more = lp.variants_stream(log.encode(), chunk_bytes=4096, max_distinct=D + 1, **EVERY)
        assert more == golden.variants(log, max_distinct=D + 1, **EVERY) and more["unboundedFields"] == 0
        assert {r["example"].split()[0]: r["distinct"] for r in more["top"]} == {"alpha": D, "beta": D + 1, "gamma": D + 1,
                                                                                 "tick": 2}
    # the table after the log: the enumerable fields' rows only
    acc = lp.variant_accumulator(D)
    acc.add_stream(log.encode(), 4096)
    assert acc.table.used == D + 2 + 1 and len(acc.unbounded) == 2


def test_id_field_brings_no_line():
    """One id field of 3,000 distinct values and D = 4: no example line is fetched for it -- as a
    document and in 4 KiB chunks (the first chunk alone takes it above D)."""
    lp = LogParser([], config=Config.load(overrides=CPU))
    log = "".join("request r%05d served by worker w%d\n" % (i * 7919 % 100003, i % 3) for i in range(3000))
    sig = golden.line_signature(b"request r00000 served by worker w0")
    id_key, worker_key = signed(golden.val_key(sig, 0)), signed(golden.val_key(sig, 1))
    for feed in (lambda a: a.add_document(log), lambda a: a.add_stream(log.encode(), 4096),
                 lambda a: a.add_resident(lp.load_resident(log.encode(), chunk_bytes=4096))):
        acc = lp.variant_accumulator(4)
        feed(acc)
        assert acc.example_fields == [worker_key] * 3 and acc.example_lines == 3 and id_key not in acc.example_fields
        assert acc.unbounded == {id_key} and acc.table.used == 3
        rep = acc.report(top=None)
        assert rep == golden.variants(log, max_distinct=4, top=None) and rep["unboundedFields"] == 1 and len(rep["top"]) == 1
        assert rep["tokens"] == 6000 and [v["token"] for v in rep["top"][0]["values"]] == ["w0", "w1", "w2"]
    # (in one-line chunks an id field shows D values before it is known to be one: at most D lines)
    acc = lp.variant_accumulator(4)
    acc.add_stream(log.encode()[:3700], 64)
    assert acc.example_fields.count(id_key) == 4 and acc.unbounded == {id_key}


# ---- 5. edge logs

EDGE = {
    "empty": "",
    "only a line end": "\n",
    "no digit": "start\nwork in progress\nend\n",
    "crlf": "exit code 1\r\nexit code 1\r\n\r\nexit code 137\r\n",
    "one long line": "v 1 " + "x" * 4990 + " 2",
    "a field that never varies": "retry 5 of 5\nretry 5 of 5\nretry 5 of 5\n",
    "case": "peer 0xAB up\npeer 0xab up\npeer 0xAB up\n",
    "nine fields": "a1 b2 c3 d4 e5 f6 g7 h8 i9\n" * 2 + "a1 b2 c3 d4 e5 f6 g7 h0 i7\n",
    "bytes that are no utf-8": b"caf\xe9 7ms \xff\nnext\x80 9 \x80\ncaf\xe9 9ms \xff\n",
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_logs(name):
    lp = LogParser([], config=Config.load(overrides=CPU))
    log = EDGE[name]
    data = log if isinstance(log, bytes) else log.encode()
    for kw in ({"top": None}, EVERY, {"order": "first", "min_count": 2}, dict(EVERY, order="distinct", max_distinct=2, show=1)):
        want = golden.variants(log, **kw)
        got = [lp.variants(log, **kw), lp.variants_stream(data, **kw), lp.variants_stream(data, chunk_bytes=2, **kw)]
        if name != "only a line end":           # (a resident log of line ends alone holds one empty line, for every report)
            got.append(lp.variants_resident(lp.load_resident(data, chunk_bytes=16), **kw))
        for k, g in enumerate(got):
            assert g == want, (name, kw, k)
    full = golden.variants(log, **EVERY)
    rows = [(r["field"], r["count"], r["lines"], r["distinct"], r["odd"], r["firstLine"],
             [(v["token"], v["count"], v["firstLine"], v["lastLine"]) for v in r["values"]]) for r in full["top"]]
    if name in ("empty", "only a line end", "no digit"):
        assert rows == [] and (full["tokens"], full["fieldLines"], full["fields"]) == (0, 0, 0)
    elif name == "crlf":
        assert rows == [(0, 3, 3, 2, 1, 1, [("1", 2, 1, 2), ("137", 1, 4, 4)])] and full["top"][0]["example"] == "exit code 1"
    elif name == "one long line":
        assert rows == [(0, 1, 1, 1, 0, 1, [("1", 1, 1, 1)])]
    elif name == "a field that never varies":
        assert rows == [(0, 3, 3, 1, 0, 1, [("5", 3, 1, 3)]), (1, 3, 3, 1, 0, 1, [("5", 3, 1, 3)])]
        assert golden.variants(log, min_count=1)["top"] == []
    elif name == "case":
        assert rows == [(0, 3, 3, 2, 1, 1, [("0xAB", 2, 1, 3), ("0xab", 1, 2, 2)])]
    elif name == "nine fields":
        assert [r[0] for r in rows] == list(range(8)) and rows[7][6] == [("h8", 2, 1, 2), ("h0", 1, 3, 3)]     # (no ninth)
        assert full["tokens"] == 24
    else:
        assert rows == [(0, 1, 1, 1, 0, 2, [("9", 1, 2, 2)]), (0, 2, 2, 2, 1, 1, [("7ms", 1, 1, 1), ("9ms", 1, 3, 3)])]


# ---- 6. the report's cross-checks, arguments and the command line

def test_report_cross_checks():
    lp = LogParser([], config=Config.load(overrides=CPU))
    log = "exit code 1\nexit code 1\nexit code 137\n"

    def fed():
        acc = VariantAccumulator(lp.engine)
        acc.add_document(log)
        return acc
    assert fed().report(**EVERY) == golden.variants(log, **EVERY)
    acc = fed()                                 # a count above the template's lines
    acc.table._count[acc.table._count > 0] += 5
    with pytest.raises(RuntimeError, match="tokens on"):
        acc.report(**EVERY)
    acc = fed()                                 # a value that ends before it begins
    acc.table._last[acc.table._count > 0] = -1
    with pytest.raises(RuntimeError, match="ends before"):
        acc.report(**EVERY)
    acc = fed()                                 # an example line whose token does not hash to the value
    held = acc._examples._held
    for k, (o, (s, raw)) in list(held.items()):
        held[k] = (o, (s, raw.replace(b"137", b"138")))
    with pytest.raises(RuntimeError, match="does not hold"):
        acc.report(**EVERY)
    acc = fed()                                 # an example that is not the value's first line
    acc.table._first[acc.table._count == 2] = 1
    with pytest.raises(RuntimeError, match="not its first line"):
        acc.report(**EVERY)
    sig = golden.line_signature(b"exit code 1")
    with pytest.raises(ValueError, match="does not hold"):
        golden.variants_value(sig, 0, golden.var_hash(b"2"), 1, 1, 0, 0, b"exit code 1")
    with pytest.raises(ValueError, match="does not hold"):
        golden.variants_value(sig, 1, golden.var_hash(b"1"), 1, 1, 0, 0, b"exit code 1")


def test_bad_arguments_raise():
    lp = LogParser([], config=Config.load(overrides=CPU))
    log = "exit code 1\nexit code 137\n"
    res = lp.load_resident(log.encode())
    for kw in ({"order": "peak"}, {"order": ""}, {"min_count": 0}, {"min_count": 2.5}, {"min_fill": -0.1}, {"min_fill": 1.5},
               {"min_fill": "0.9"}, {"show": 0}, {"show": 1.5}, {"max_distinct": 1}, {"max_distinct": 4097},
               {"max_distinct": 8.0}, {"max_distinct": True}):
        with pytest.raises(ValueError):
            golden.variants(log, **kw)
        acc_kw = {k: v for k, v in kw.items() if k != "max_distinct"}
        for call in (lambda: lp.variants(log, **kw), lambda: lp.variants_file(os.path.join(ROOT, "no", "such", "file"), **kw),
                     lambda: lp.variants_stream(log.encode(), **kw), lambda: lp.variants_resident(res, **kw),
                     lambda: lp.engine.variants_bytes(log.encode(), **kw),
                     lambda: lp.variant_accumulator(kw.get("max_distinct", 64)).report(**acc_kw)):
            with pytest.raises(ValueError):
                call()
    for bad in (-1, 1 << 62, 1.5, True):
        with pytest.raises(ValueError):
            VariantAccumulator(lp.engine, line_base=bad)
    acc = lp.variant_accumulator(line_base=10 ** 12)                                # a log that continues an earlier one
    acc.add_document(log)
    rep = acc.report(**EVERY)
    assert [(v["firstLine"], v["lastLine"]) for v in rep["top"][0]["values"]] == [(10 ** 12 + 1,) * 2, (10 ** 12 + 2,) * 2]


def test_frequency_window_untouched():
    lp = LogParser.from_directory(PAT, config=Config.load(overrides=CPU))
    log = "ERROR OOMKilled container app exit code 1\n" * 6 + "ERROR OOMKilled container app exit code 137\n"
    before = lp.frequency_statistics()
    assert lp.variants(log)["tokens"] == 7 and lp.variants(log)["top"][0]["odd"] == 1
    assert lp.variants_stream(log.encode(), chunk_bytes=64)["tokens"] == 7
    acc = lp.variant_accumulator()
    acc.add_resident(lp.load_resident(log.encode()))
    assert acc.report()["tokens"] == 7 and lp.frequency_statistics() == before


def _cli(*argv, code: int = 0):
    r = subprocess.run([sys.executable, "-m", "log_parser_amd", "variants", *argv, "--patterns", PAT, "--device", "cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == code, r.stderr
    return json.loads(r.stdout) if code == 0 else r.stderr


def test_cli(tmp_path):
    text, facts = variant_log(600, log_templates(8, 1), seed=4, rare_from=0.5, rare_to=0.9)
    log = tmp_path / "app.log"
    log.write_text(text)
    one = _cli(str(log))
    assert one == golden.variants(text) and set(one) == KEYS and one["totalLines"] == 600
    assert one["top"][0]["values"][-1]["token"] == "503" and one["top"][0]["values"][-1]["firstLine"] == facts["rareLines"][0] + 1
    other = _cli(str(log), "--stream", "--chunk-bytes", "4096", "--max-distinct", "8", "--order", "count", "--top", "3",
                 "--min-count", "2", "--min-fill", "0.5", "--all", "--show", "1")
    assert other == golden.variants(text, max_distinct=8, top=3, order="count", min_count=2, min_fill=0.5, varying=False, show=1)
    assert [r["distinct"] for r in other["top"]] == [2, 8] and other["unboundedFields"] == 20      # status and worker
    # several files continue ONE log
    keep = text.splitlines(keepends=True)
    a, b = tmp_path / "a.log", tmp_path / "b.log"
    a.write_text("".join(keep[:250]))
    b.write_text("".join(keep[250:]))
    assert _cli(str(a), str(b)) == one
    assert "min_count" in _cli(str(log), "--min-count", "0", code=2)
    assert "max_distinct" in _cli(str(log), "--max-distinct", "1", code=2)
