"""Variants report on a resident 1M-line document: the variants kernel next to the value kernel on the
same text, the rate of the whole report, and where the report's time goes.

The document is ``utils.synth.variant_log``: the templated log of ``bench_values.py`` with an
``upstream returned status <code> to worker <w> for request <id>`` line on about a tenth of its
lines -- a status field with a rare code confined to a range of lines, a worker field of eight
values, and a request id that never repeats.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``line_vars_ms``     (a) ``K.line_vars`` (k_line_vars: walk every line once for its template
                       signature and the token hashes of its fields, compact the (line, field,
                       value) triples; one counter read);
* ``line_values_ms``   (b) ``K.line_values`` of the same text (k_line_vals walks the same bytes and
                       emits the numeric fields only);
                       both with room for 4 triples per line, so that neither call walks twice
                       (``line_values_default_ms``: the same call at its own first capacity of 2 per
                       line, which this log exceeds -- the re-run is a second pass);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``variants_resident_lines_per_s``  (c) ``variants_stream`` of the document as a resident log: the
                       kernel, the folds, census, purge and winners per chunk, and the report;
* ``fold_lines_ms`` / ``fold_ms`` / ``census_ms`` / ``purge_ms`` / ``winners_ms`` / ``examples_ms``
                       the steps of one piece of (c) on the whole document's triples: the
                       ``GapTable`` fold of the signatures, the ``VarTable`` fold into a fresh table
                       (nothing skipped: the first piece of a log), the rows with ``unique``, the
                       purge of the fields above D from a table that holds them, the winners after
                       it, and the fetch of the winners' lines;
* ``fold_skip_ms``     the same fold with the unbounded fields skipped (every later piece);
* ``report_ms``        ``VariantAccumulator.report(top=5)`` alone, of an accumulator that holds the
                       document.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_variants.py --rounds 1 --steps 3 --warmup 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from log_parser_amd.engine import Engine  # noqa: E402
from log_parser_amd.models.compiled import CompiledLibrary  # noqa: E402
from log_parser_amd.ops import kernels as K  # noqa: E402
from log_parser_amd.parallel.stream import ResidentLog  # noqa: E402
from log_parser_amd.pieces import gather_lines  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import log_templates, realistic_library, variant_log  # noqa: E402
from log_parser_amd.variants import VariantAccumulator, variants_stream  # noqa: E402


def _median_ms(fn, warmup: int, steps: int, dev) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=300)
    ap.add_argument("--max-distinct", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_variants: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    D = args.max_distinct
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, facts = variant_log(args.lines, log_templates(args.templates, seed=11), seed=5)
    data = log.encode()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    out = {}

    room = 4 * L        # one pass each: this log holds more than two numbers per line, above ``line_values``' first capacity

    def vars_():
        out["a"] = K.line_vars(text, ls, ll, cap=room)

    def vals():
        out["b"] = K.line_values(text, ls, ll, cap=room)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(vars_, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(vals, args.warmup, args.steps, dev))
    sig, line, field, value, (triples, held) = out["a"]
    default_ms = _median_ms(lambda: K.line_values(text, ls, ll), args.warmup, args.steps, dev)
    res = ResidentLog.load(data, eng)

    def report():
        out["c"] = variants_stream(eng, res, max_distinct=D, top=5)

    few = max(3, args.steps // 2)
    c_ms = _median_ms(report, 1, few, dev)
    rep = out["c"]
    # the steps of VariantAccumulator._add_piece on the whole document's triples
    g = line.long()
    every = torch.arange(L, dtype=torch.int64, device=dev)
    parts = {"fold_lines_ms": _median_ms(lambda: K.GapTable(dev).fold(sig, every, winners=False), 1, few, dev),
             "fold_ms": _median_ms(lambda: K.VarTable(dev).fold(field, value, g), 1, few, dev)}
    full = K.VarTable(dev)
    full.fold(field, value, g)

    def census():
        fields, distinct = torch.unique(full.rows()[0], return_counts=True)
        out["over"] = fields[distinct > D]

    parts["census_ms"] = _median_ms(census, 1, few, dev)
    over = out["over"]
    skip = K.GapTable(dev)
    skip.fold(over, torch.zeros_like(over), winners=False)
    parts["fold_skip_ms"] = _median_ms(lambda: K.VarTable(dev).fold(field, value, g, skip=skip), 1, few, dev)
    rows = tuple(c.clone() for c in full.rows())
    rows_n, cap = rows[0].numel(), full.cap

    def purge():
        t = K.VarTable(dev, cap=cap)            # the table as the fold left it: re-inserted, then purged
        t._reinsert(rows, rows_n)
        t._bound = rows_n
        out["purged"] = t.purge(over)
        out["t"] = t

    def refill():
        t = K.VarTable(dev, cap=cap)
        t._reinsert(rows, rows_n)

    # (the purge is timed with the re-insert that sets it up, and that re-insert alone is taken off)
    parts["purge_ms"] = max(0.0, _median_ms(purge, 1, few, dev) - _median_ms(refill, 1, few, dev))
    kept = out["t"]
    parts["winners_ms"] = _median_ms(lambda: out.__setitem__("w", kept.winners(field, value, g)), 1, few, dev)
    win = out["w"]
    parts["examples_ms"] = _median_ms(lambda: gather_lines(text, ls[line[win].long()], ll[line[win].long()]), 1, few, dev)
    fed = VariantAccumulator(eng, D)
    fed.add_resident(res)
    parts["report_ms"] = _median_ms(lambda: fed.report(top=5), 1, few, dev)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    top = rep["top"][0] if rep["top"] else {}
    rare = top.get("values", [{}])[-1]
    lo, hi = facts["rareRange"]
    print(json.dumps({"config": f"variants-{L}-lines-{args.templates}-templates-D{D}", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "triples": triples, "field_lines": held,
                      "triples_per_line": round(triples / max(1, L), 3), "value_triples": out["b"][4][0],
                      "line_vars_ms": round(a, 3), "line_values_ms": round(b, 3), "ratio": round(a / b, 3),
                      "line_values_default_ms": round(default_ms, 3),
                      "line_vars_ms_rounds": [round(x, 3) for x in a_ms],
                      "line_values_ms_rounds": [round(x, 3) for x in b_ms],
                      "variants_resident_ms": round(c_ms, 3), "resident_chunks": len(res.chunks),
                      "variants_resident_lines_per_s": round(L / (c_ms / 1e3)),
                      **{k: round(v, 3) for k, v in parts.items()},
                      "table_rows_before_purge": rows_n, "table_rows_after_purge": rows_n - out["purged"],
                      "winners": int(win.numel()), "example_lines": fed.example_lines,
                      "report_fields": rep["fields"], "report_unbounded": rep["unboundedFields"],
                      "report_templates": rep["templates"], "report_tokens": rep["tokens"],
                      "planted_field_first": "upstream returned status" in top.get("example", "") and top.get("field") == 0,
                      "rare_value_found": rare.get("token") == facts["rare"] and lo < rare.get("firstLine", 0) <= hi}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
