"""Trends report on a resident 1M-line document: the fused stamp-and-signature kernel next to the two
kernels it replaces, the cell fold next to a plain signature fold, the rate of the whole report, and
where the report's time goes.

The document is ``utils.synth.trend_log``: the templated log of ``bench_novelty.py`` on a clock of
its own, with a heartbeat that stops, an error that starts and a line that surges at 75 %.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``line_stamps_ms``   (a) ``K.line_stamps`` (k_line_stamps: one visit of every line for its stamp
                       and its template signature);
* ``pair_ms``          (b) ``K.line_signatures`` followed by ``K.line_timestamps`` of the same text
                       (k_gap_sig and k_ts_parse: two launches that each fetch the line index and
                       the text);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``cell_fold_ms``     (c) one ``CellTable.fold`` of the document's lines into a fresh table;
* ``gap_fold_ms``      (d) one ``GapTable.fold(sig, g, winners=False)`` of the same lines into a
                       fresh table; ``fold_ratio`` = (c) / (d), rounds as above;
* ``trends_resident_lines_per_s``  (e) ``trends_stream`` of the document as a resident log: the
                       kernel, the fill, the two folds and the report; next to it
                       ``values_resident_lines_per_s`` of the same resident log in the same call;
* ``fill_ms``          ``K.timeline_fill`` of the document's stamps;
* ``report_ms``        ``TrendAccumulator.report(top=5)`` alone, of an accumulator that holds the
                       document; ``report_rows_ms`` the table's rows, ``report_sort_ms`` the two
                       stable sorts of the cells in it.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_trends.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.trends import TrendAccumulator, trends_stream  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import log_templates, realistic_library, trend_log  # noqa: E402
from log_parser_amd.values import values_stream  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bucket", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_trends: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, planted = trend_log(args.lines, log_templates(args.templates, seed=11), seed=5)
    data = log.encode()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    W = 1000 * args.bucket
    out = {}

    def fused():
        out["a"] = K.line_stamps(text, ls, ll)

    def pair():
        out["b"] = (K.line_signatures(text, ls, ll), K.line_timestamps(text, ls, ll))

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(fused, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(pair, args.warmup, args.steps, dev))
    sig, ts = out["a"]
    same = bool(torch.equal(sig, out["b"][0]) and torch.equal(ts, out["b"][1]))
    few = max(3, args.steps // 2)
    fill_ms = _median_ms(lambda: out.__setitem__("eff", K.timeline_fill(ts)[0]), 1, few, dev)
    eff = out["eff"]
    g = torch.arange(L, dtype=torch.int64, device=dev)
    c_ms, d_ms = [], []
    for _ in range(args.rounds):
        c_ms.append(_median_ms(lambda: K.CellTable(dev).fold(sig, eff, 0, W), 1, few, dev))
        d_ms.append(_median_ms(lambda: K.GapTable(dev).fold(sig, g, winners=False), 1, few, dev))
    res = ResidentLog.load(data, eng)

    def report():
        out["e"] = trends_stream(eng, res, bucket_seconds=args.bucket, top=5)

    e_ms = _median_ms(report, 1, few, dev)
    v_ms = _median_ms(lambda: values_stream(eng, res, top=5), 1, few, dev)
    rep = out["e"]
    fed = TrendAccumulator(eng, args.bucket)
    fed.add_resident(res)
    report_ms = _median_ms(lambda: fed.report(top=5), 1, few, dev)
    rows_ms = _median_ms(lambda: out.__setitem__("rows", fed.cells.rows()), 1, few, dev)
    r_sig, r_bucket = out["rows"][:2]

    def sorts():
        o = torch.sort(r_bucket, stable=True)[1]
        out["o"] = o[torch.sort(r_sig[o], stable=True)[1]]

    sort_ms = _median_ms(sorts, 1, few, dev)
    a, b, c, d = (statistics.median(x) for x in (a_ms, b_ms, c_ms, d_ms))
    kinds = [r["kind"] for r in rep["top"][:3]]
    print(json.dumps({"config": f"trends-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "bucket_seconds": args.bucket,
                      "line_stamps_ms": round(a, 3), "pair_ms": round(b, 3), "ratio": round(a / b, 3),
                      "line_stamps_ms_rounds": [round(x, 3) for x in a_ms], "pair_ms_rounds": [round(x, 3) for x in b_ms],
                      "fused_equals_pair": same,
                      "cell_fold_ms": round(c, 3), "gap_fold_ms": round(d, 3), "fold_ratio": round(c / d, 3),
                      "cell_fold_ms_rounds": [round(x, 3) for x in c_ms], "gap_fold_ms_rounds": [round(x, 3) for x in d_ms],
                      "fill_ms": round(fill_ms, 3),
                      "trends_resident_ms": round(e_ms, 3), "resident_chunks": len(res.chunks),
                      "trends_resident_lines_per_s": round(L / (e_ms / 1e3)),
                      "values_resident_ms": round(v_ms, 3), "values_resident_lines_per_s": round(L / (v_ms / 1e3)),
                      "report_ms": round(report_ms, 3), "report_rows_ms": round(rows_ms, 3), "report_sort_ms": round(sort_ms, 3),
                      "report_cells": rep["cells"], "report_templates": rep["templates"], "report_buckets": rep["buckets"],
                      "top_kinds": kinds,
                      "planted_in_top": sorted(p.split("%d")[0] in r["example"] for r in rep["top"][:3] for p in planted).count(True)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
