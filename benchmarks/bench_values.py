"""Values report on a resident 1M-line document: the value kernel next to the key kernel on the same
text, the rate of the whole report, and where the report's time goes.

The document is ``utils.synth.metric_log``: the templated log of ``bench_novelty.py`` with a
``served request in <n>ms`` line on about a tenth of its lines and a burst of slow requests at 80 %.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``line_values_ms``   (a) ``K.line_values`` (k_line_vals: walk every line once for its template
                       signature and its numeric fields, compact the (line, key, value) triples;
                       one counter read);
* ``line_keys_ms``     (b) ``K.line_keys`` of the same text without a table (k_line_keys walks the
                       same bytes and emits 0..8 (line, key) pairs per line);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``values_resident_lines_per_s``  (c) ``values_stream`` of the document as a resident log: the
                       kernel, the five folds, the sums and the report;
* ``fold_*_ms`` / ``sum_ms``  the steps of one chunk of (c) on the whole document's triples, each
                       into a fresh table: the five ``GapTable`` folds and the torch sum step
                       (``unique`` + ``index_add_`` + merge);
* ``report_ms``        ``ValueAccumulator.report(top=5)`` alone, of an accumulator that holds the
                       document: the tables' rows, the host's filters and order.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_values.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import log_templates, metric_log, realistic_library  # noqa: E402
from log_parser_amd.values import ValueAccumulator, values_stream  # noqa: E402


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_values: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, burst = metric_log(args.lines, log_templates(args.templates, seed=11), seed=5)
    data = log.encode()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    out = {}

    def vals():
        out["a"] = K.line_values(text, ls, ll)

    def keys():
        out["b"] = K.line_keys(text, ls, ll)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(vals, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(keys, args.warmup, args.steps, dev))
    sig, line, key, value, (triples, held) = out["a"]
    res = ResidentLog.load(data, eng)

    def report():
        out["c"] = values_stream(eng, res, top=5)

    c_ms = _median_ms(report, 1, max(3, args.steps // 2), dev)
    rep = out["c"]
    # the steps of ValueAccumulator._add_piece on the whole document's triples, each into a fresh table
    g, v = line.long(), value.long()
    at = (g << 30) | v
    every = torch.arange(L, dtype=torch.int64, device=dev)
    steps = {"fold_lines": (sig, every, False), "fold_lo": (key, v, False),
             "fold_hi": (key, -((v << 32) | (0xFFFFFFFF - g)), False), "fold_first": (key, at, True),
             "fold_last": (key, -at, False)}
    parts = {}
    for name, (k, o, win) in steps.items():
        parts[name + "_ms"] = round(_median_ms(lambda: K.GapTable(dev).fold(k, o, winners=win), 1, max(3, args.steps // 2), dev), 3)
    acc = ValueAccumulator(eng)

    def sums():
        uk, inv = torch.unique(key, return_inverse=True)
        part = torch.zeros(uk.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, v)
        allk, inv2 = torch.unique(torch.cat([acc._sum_key, uk]), return_inverse=True)
        out["s"] = torch.zeros(allk.numel(), dtype=torch.int64, device=dev).index_add_(0, inv2, torch.cat([acc._sum, part]))

    parts["sum_ms"] = round(_median_ms(sums, 1, max(3, args.steps // 2), dev), 3)
    fed = ValueAccumulator(eng)
    fed.add_resident(res)
    parts["report_ms"] = round(_median_ms(lambda: fed.report(top=5), 1, max(3, args.steps // 2), dev), 3)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    top = rep["top"][0] if rep["top"] else {}
    print(json.dumps({"config": f"values-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "triples": triples, "value_lines": held,
                      "triples_per_line": round(triples / max(1, L), 3), "key_pairs": out["b"][3][0],
                      "line_values_ms": round(a, 3), "line_keys_ms": round(b, 3), "ratio": round(a / b, 3),
                      "line_values_ms_rounds": [round(x, 3) for x in a_ms],
                      "line_keys_ms_rounds": [round(x, 3) for x in b_ms],
                      "values_resident_ms": round(c_ms, 3), "resident_chunks": len(res.chunks),
                      "values_resident_lines_per_s": round(L / (c_ms / 1e3)), **parts,
                      "report_fields": rep["fields"], "report_templates": rep["templates"], "report_values": rep["values"],
                      "planted_field_first": "served request in" in top.get("example", ""),
                      "max_line_in_burst": (top.get("maxLine", 0) - 1) in burst}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
