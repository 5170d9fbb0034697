"""Correlation passes on a resident 1M-line document: the key kernel in its pass-2 form next to the
novelty kernel on the same text, its pass-1 form, and the rate of the whole report.

The document is ``utils.synth.correlated_log``: the templated log of ``bench_novelty.py`` with a
`` rid=<16 hex>`` field on its lines, ``--lines / 100`` interleaved requests of which a tenth fail
-- one failing request in about a thousand lines. The failing lines are the event lines.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``line_keys_ms``     (a) ``K.line_keys(table=on_event)``, the pass-2 form (k_line_keys: walk every
                       line, probe the table of the event keys with each of its up to eight keys,
                       compact the pairs found; one counter read);
* ``novel_lines_ms``   (b) ``K.novel_lines`` of the same text against a baseline that holds every
                       template (k_novel_sig walks the same bytes, probes once per line and writes
                       next to nothing);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``pass1_ms``         (c) ``K.line_keys(sel=event lines)``, the pass-1 form, kernel call alone;
* ``correlate_resident_lines_per_s``  (d) ``correlate_stream`` of the document as a resident log:
                       both passes, matchers included, and the report.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_correlate.py --rounds 1 --steps 3 --warmup 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from log_parser_amd.correlate import correlate_stream  # noqa: E402
from log_parser_amd.engine import Engine  # noqa: E402
from log_parser_amd.models.compiled import CompiledLibrary  # noqa: E402
from log_parser_amd.models.schema import PatternSet  # noqa: E402
from log_parser_amd.novelty import Baseline  # noqa: E402
from log_parser_amd.ops import kernels as K  # noqa: E402
from log_parser_amd.parallel.stream import ResidentLog  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import correlated_log, log_templates, realistic_library  # noqa: E402


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
        print("bench_correlate: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    sets = sets + [PatternSet.model_validate({"metadata": {"library_id": "correlate"}, "patterns": [
        {"id": "aborted", "name": "request aborted", "severity": "HIGH",
         "primary_pattern": {"regex": r"request aborted:", "confidence": 0.9}}]})]
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, failing = correlated_log(args.lines, log_templates(args.templates, seed=11), max(1, args.lines // 100), seed=5,
                                  fail_rate=0.1)
    data = log.encode()
    base = Baseline(eng)
    base.add_document(data)
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    ev = torch.tensor(sorted(at[-1] for at in failing.values()), dtype=torch.int32, device=dev)
    out = {}

    def pass1():
        out["c"] = K.line_keys(text, ls, ll, sel=ev)

    pass1()
    on_event = K.GapTable(dev)
    on_event.fold(out["c"][1], out["c"][0].long(), winners=False)

    def pass2():
        out["a"] = K.line_keys(text, ls, ll, table=on_event)

    def novel():
        out["b"] = K.novel_lines(text, ls, ll, base.table)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(pass2, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(novel, args.warmup, args.steps, dev))
    c_ms = _median_ms(pass1, args.warmup, args.steps, dev)
    pairs, held = out["a"][3]
    same = pairs == held == sum(len(at) for at in failing.values()) and out["c"][3] == (len(failing), len(failing))
    res = ResidentLog.load(data, eng)

    def report():
        out["d"] = correlate_stream(eng, res, top=5)

    d_ms = _median_ms(report, 1, max(3, args.steps // 2), dev)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    rep = out["d"]
    print(json.dumps({"config": f"correlate-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "requests": max(1, args.lines // 100),
                      "event_lines": ev.numel(), "event_keys": on_event.used, "key_pairs": pairs, "key_lines": held,
                      "novel_lines": out["b"][3][1],
                      "line_keys_ms": round(a, 3), "novel_lines_ms": round(b, 3), "ratio": round(a / b, 3),
                      "line_keys_ms_rounds": [round(x, 3) for x in a_ms],
                      "novel_lines_ms_rounds": [round(x, 3) for x in b_ms], "pass1_ms": round(c_ms, 3),
                      "pairs_as_constructed": same,
                      "correlate_resident_ms": round(d_ms, 3), "resident_chunks": len(res.chunks),
                      "correlate_resident_lines_per_s": round(L / (d_ms / 1e3)),
                      "report_event_lines": rep["eventLines"], "report_keys": rep["keys"],
                      "report_key_lines": rep["keyLines"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
