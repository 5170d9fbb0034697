"""Pauses report on a resident 1M-line document: the pause scan next to the timeline's fill (the
nearest existing scan: the same reads, one output column instead of rows), and the rate of the whole
report next to the trends report of the same resident log.

The document is ``utils.synth.pause_log``: the templated log of ``bench_novelty.py`` on a clock of
its own, with planted silences of 5 s and more.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``pause_scan_ms``    (a) ``K.pause_scan`` of the document's stamps and signatures at ``--min-ms``
                       (k_ps_tiles, k_ps_prefix, the read of the row count and the carry, k_ps_emit);
* ``timeline_fill_ms`` (b) ``K.timeline_fill`` of the same stamps (k_tl_tiles, k_tl_prefix, k_tl_fill;
                       no read);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``pause_scan_all_rows_ms``  (a) at ``min_ms=1``: nearly every step becomes a row -- what the row
                       writes cost at most;
* ``pause_scan_given_ms``  (a) with the statistics and the histogram passed in, as the accumulator
                       calls it: without the two small tensors a bare call makes;
* ``pauses_resident_lines_per_s``  ``pauses_stream`` of the document as a resident log: stamps, the
                       scan, the template fold, the groups and the report; next to it
                       ``trends_resident_lines_per_s`` of the same resident log in the same call.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_pauses.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.pauses import pauses_stream  # noqa: E402
from log_parser_amd.trends import trends_stream  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import log_templates, pause_log, realistic_library  # noqa: E402


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
    ap.add_argument("--min-ms", type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_pauses: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, planted = pause_log(args.lines, log_templates(args.templates, seed=11), seed=5, pauses=12)
    data = log.encode()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    sig, ts = K.line_stamps(text, ls, ll)
    out = {}

    def scan(min_ms=args.min_ms):
        out["a"] = K.pause_scan(ts, sig, min_ms)

    def fill():
        out["b"] = K.timeline_fill(ts)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(scan, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(fill, args.warmup, args.steps, dev))
    rows, stats, hist, carry = out["a"]
    few = max(3, args.steps // 2)
    all_ms = _median_ms(lambda: scan(1), 1, few, dev)
    all_rows = int(out["a"][0][0].numel())
    run_stats, run_hist = K.pause_stats(dev), torch.zeros(K.PS_BUCKETS, dtype=torch.int64, device=dev)
    given_ms = _median_ms(lambda: K.pause_scan(ts, sig, args.min_ms, stats=run_stats, hist=run_hist), args.warmup, args.steps, dev)
    res = ResidentLog.load(data, eng)

    def report():
        out["e"] = pauses_stream(eng, res, min_ms=args.min_ms, top=5)

    e_ms = _median_ms(report, 1, few, dev)
    t_ms = _median_ms(lambda: trends_stream(eng, res, top=5), 1, few, dev)
    rep = out["e"]
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    print(json.dumps({"config": f"pauses-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "min_ms": args.min_ms,
                      "pause_scan_ms": round(a, 3), "timeline_fill_ms": round(b, 3), "ratio": round(a / b, 3),
                      "pause_scan_ms_rounds": [round(x, 3) for x in a_ms], "timeline_fill_ms_rounds": [round(x, 3) for x in b_ms],
                      "scan_rows": int(rows[0].numel()), "scan_stamped": int(stats[K.PS_STAMPED]),
                      "pause_scan_all_rows_ms": round(all_ms, 3), "all_rows": all_rows,
                      "pause_scan_given_ms": round(given_ms, 3),
                      "pauses_resident_ms": round(e_ms, 3), "resident_chunks": len(res.chunks),
                      "pauses_resident_lines_per_s": round(L / (e_ms / 1e3)),
                      "trends_resident_ms": round(t_ms, 3), "trends_resident_lines_per_s": round(L / (t_ms / 1e3)),
                      "report_pauses": rep["pauses"], "report_paused_ms": rep["pausedMs"],
                      "planted_lead_longest": [r["ms"] for r in rep["longest"]] == [p[0] for p in planted[:5]]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
