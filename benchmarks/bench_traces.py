"""Trace pass on a resident 1M-line document: the classify-and-scan kernels next to the novelty
kernel on the same text, and the rate of the whole report.

The document is a templated log (``utils.synth.templated_log``) with about a tenth of its lines
in stack traces planted from a few dozen sites with cause chains (``utils.synth.traced_log``).

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``trace_runs_ms``    (a) ``K.trace_runs`` (k_tr_class, then the scan k_tr_tiles / k_tr_prefix /
                       k_tr_emit; one read of the count and the carry);
* ``novel_lines_ms``   (b) ``K.novel_lines`` of the same text against a baseline of the plain
                       templates (k_novel_sig signs EVERY line; the trace pass signs only the frames);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``traces_resident_lines_per_s``  (c) ``TraceAccumulator.add_resident`` + ``report`` of the same
                       document, matchers included.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_traces.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.novelty import Baseline  # noqa: E402
from log_parser_amd.ops import kernels as K  # noqa: E402
from log_parser_amd.parallel.stream import ResidentLog  # noqa: E402
from log_parser_amd.traces import TraceAccumulator  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import log_templates, realistic_library, templated_log, trace_sites, traced_log  # noqa: E402


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
    ap.add_argument("--sites", type=int, default=36)
    ap.add_argument("--trace-share", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_traces: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    temps = log_templates(args.templates, seed=11)
    data = traced_log(args.lines, temps, trace_sites(args.sites, seed=3), seed=5, trace_share=args.trace_share).encode()
    # the novelty pass next to it: a baseline that knows the plain templates, so the trace lines are the novel ones
    base = Baseline(eng)
    base.add_document(templated_log(args.lines // 4, temps, seed=6).encode())
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    out = {}

    def runs():
        out["a"] = K.trace_runs(text, ls, ll, None, K.TR_CARRY_START, True)

    def novel():
        out["b"] = K.novel_lines(text, ls, ll, base.table)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(runs, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(novel, args.warmup, args.steps, dev))
    cols, (n_traces,), _ = out["a"]
    run_lines = int(cols[K.TR_LINES].sum())
    frame_lines = int(cols[K.TR_FRAMES].sum())
    n_novel = out["b"][3][1]
    res = ResidentLog.load(data, eng)

    def report():
        acc = TraceAccumulator(eng)
        acc.add_resident(res)
        out["c"] = acc.report(top=5)

    c_ms = _median_ms(report, 1, max(3, args.steps // 2), dev)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    rep = out["c"]
    print(json.dumps({"config": f"traces-{L}-lines-{args.sites}-sites", "bytes": n, "lines": L, "steps": args.steps,
                      "rounds": args.rounds, "traces": n_traces, "run_lines": run_lines, "frame_lines": frame_lines,
                      "trace_share": round(run_lines / max(L, 1), 4), "novel_lines": n_novel,
                      "trace_runs_ms": round(a, 3), "novel_lines_ms": round(b, 3), "ratio": round(a / b, 3),
                      "trace_runs_ms_rounds": [round(x, 3) for x in a_ms],
                      "novel_lines_ms_rounds": [round(x, 3) for x in b_ms],
                      "traces_resident_ms": round(c_ms, 3), "resident_chunks": len(res.chunks),
                      "traces_resident_lines_per_s": round(L / (c_ms / 1e3)),
                      "report_traces": rep["traces"], "report_groups": rep["groups"],
                      "same_traces": rep["traces"] == n_traces and rep["frameLines"] == frame_lines}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
