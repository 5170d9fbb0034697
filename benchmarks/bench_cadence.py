"""Cadence report on a resident 1M-line document: the beat scan next to the pause scan on the same
stamps and signatures (the nearest existing scan: the same reads, one clock for the whole log instead
of one per template), the share of its three steps, and the rate of the whole report next to the
pauses report of the same resident log.

The document is ``utils.synth.cadence_log``: the templated log of ``bench_pauses.py`` on a clock of
its own, with three periodic lines planted in it.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``beat_scan_ms``     (a) ``K.beat_scan`` of the document's stamps and signatures without a state
                       (k_cd_tile, the read of the row count, the two torch sorts, k_cdl_tiles,
                       k_cdl_prefix, k_cdl_emit, the read of the state's row count);
* ``pause_scan_ms``    (b) ``K.pause_scan`` of the same columns at ``min_ms=1000``;
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``line_stamps_ms``   ``K.line_stamps`` of the same lines: the walk over the text that feeds both;
* ``tile_ms`` / ``sort_ms`` / ``link_ms``  the three steps of (a), each timed alone on the inputs the
                       step before it left, and their shares of the sum;
* ``tile_rows`` / ``state_rows``  the rows k_cd_tile wrote and the templates they join into;
* ``cadence_resident_lines_per_s``  ``cadence_stream`` of the document as a resident log: stamps, the
                       scan with the state carried, the cell fold, the template fold and the report;
                       next to it ``pauses_resident_lines_per_s`` of the same resident log in the
                       same call.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_cadence.py --rounds 1 --steps 3 --warmup 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from log_parser_amd.cadence import cadence_stream  # noqa: E402
from log_parser_amd.engine import Engine  # noqa: E402
from log_parser_amd.models.compiled import CompiledLibrary  # noqa: E402
from log_parser_amd.ops import kernels as K  # noqa: E402
from log_parser_amd.parallel.stream import ResidentLog  # noqa: E402
from log_parser_amd.pauses import pauses_stream  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import cadence_log, log_templates, realistic_library  # noqa: E402


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
        print("bench_cadence: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, known = cadence_log(args.lines, log_templates(args.templates, seed=11), seed=5)
    data = log.encode()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    sig, ts = K.line_stamps(text, ls, ll)
    out = {}

    def beats():
        out["a"] = K.beat_scan(ts, sig)

    def pauses():
        out["b"] = K.pause_scan(ts, sig, 1000)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(beats, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(pauses, args.warmup, args.steps, dev))
    stamps_ms = _median_ms(lambda: K.line_stamps(text, ls, ll), args.warmup, args.steps, dev)
    # the three steps alone, each on what the step before it left
    beat, bkt = torch.empty_like(ts), torch.empty_like(ts)
    tile_ms = _median_ms(lambda: out.__setitem__("rows", K.beat_tile_rows(ts, sig, 0, beat, bkt)), args.warmup, args.steps, dev)
    sort_ms = _median_ms(lambda: out.__setitem__("sorted", K.beat_sort_rows(out["rows"])), args.warmup, args.steps, dev)
    link_ms = _median_ms(lambda: out.__setitem__("state", K.beat_link_rows(out["sorted"], 0, beat, bkt)), args.warmup,
                         args.steps, dev)
    parts = tile_ms + sort_ms + link_ms
    same = bool(torch.equal(out["state"], out["a"][2]) and torch.equal(beat, out["a"][0]) and torch.equal(bkt, out["a"][1]))
    few = max(3, args.steps // 2)
    res = ResidentLog.load(data, eng)

    def report():
        out["e"] = cadence_stream(eng, res, top=5)

    e_ms = _median_ms(report, 1, few, dev)
    p_ms = _median_ms(lambda: pauses_stream(eng, res, top=5), 1, few, dev)
    rep = out["e"]
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    hole = known["hole"]
    print(json.dumps({"config": f"cadence-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds,
                      "beat_scan_ms": round(a, 3), "pause_scan_ms": round(b, 3), "ratio": round(a / b, 3),
                      "beat_scan_ms_rounds": [round(x, 3) for x in a_ms], "pause_scan_ms_rounds": [round(x, 3) for x in b_ms],
                      "line_stamps_ms": round(stamps_ms, 3),
                      "tile_ms": round(tile_ms, 3), "sort_ms": round(sort_ms, 3), "link_ms": round(link_ms, 3),
                      "tile_share": round(tile_ms / parts, 3), "sort_share": round(sort_ms / parts, 3),
                      "link_share": round(link_ms / parts, 3),
                      "tile_rows": int(out["rows"].shape[1]), "state_rows": int(out["state"].shape[1]),
                      "steps_equal_scan": same,
                      "cadence_resident_ms": round(e_ms, 3), "resident_chunks": len(res.chunks),
                      "cadence_resident_lines_per_s": round(L / (e_ms / 1e3)),
                      "pauses_resident_ms": round(p_ms, 3), "pauses_resident_lines_per_s": round(L / (p_ms / 1e3)),
                      "report_periodic": rep["periodic"], "report_missed": rep["missed"], "report_stopped": rep["stopped"],
                      "planted_hole_found": any(r["maxMs"] == hole["maxMs"] and r["toLine"] - 1 == hole["toLine"]
                                                for r in rep["top"])}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
