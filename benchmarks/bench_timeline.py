"""Timeline report on a resident document (a 1M-line log, the 256-pattern realistic library) next
to ``Engine.gaps_document`` and ``Engine.run_document`` on the same document in the same process.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line: the
median over ``--steps`` runs (after ``--warmup``) of ``Engine.timeline_document`` (everything of
``timeline_bytes`` after the text is staged), of ``gaps_document`` and of ``run_document``.

Kernel times (k_ts_parse, k_tl_hist, and k_nl_count of the line index on the same text as the
full-text-read yardstick) come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_timeline.py --timeline-only --steps 3 --warmup 1``.
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
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import make_log, realistic_library  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bucket", type=int, default=60, metavar="SECONDS")
    ap.add_argument("--timeline-only", action="store_true",
                    help="skip gaps_document and run_document (for a kernel trace of the report)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_timeline: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, trig = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    data = make_log(args.lines, trig, seed=5, hit_rate=0.004, aux_rate=0.01, stack_rate=0.01).encode()
    text, n = eng.stage_text(data)
    rep = {}

    def timeline():
        rep.update(eng.timeline_document(text, n, data, bucket_seconds=args.bucket))

    t = _median_ms(timeline, args.warmup, args.steps, dev)
    g = d = float("nan")
    if not args.timeline_only:
        g = _median_ms(lambda: eng.gaps_document(text, n, data, top=20), args.warmup, args.steps, dev)
        d = _median_ms(lambda: eng.run_document(text, n), args.warmup, args.steps, dev)
    print(json.dumps({"config": f"timeline-{args.lines}-lines-256-patterns", "bytes": n, "steps": args.steps,
                      "bucket_seconds": args.bucket, "timeline_document_ms": round(t, 3),
                      "gaps_document_ms": round(g, 3), "run_document_ms": round(d, 3),
                      "report": {k: v for k, v in rep.items() if k != "buckets"}, "buckets": len(rep["buckets"]),
                      "bucket0": rep["buckets"][0] if rep["buckets"] else None}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
