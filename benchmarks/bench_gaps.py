"""Coverage-gap report on a resident document (config 2's input: a 1M-line log, the 256-pattern
realistic library) next to ``Engine.run_document`` on the same document in the same process.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:
the median over ``--steps`` runs (after ``--warmup``) of ``Engine.gaps_document`` (everything of
``gaps_bytes`` after the text is staged) and of ``run_document``, and their ratio.

``--stream CHUNK_BYTES`` measures the chunked report instead (``GapAccumulator.add_stream`` +
``report``, what ``LogParser.gaps_stream`` runs) against ``gaps_document`` on the same data in the
same run. The stream starts from the host bytes, so its time includes staging and the H2D copies
that ``gaps_document`` (text already on the device) does not pay.

Kernel times (k_gap_sig, k_feat_cov; with ``--stream`` also k_gap_fold, k_gap_winners) come from a
separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_gaps.py --gaps-only --steps 3 --warmup 1``.
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
    ap.add_argument("--cover", choices=("events", "context"), default="context")
    ap.add_argument("--gaps-only", action="store_true", help="skip run_document (for a kernel trace of the report)")
    ap.add_argument("--stream", type=int, default=0, metavar="CHUNK_BYTES",
                    help="measure the chunked report (gaps_stream) against gaps_document")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_gaps: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, trig = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    data = make_log(args.lines, trig, seed=5, hit_rate=0.004, aux_rate=0.01, stack_rate=0.01).encode()
    text, n = eng.stage_text(data)
    rep = {}

    def gaps():
        rep.update(eng.gaps_document(text, n, data, top=20, cover=args.cover))

    def document():
        return eng.run_document(text, n)

    if args.stream:
        from log_parser_amd.gapreport import GapAccumulator
        srep = {}

        def stream():
            acc = GapAccumulator(eng, cover=args.cover)
            acc.add_stream(data, chunk_bytes=args.stream)
            srep.clear()
            srep.update(acc.report(top=20))

        s = _median_ms(stream, args.warmup, args.steps, dev)
        g = float("nan") if args.gaps_only else _median_ms(gaps, args.warmup, args.steps, dev)
        print(json.dumps({"config": f"gaps-stream-{args.lines}-lines-256-patterns", "bytes": n, "steps": args.steps,
                          "chunk_bytes": args.stream, "gaps_stream_ms": round(s, 3), "gaps_document_ms": round(g, 3),
                          "ratio": round(s / g, 3), "same_report": None if args.gaps_only else srep == rep,
                          "report": {k: v for k, v in srep.items() if k != "top"}}))
        return 0
    g = _median_ms(gaps, args.warmup, args.steps, dev)
    # (a kernel trace of the report alone: run_document's own k_feat_cov launches would mix in)
    d = _median_ms(document, args.warmup, args.steps, dev) if not args.gaps_only else float("nan")
    print(json.dumps({"config": f"gaps-{args.lines}-lines-256-patterns", "bytes": n, "steps": args.steps,
                      "gaps_document_ms": round(g, 3), "run_document_ms": round(d, 3), "ratio": round(g / d, 3),
                      "report": {k: v for k, v in rep.items() if k != "top"},
                      "top3": [(t["count"], t["template"][:60]) for t in rep["top"][:3]]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
