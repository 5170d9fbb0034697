"""Novelty pass on a resident 1M-line document: the one-pass kernel next to the composition the
tree could run without it, and the rate at which a baseline is built.

The document is made of a fixed set of a few hundred templates with varying numbers
(``utils.synth.templated_log``; ``make_log``'s noise lines are nearly all distinct templates, which
is not what logs look like). The baseline is built from a sibling document that lacks some of the
templates, so that a few percent of the lines are novel.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``novel_lines_ms``   (a) ``K.novel_lines`` (k_novel_sig: sign, probe, compact; one counter read);
* ``composition_ms``   (b) ``K.line_signatures`` over every line, ``torch.isin`` against the
                       baseline's sorted signatures, ``nonzero``;
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed, so
                       the run-to-run spread is in the output;
* ``baseline_lines_per_s``  (c) ``Baseline.add_resident`` of the same document into an empty baseline.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_novelty.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import log_templates, realistic_library, templated_log  # noqa: E402


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
        print("bench_novelty: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    temps = log_templates(args.templates, seed=11)
    # the sibling lacks every tenth template from the 30th on: ~4 % of the lines with 300 templates
    healthy = [t for k, t in enumerate(temps) if k < 29 or k % 10 != 9]
    data = templated_log(args.lines, temps, seed=5).encode()
    sibling = templated_log(args.lines // 4, healthy, seed=6).encode()
    base = Baseline(eng)
    base.add_document(sibling)
    base_sig = base.signatures()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    out = {}

    def novel():
        out["a"] = K.novel_lines(text, ls, ll, base.table)

    def composition():
        sig = K.line_signatures(text, ls, ll)
        out["b"] = (~torch.isin(sig, base_sig)).nonzero().flatten()

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(novel, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(composition, args.warmup, args.steps, dev))
    line, _, _, (_, n_novel, _) = out["a"]
    same = torch.equal(torch.sort(line.long())[0], out["b"])
    res = ResidentLog.load(data, eng)

    def build():
        b = Baseline(eng)
        b.add_resident(res)
        out["c"] = b

    c_ms = _median_ms(build, 1, max(3, args.steps // 2), dev)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    print(json.dumps({"config": f"novelty-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "novel_lines": n_novel,
                      "novel_share": round(n_novel / max(L, 1), 4), "baseline_templates": base.templates,
                      "novel_lines_ms": round(a, 3), "composition_ms": round(b, 3), "ratio": round(a / b, 3),
                      "novel_lines_ms_rounds": [round(x, 3) for x in a_ms],
                      "composition_ms_rounds": [round(x, 3) for x in b_ms], "same_lines": same,
                      "baseline_add_resident_ms": round(c_ms, 3), "baseline_chunks": len(res.chunks),
                      "baseline_lines_per_s": round(L / (c_ms / 1e3)),
                      "baseline_built_templates": out["c"].templates}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
