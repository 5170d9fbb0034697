"""Lead-up pass on a resident 1M-line document: the sign-and-mark kernel next to the novelty kernel
on the same text, and the rate of the whole report.

The document is the templated log of ``bench_novelty.py`` (a few hundred fixed templates with
varying numbers, ``utils.synth.templated_log``). The event lines of (a) are planted: one about
every ``--event-every`` lines at random places, so that with ``--window 50`` about a twentieth of
the lines is in the lead-up.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``lead_lines_ms``    (a) ``K.lead_lines`` (k_lead_sig: sign every line, search the event list, write
                       9 bytes per line, compact the lead-up lines; one counter read);
* ``novel_lines_ms``   (b) ``K.novel_lines`` of the same text against a baseline that holds every
                       template (k_novel_sig signs every line too, probes, and writes next to nothing);
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``leadup_resident_lines_per_s``  (c) ``LeadupAccumulator.add_resident`` + ``report`` of the same
                       document with a line that the library matches planted on every event line of
                       (a), matchers included.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_leadup.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.leadup import LeadupAccumulator  # noqa: E402
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
    ap.add_argument("--event-every", type=int, default=1000)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_leadup: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, trig = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    temps = log_templates(args.templates, seed=11)
    data = templated_log(args.lines, temps, seed=5).encode()
    # the novelty pass next to it: a baseline of the document itself, so it holds every template
    base = Baseline(eng)
    base.add_document(data)
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    g = torch.Generator().manual_seed(3)
    ev = torch.unique(torch.randint(0, L, (max(1, L // args.event_every),), generator=g)).to(dtype=torch.int32, device=dev)
    out = {}

    def lead():
        out["a"] = K.lead_lines(text, ls, ll, ev, args.window)

    def novel():
        out["b"] = K.novel_lines(text, ls, ll, base.table)

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(lead, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(novel, args.warmup, args.steps, dev))
    sig, mark, line, _, n_lead = out["a"]
    same = int(mark.sum()) == n_lead == line.numel() and torch.equal(sig, K.line_signatures(text, ls, ll))
    n_novel = out["b"][3][1]
    # (c): the same document with a line the library matches planted on every event line of (a)
    rows = data.split(b"\n")
    for k, e in enumerate(ev.tolist()):
        sample = trig[k % len(trig)]["sample"]
        rows[e] = sample.encode() if sample[:1].isspace() else rows[e][:40] + b" " + sample.encode()
    res = ResidentLog.load(b"\n".join(rows), eng)

    def report():
        acc = LeadupAccumulator(eng, args.window)
        acc.add_resident(res)
        out["c"] = acc.report(top=5)

    c_ms = _median_ms(report, 1, max(3, args.steps // 2), dev)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    rep = out["c"]
    print(json.dumps({"config": f"leadup-{L}-lines-{args.templates}-templates", "bytes": n, "lines": L,
                      "steps": args.steps, "rounds": args.rounds, "window": args.window, "event_lines": ev.numel(),
                      "lead_lines": n_lead, "lead_share": round(n_lead / max(L, 1), 4), "novel_lines": n_novel,
                      "lead_lines_ms": round(a, 3), "novel_lines_ms": round(b, 3), "ratio": round(a / b, 3),
                      "lead_lines_ms_rounds": [round(x, 3) for x in a_ms],
                      "novel_lines_ms_rounds": [round(x, 3) for x in b_ms], "same_signatures": same,
                      "leadup_resident_ms": round(c_ms, 3), "resident_chunks": len(res.chunks),
                      "leadup_resident_lines_per_s": round(L / (c_ms / 1e3)),
                      "report_event_lines": rep["eventLines"], "report_lead_lines": rep["leadLines"],
                      "report_templates": rep["templates"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
