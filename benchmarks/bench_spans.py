"""Spans report on a resident 1M-line document: the span kernel next to the two launches it
replaces on the same text, the table steps each on its own, and the rate of the whole report next to
``variants`` and ``cadence`` from the same run.

The document is ``utils.synth.span_log``: interleaved requests of three kinds, every line of a
request carrying its id, one request that never closes, one far longer than the rest, a host token on
every line, some unstamped continuation lines and a few out-of-order stamps.

Needs a GPU: the times are device-event times, there is no CPU fallback. Prints one JSON line:

* ``span_keys_ms``     (a) ``K.span_keys`` (k_span_keys: one visit per line for its stamp, its
                       template signature and its keys with their places; one counter read);
* ``keys_plus_stamps_ms``  (b) ``K.line_keys`` (every line, no table) plus ``K.line_stamps`` of the
                       same text: the two launches, and the two walks over the text, that (a)
                       replaces (``line_keys_ms`` / ``line_stamps_ms``: each alone);
                       all with room for 4 pairs per line, so that no call walks twice;
* ``ratio``            (a) / (b), from the medians of ``--rounds`` alternating rounds (a, b, a, b, ...),
                       each round the median of ``--steps`` calls; every round's median is listed;
* ``fold_ms`` / ``ends_ms`` / ``rows_ms``  the table steps on the whole document's pairs, each on its
                       own: k_span_fold into a fresh table sized for them (the allocation of the
                       table is in ``table_alloc_ms`` and taken off), k_span_ends after it, and the
                       read of the rows (k_span_rows);
* ``fill_ms`` / ``fold_lines_ms``  the other steps of a piece: ``K.timeline_fill`` and the template fold;
* ``purge_ms``         ``SpanTable.purge(1)`` of the full table (about half of the ids leave);
* ``report_ms``        ``SpanAccumulator.report()`` alone, of an accumulator that holds the document;
* ``spans_resident_lines_per_s`` / ``variants_...`` / ``cadence_...``  the three reports of the document
                       as a resident log, in the same run.

Kernel times come from a separate traced run, e.g.
``rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/bench_spans.py --rounds 1 --steps 3 --warmup 1``.
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
from log_parser_amd.native import N  # noqa: E402
from log_parser_amd.ops import kernels as K  # noqa: E402
from log_parser_amd.parallel.stream import ResidentLog  # noqa: E402
from log_parser_amd.spans import SpanAccumulator, spans_stream  # noqa: E402
from log_parser_amd.utils.config import Config, ScoringParams  # noqa: E402
from log_parser_amd.utils.synth import realistic_library, span_log  # noqa: E402
from log_parser_amd.variants import variants_stream  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_spans: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    sets, _ = realistic_library(256, seed=7)
    eng = Engine(CompiledLibrary(sets, ScoringParams()), Config.load(overrides={"engine.device": str(dev)}), device=dev)
    log, facts = span_log(args.lines, seed=5)
    data = log.encode()
    text, n = eng.stage_text(data)
    ls, ll = K.split_lines(text, n)
    L = ls.numel()
    out = {}
    room = 4 * L        # one pass each

    def spans_():
        out["a"] = K.span_keys(text, ls, ll, cap=room)

    def keys():
        out["k"] = K.line_keys(text, ls, ll, cap=room)

    def stamps():
        out["s"] = K.line_stamps(text, ls, ll)

    def both():
        keys()
        stamps()

    a_ms, b_ms = [], []
    for _ in range(args.rounds):
        a_ms.append(_median_ms(spans_, args.warmup, args.steps, dev))
        b_ms.append(_median_ms(both, args.warmup, args.steps, dev))
    k_ms = _median_ms(keys, args.warmup, args.steps, dev)
    s_ms = _median_ms(stamps, args.warmup, args.steps, dev)
    sig, ts, line, key, tok, (pairs, held) = out["a"]
    few = max(3, args.steps // 2)
    parts = {"fill_ms": _median_ms(lambda: out.__setitem__("eff", K.timeline_fill(ts)[0]), 1, few, dev)}
    eff = out["eff"]
    every = torch.arange(L, dtype=torch.int64, device=dev)
    parts["fold_lines_ms"] = _median_ms(lambda: K.GapTable(dev).fold(sig, every, winners=False), 1, few, dev)
    cap = K.SpanTable._fit(1 << 12, 0, pairs)
    pack = (line.data_ptr(), key.data_ptr(), tok.data_ptr(), pairs, sig.data_ptr(), eff.data_ptr(), L, text.data_ptr(),
            text.numel(), ls.data_ptr(), 0)

    def fold():
        t = K.SpanTable(dev, cap=cap)
        N.span_fold(t._tab(), pack, K._s(text), True)
        out["t"] = t

    parts["table_alloc_ms"] = _median_ms(lambda: K.SpanTable(dev, cap=cap), 1, few, dev)
    parts["fold_ms"] = max(0.0, _median_ms(fold, 1, few, dev) - parts["table_alloc_ms"])
    full = out["t"]
    parts["ends_ms"] = _median_ms(lambda: N.span_ends(full._tab(), pack, K._s(text), True), 1, few, dev)
    full._bound = pairs
    parts["rows_ms"] = _median_ms(lambda: out.__setitem__("rows", full.rows()), 1, few, dev)
    rows = out["rows"]
    rows_n = rows[0].numel()

    def purge():
        t = K.SpanTable(dev, cap=cap)           # the table as the fold left it: re-inserted, then purged
        t._reinsert(rows, rows_n)
        t._bound = rows_n
        out["purged"] = t.purge(1)

    def refill():
        t = K.SpanTable(dev, cap=cap)
        t._reinsert(rows, rows_n)

    # (the purge is timed with the re-insert that sets it up, and that re-insert alone is taken off)
    parts["purge_ms"] = max(0.0, _median_ms(purge, 1, few, dev) - _median_ms(refill, 1, few, dev))
    res = ResidentLog.load(data, eng)
    fed = SpanAccumulator(eng)
    fed.add_resident(res)
    parts["report_ms"] = _median_ms(lambda: out.__setitem__("rep", fed.report()), 1, few, dev)
    rep = out["rep"]
    rates = {}
    for name, fn in (("spans", lambda: spans_stream(eng, res)), ("variants", lambda: variants_stream(eng, res, top=5)),
                     ("cadence", lambda: cadence_stream(eng, res, top=5))):
        ms = _median_ms(fn, 1, few, dev)
        rates[name + "_resident_ms"] = round(ms, 3)
        rates[name + "_resident_lines_per_s"] = round(L / (ms / 1e3))
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    unfinished = [k for k in rep["kinds"] if k["unfinished"]]
    print(json.dumps({"config": f"spans-{L}-lines", "bytes": n, "lines": L, "steps": args.steps, "rounds": args.rounds,
                      "pairs": pairs, "id_lines": held, "pairs_per_line": round(pairs / max(1, L), 3), "ids": rows_n,
                      "span_keys_ms": round(a, 3), "keys_plus_stamps_ms": round(b, 3), "ratio": round(a / b, 3),
                      "line_keys_ms": round(k_ms, 3), "line_stamps_ms": round(s_ms, 3),
                      "span_keys_ms_rounds": [round(x, 3) for x in a_ms],
                      "keys_plus_stamps_ms_rounds": [round(x, 3) for x in b_ms],
                      **{k: round(v, 3) for k, v in parts.items()}, "purged": out["purged"], "table_cap": cap,
                      "resident_chunks": len(res.chunks), **rates,
                      "report_listed": rep["listed"], "report_shift": rep["sampleShift"],
                      "long_span_first": bool(rep["top"]) and rep["top"][0]["key"] == facts["long"],
                      "unfinished_kinds": len(unfinished), "unfinished_spans": sum(k["unfinished"] for k in unfinished)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
