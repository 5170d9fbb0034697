"""Command line: ``python -m log_parser_amd <command>`` (also installed as ``log-parser-amd``).

  serve     [-Dkey=value ...]                  REST service (POST /parse, Parse.java:23-62)
  analyze   FILE [--patterns DIR] [--stream]   analyse one log file; prints the AnalysisResult
                                               JSON (or a stream summary + top-k for huge logs)
  validate  [DIR]                              compile a pattern library and report every regex
                                               that is invalid, unsupported on the device path,
                                               or routed to the host fallback (the reference only
                                               finds bad regexes per request, AnalysisService.java:64)
  gaps      FILE [FILE ...] [--patterns DIR] [--device D] [--top N] [--cover events|context] [--stream]
                                               the error lines of a log that no pattern of the
                                               library explains, grouped by line template (JSON);
                                               several files: the corpus report, in argument order;
                                               --stream: one file in chunks (any size)
  timeline  FILE [--patterns DIR] [--device D] [--bucket SECONDS] [--stream]
                                               when the lines, error lines and events of a log
                                               happened: the stamps at the head of its lines, counts
                                               per time bucket (JSON); --stream: in chunks (any size)
  novel     FILE (--baseline FILE [FILE ...] | --baseline-file B.npz) [--save-baseline B.npz]
            [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--top N]
            [--order count|first] [--errors-only]
                                               the lines of a log whose template a baseline of
                                               healthy logs never showed, grouped by template (JSON)
  traces    FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--top N]
            [--order count|first] [--unexplained-only]
                                               the stack traces of a log grouped by their frames and
                                               causes: how often, where first, the root cause, and
                                               whether an event lies on them (JSON)
  leadup    FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--window N] [--top N]
            [--order share|count|first] [--min-count N]
                                               the line templates that lie within a window of lines
                                               before the events of a log more often than elsewhere:
                                               what the log said just before each failure (JSON)
  correlate FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--min-length N]
            [--order events|lines|first] [--min-lines N] [--max-share F] [--top N]
                                               the ids on the event lines of a log (request ids,
                                               trace ids, pod hashes, addresses) followed through
                                               the log: which other lines hold them (JSON)
  values    FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--top N]
            [--order peak|max|count|first] [--min-count N] [--min-fill F] [--all-fields]
                                               the numeric fields of the line templates of a log:
                                               count, sum, min, max, and the line of the largest
                                               value -- the fields that peak first (JSON)
  variants  FILE... [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--max-distinct N]
            [--order odd|count|distinct|first] [--min-count N] [--min-fill F] [--all] [--show N]
            [--top N]
                                               the values that the variable tokens of the line
                                               templates take: how often, where first and last, the
                                               field with one deviant among thousands first; several
                                               files continue ONE log (JSON)
  spans     FILE... [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--min-length N]
            [--min-lines N] [--max-share F] [--min-ms N] [--order duration|lines|first]
            [--unfinished-only] [--max-ids N] [--top N] [--kinds N]
                                               the lifetimes of the ids of a log: the longest first,
                                               and the ones that never logged the line their kind
                                               usually ends on; several files continue ONE log (JSON)
  trends    FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--bucket S]
            [--at T|first-event|first-error] [--ratio R] [--min-count N] [--kind K] [--order O]
            [--top N]
                                               the line templates of a log that started, stopped,
                                               surged or faded across a pivot in the log's own
                                               time: what changed (JSON)
  pauses    FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--min-ms N]
            [--by before|after] [--order total|max|count|share|first] [--min-count N] [--top N]
                                               where the log went silent: the steps between its
                                               stamped lines, the long ones with the lines around
                                               them and grouped by the template in front (JSON)
  cadence   FILE [--patterns DIR] [--device D] [--stream] [--chunk-bytes N] [--min-ms N]
            [--ratio R] [--min-count N] [--min-regularity F] [--kind missed|stopped|all]
            [--order gap|overdue|count|first] [--top N]
                                               the line templates that come at a steady beat: where
                                               one missed beats while the log went on, and which
                                               stopped before the log ended (JSON)

Config keys use the reference names (``-Dpattern.directory=...``, env ``PATTERN_DIRECTORY``).
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
from typing import List, Optional

from .utils.config import Config, parse_cli_overrides


def _split(argv: List[str]):
    rest = [a for a in argv if not (a.startswith("-D") and "=" in a)]
    return rest, parse_cli_overrides(argv)


def cmd_validate(args, cfg: Config) -> int:
    from .api import LogParser
    d = args.directory or cfg["pattern.directory"]
    rep = LogParser.from_directory(d, config=cfg.replace({"engine.device": "cpu"})).validate(
        allow=tuple(x for x in args.allow.split(",") if x))
    print(json.dumps({"directory": d, **rep}, indent=2))
    return 1 if any(p["kind"] == "invalid" for p in rep["problems"]) else 0


def _parser(args, cfg: Config):
    """The parser of a command that takes ``--patterns`` / ``--device`` (``_library_options``)."""
    from .api import LogParser
    if args.patterns:
        cfg = cfg.replace({"pattern.directory": args.patterns})
    if args.device:
        cfg = cfg.replace({"engine.device": args.device})
    return LogParser.from_directory(cfg["pattern.directory"], config=cfg)


def _library_options(sub) -> None:
    sub.add_argument("--patterns", help="pattern directory (default: pattern.directory)")
    sub.add_argument("--device", help="cuda | cpu | auto")


def cmd_analyze(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    out = lp.parse_file(args.file, stream=True if args.stream else None, topk=args.topk, raw=True)
    if isinstance(out, (bytes, bytearray)):
        sys.stdout.buffer.write(out)
        sys.stdout.write("\n")
        return 0
    pats = lp.library.patterns
    top = [{"lineNumber": int(l) + 1, "score": float(s), "patternId": pats[int(p)].id}
           for s, l, p in zip(out.topk_score, out.topk_line, out.topk_pat)]
    print(json.dumps({"totalLines": out.total_lines, "bytes": out.bytes, "chunks": out.chunks,
                      "seconds": round(out.seconds, 3), "summary": out.summary, "topEvents": top}))
    return 0


def cmd_gaps(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    if len(args.file) > 1:
        if args.stream:
            print("gaps: --stream takes one file", file=sys.stderr)
            return 2

        def docs():
            for path in args.file:
                with open(path, "rb") as f:
                    yield f.read()
        rep = lp.gaps_corpus(docs(), top=args.top, cover=args.cover)
    elif args.stream:
        rep = lp.gaps_stream(args.file[0], top=args.top, cover=args.cover)
    else:
        rep = lp.gaps_file(args.file[0], top=args.top, cover=args.cover)
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_timeline(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    call = lp.timeline_stream if args.stream else lp.timeline_file
    try:
        rep = call(args.file, bucket_seconds=args.bucket)
    except ValueError as e:                 # the span of the log against max_buckets
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_novel(args, cfg: Config) -> int:
    from .api import _source
    lp = _parser(args, cfg)
    try:
        if args.baseline_file:
            base = lp.load_baseline(args.baseline_file)
        else:
            base = lp.baseline()
            for path in args.baseline:      # every file one document; big ones in chunks, as parse_file reads them
                if os.path.getsize(path) > lp.stream_threshold():
                    with _source(path) as src:
                        base.add_stream(src)
                else:
                    base.add_file(path)
        if args.save_baseline:
            base.save(args.save_baseline)
        kw = {"top": args.top, "order": args.order, "errors_only": args.errors_only}
        if args.stream:
            rep = lp.novelty_stream(args.file, base, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.novelty_file(args.file, base, **kw)
    except ValueError as e:                 # a baseline file of another format
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_traces(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    kw = {"top": args.top, "order": args.order, "unexplained_only": args.unexplained_only}
    if args.stream:
        rep = lp.traces_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
    else:
        rep = lp.traces_file(args.file, **kw)
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_leadup(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    kw = {"window": args.window, "top": args.top, "order": args.order, "min_count": args.min_count}
    try:
        if args.stream:
            rep = lp.leadup_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.leadup_file(args.file, **kw)
    except ValueError as e:                 # a window or a minimum count out of range
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_correlate(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    kw = {"min_len": args.min_length, "top": args.top, "order": args.order, "min_lines": args.min_lines,
          "max_share": args.max_share}
    try:
        if args.stream:
            rep = lp.correlate_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.correlate_file(args.file, **kw)
    except ValueError as e:                 # a length, a count or a share out of range
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_values(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    kw = {"top": args.top, "order": args.order, "min_count": args.min_count, "min_fill": args.min_fill,
          "varying": not args.all_fields}
    try:
        if args.stream:
            rep = lp.values_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.values_file(args.file, **kw)
    except ValueError as e:                 # a count or a share out of range, a log of 2^32 lines
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_variants(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    try:
        acc = lp.variant_accumulator(args.max_distinct)
        for path in args.files:             # several files continue ONE log
            if args.stream:
                from .api import _source
                with _source(path) as src:
                    acc.add_stream(src, args.chunk_bytes)
            else:
                with open(path, "rb") as f:
                    acc.add_document(f.read())
        rep = acc.report(top=args.top, order=args.order, min_count=args.min_count, min_fill=args.min_fill,
                         varying=not args.all, show=args.show)
    except ValueError as e:                 # a count, a share or the limit of distinct values out of range
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_spans(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    try:
        acc = lp.span_accumulator(args.min_length, args.max_ids)
        for path in args.files:             # several files continue ONE log
            if args.stream:
                from .api import _source
                with _source(path) as src:
                    acc.add_stream(src, args.chunk_bytes)
            else:
                with open(path, "rb") as f:
                    acc.add_document(f.read())
        rep = acc.report(top=args.top, order=args.order, unfinished_only=args.unfinished_only, min_lines=args.min_lines,
                         max_share=args.max_share, min_ms=args.min_ms, kinds=args.kinds)
    except ValueError as e:                 # a length, a count, a share or the limit of ids out of range
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_trends(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    at = int(args.at) if args.at is not None and args.at.lstrip("-").isdigit() else args.at
    kw = {"bucket_seconds": args.bucket, "at": at, "ratio": args.ratio, "min_count": args.min_count, "kind": args.kind,
          "order": args.order, "top": args.top}
    try:
        if args.stream:
            rep = lp.trends_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.trends_file(args.file, **kw)
    except ValueError as e:                 # a pivot outside the log's span, a span against max_buckets
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_pauses(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    kw = {"min_ms": args.min_ms, "by": args.by, "order": args.order, "min_count": args.min_count, "top": args.top}
    try:
        if args.stream:
            rep = lp.pauses_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.pauses_file(args.file, **kw)
    except ValueError as e:                 # a threshold or a count out of range
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def cmd_cadence(args, cfg: Config) -> int:
    lp = _parser(args, cfg)
    kw = {"min_ms": args.min_ms, "ratio": args.ratio, "min_count": args.min_count,
          "min_regularity": args.min_regularity, "kind": args.kind, "order": args.order, "top": args.top}
    try:
        if args.stream:
            rep = lp.cadence_stream(args.file, chunk_bytes=args.chunk_bytes, **kw)
        else:
            rep = lp.cadence_file(args.file, **kw)
    except ValueError as e:                 # a threshold, a ratio or a share out of range
        print(str(e), file=sys.stderr)
        return 2
    print(json.dumps(rep, ensure_ascii=False))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    from .utils.launch import ensure_hw_queues
    ensure_hw_queues()                  # before the first HIP call (profiles/r3_f)
    if argv and argv[0] == "serve":
        from .serve.__main__ import main as serve_main
        serve_main(argv[1:])
        return 0
    rest, overrides = _split(argv)
    ap = argparse.ArgumentParser(prog="log-parser-amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("serve", help="run the REST service")
    a = sub.add_parser("analyze", help="analyse a log file")
    a.add_argument("file")
    _library_options(a)
    a.add_argument("--stream", action="store_true", help="chunked streaming pass (automatic for big files)")
    a.add_argument("--topk", type=int, default=20)
    v = sub.add_parser("validate", help="compile a pattern library and report problem regexes")
    v.add_argument("directory", nargs="?")
    v.add_argument("--allow", default="nfa", help="comma list of non-DFA kinds not reported (default nfa)")
    g = sub.add_parser("gaps", help="error lines of a log file that no pattern explains, grouped by template")
    g.add_argument("file", nargs="+", help="one log file, or several: the corpus report in argument order")
    _library_options(g)
    g.add_argument("--stream", action="store_true", help="one file processed in chunks (same report)")
    g.add_argument("--top", type=int, default=20, help="groups reported (default 20)")
    g.add_argument("--cover", choices=("events", "context"), default="context",
                   help="what an event covers: its own line, or its context window too (default)")
    t = sub.add_parser("timeline", help="lines, error lines and events of a log file per time bucket")
    t.add_argument("file")
    _library_options(t)
    t.add_argument("--bucket", type=int, default=60, metavar="SECONDS", help="bucket width (default 60)")
    t.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    n = sub.add_parser("novel", help="lines of a log file whose template a baseline of healthy logs never showed")
    n.add_argument("file")
    _library_options(n)
    src = n.add_mutually_exclusive_group(required=True)
    src.add_argument("--baseline", nargs="+", metavar="FILE", help="healthy log files, each one document")
    src.add_argument("--baseline-file", metavar="B.npz", help="a baseline saved by --save-baseline")
    n.add_argument("--save-baseline", metavar="B.npz", help="write the baseline's signatures to this file")
    n.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    n.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    n.add_argument("--top", type=int, default=20, help="groups reported (default 20)")
    n.add_argument("--order", choices=("count", "first"), default="count",
                   help="most frequent first (default), or in order of first appearance")
    n.add_argument("--errors-only", action="store_true", help="list only the groups with error lines")
    r = sub.add_parser("traces", help="stack traces of a log file grouped by their frames and causes")
    r.add_argument("file")
    _library_options(r)
    r.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    r.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    r.add_argument("--top", type=int, default=20, help="groups reported (default 20)")
    r.add_argument("--order", choices=("count", "first"), default="count",
                   help="most frequent first (default), or in order of first appearance")
    r.add_argument("--unexplained-only", action="store_true", help="list only the groups no event lies on")
    u = sub.add_parser("leadup", help="line templates of a log file that precede its events more often than elsewhere")
    u.add_argument("file")
    _library_options(u)
    u.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    u.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    u.add_argument("--window", type=int, default=50, metavar="N", help="lines before an event that count (default 50)")
    u.add_argument("--top", type=int, default=20, help="groups reported (default 20)")
    u.add_argument("--order", choices=("share", "count", "first"), default="share",
                   help="largest share of the template's lines first (default), most frequent first, "
                        "or in order of first appearance")
    u.add_argument("--min-count", type=int, default=2, metavar="N",
                   help="list only the groups with at least N lead-up lines (default 2)")
    c = sub.add_parser("correlate", help="the ids on the event lines of a log file, followed through the log")
    c.add_argument("file")
    _library_options(c)
    c.add_argument("--stream", action="store_true", help="the file processed in chunks, read twice (same report)")
    c.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    c.add_argument("--min-length", type=int, default=8, metavar="N", help="bytes of an id at least (4..64, default 8)")
    c.add_argument("--top", type=int, default=20, help="ids reported (default 20)")
    c.add_argument("--order", choices=("events", "lines", "first"), default="events",
                   help="most event lines first (default), most lines first, or in order of the first event line")
    c.add_argument("--min-lines", type=int, default=2, metavar="N",
                   help="list only the ids on at least N lines (default 2)")
    c.add_argument("--max-share", type=float, default=0.25, metavar="F",
                   help="drop the ids on more than this share of all lines (default 0.25)")
    v = sub.add_parser("values", help="the numeric fields of the line templates of a log file and their peaks")
    v.add_argument("file")
    _library_options(v)
    v.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    v.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    v.add_argument("--top", type=int, default=20, help="fields reported (default 20)")
    v.add_argument("--order", choices=("peak", "max", "count", "first"), default="peak",
                   help="largest value in units of the mean first (default), largest value first, most values "
                        "first, or in order of first appearance")
    v.add_argument("--min-count", type=int, default=5, metavar="N",
                   help="list only the fields with at least N values (default 5)")
    v.add_argument("--min-fill", type=float, default=0.9, metavar="F",
                   help="list only the fields with a value on at least this share of their template's lines "
                        "(default 0.9)")
    v.add_argument("--all-fields", action="store_true", help="list the fields whose value never changes too")
    w = sub.add_parser("variants", help="the values that the variable tokens of the line templates of a log take")
    w.add_argument("files", nargs="+", metavar="FILE")
    _library_options(w)
    w.add_argument("--stream", action="store_true", help="the files processed in chunks (same report)")
    w.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    w.add_argument("--max-distinct", type=int, default=64, metavar="N",
                   help="a field with more than N distinct values is only counted (2..4096, default 64)")
    w.add_argument("--order", choices=("odd", "count", "distinct", "first"), default="odd",
                   help="smallest share of lines off the most common value first (default), most tokens first, most "
                        "distinct values first, or in order of first appearance")
    w.add_argument("--min-count", type=int, default=5, metavar="N",
                   help="list only the fields with at least N tokens (default 5)")
    w.add_argument("--min-fill", type=float, default=0.9, metavar="F",
                   help="list only the fields present on at least this share of their template's lines (default 0.9)")
    w.add_argument("--all", action="store_true", help="list the fields whose value never changes too")
    w.add_argument("--show", type=int, default=5, metavar="N",
                   help="values listed per field: all up to 2N, else the N most and the N least common (default 5)")
    w.add_argument("--top", type=int, default=20, help="fields reported (default 20)")
    n = sub.add_parser("spans", help="the lifetimes of the ids of a log: the longest, and the ones that never ended")
    n.add_argument("files", nargs="+", metavar="FILE")
    _library_options(n)
    n.add_argument("--stream", action="store_true", help="the files processed in chunks (same report)")
    n.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    n.add_argument("--min-length", type=int, default=8, metavar="N",
                   help="an id is a run of N..64 letters and digits that holds a digit (4..64, default 8)")
    n.add_argument("--min-lines", type=int, default=2, metavar="N",
                   help="list only the ids on at least N lines (default 2)")
    n.add_argument("--max-share", type=float, default=0.25, metavar="F",
                   help="drop the ids on more than this share of all lines: a host name is no id (default 0.25)")
    n.add_argument("--min-ms", type=int, default=0, metavar="N",
                   help="list only the spans that lasted at least N milliseconds (default 0)")
    n.add_argument("--order", choices=("duration", "lines", "first"), default="duration",
                   help="longest span first (default), most lines first, or in order of first appearance")
    n.add_argument("--unfinished-only", action="store_true",
                   help="list only the spans that did not close on the template their kind usually ends on")
    n.add_argument("--max-ids", type=int, default=1 << 22, metavar="N",
                   help="ids kept at most; above that the report is one of a hash sample (16..2^26, default 2^22)")
    n.add_argument("--top", type=int, default=20, help="spans reported (default 20)")
    n.add_argument("--kinds", type=int, default=10, help="kinds of span reported (default 10)")
    d = sub.add_parser("trends", help="line templates of a log file that started, stopped, surged or faded over its time")
    d.add_argument("file")
    _library_options(d)
    d.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    d.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    d.add_argument("--bucket", type=int, default=60, metavar="SECONDS", help="bucket width (default 60)")
    d.add_argument("--at", default=None, metavar="T",
                   help="the pivot: epoch milliseconds, a timestamp, first-event or first-error (default: the middle "
                        "of the log's span)")
    d.add_argument("--ratio", type=int, default=4, metavar="R",
                   help="the factor by which a rate must change to count as surged or faded (default 4)")
    d.add_argument("--min-count", type=int, default=5, metavar="N",
                   help="list only the templates with at least N dated lines (default 5)")
    d.add_argument("--kind", choices=("started", "stopped", "surged", "faded", "steady", "all"), default=None,
                   help="list only this kind (default: all but steady)")
    d.add_argument("--order", choices=("change", "count", "first"), default="change",
                   help="largest change of rate first (default), most dated lines first, or in order of first "
                        "appearance")
    d.add_argument("--top", type=int, default=20, help="templates reported (default 20)")
    q = sub.add_parser("pauses", help="where a log file went silent, and after which line templates")
    q.add_argument("file")
    _library_options(q)
    q.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    q.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    q.add_argument("--min-ms", type=int, default=1000, metavar="N",
                   help="a step of at least N milliseconds between two stamped lines is a pause (default 1000)")
    q.add_argument("--by", choices=("before", "after"), default="before",
                   help="group the pauses by the template of the line before them (default) or after them")
    q.add_argument("--order", choices=("total", "max", "count", "share", "first"), default="total",
                   help="most paused time first (default), longest pause first, most pauses first, largest share of "
                        "the template's lines first, or in order of the first pause")
    q.add_argument("--min-count", type=int, default=1, metavar="N",
                   help="list only the templates with at least N pauses (default 1)")
    q.add_argument("--top", type=int, default=20, help="pauses and templates reported (default 20)")
    b = sub.add_parser("cadence", help="line templates of a log file that come at a steady beat, and the beats they missed")
    b.add_argument("file")
    _library_options(b)
    b.add_argument("--stream", action="store_true", help="the file processed in chunks (same report)")
    b.add_argument("--chunk-bytes", type=int, default=None, metavar="N", help="chunk size of --stream")
    b.add_argument("--min-ms", type=int, default=1000, metavar="N",
                   help="a hole is at least N milliseconds long, whatever the template's beat (default 1000)")
    b.add_argument("--ratio", type=int, default=4, metavar="R",
                   help="a hole is at least R times the template's typical beat (default 4)")
    b.add_argument("--min-count", type=int, default=5, metavar="N",
                   help="judge only the templates with at least N beats (default 5)")
    b.add_argument("--min-regularity", type=float, default=0.8, metavar="F",
                   help="a template is periodic when this share of its beats lies within a factor 4 (default 0.8)")
    b.add_argument("--kind", choices=("missed", "stopped", "all"), default=None,
                   help="list only the templates that missed beats, or that stopped, or every periodic one "
                        "(default: missed or stopped)")
    b.add_argument("--order", choices=("gap", "overdue", "count", "first"), default="gap",
                   help="largest hole in beats of its template first (default), longest overdue first, most beats "
                        "first, or in order of first appearance")
    b.add_argument("--top", type=int, default=20, help="templates reported (default 20)")
    args = ap.parse_args(rest)
    logging.basicConfig(level=logging.WARNING, format="%(levelname)s [%(name)s] %(message)s")
    cfg = Config.load(overrides=overrides)
    return {"analyze": cmd_analyze, "validate": cmd_validate, "gaps": cmd_gaps,
            "timeline": cmd_timeline, "novel": cmd_novel, "traces": cmd_traces,
            "leadup": cmd_leadup, "correlate": cmd_correlate, "values": cmd_values,
            "variants": cmd_variants, "spans": cmd_spans,
            "trends": cmd_trends, "pauses": cmd_pauses, "cadence": cmd_cadence}[args.cmd](args, cfg)


if __name__ == "__main__":
    sys.exit(main())
