"""Synthetic pod logs and randomly generated pattern libraries (BASELINE.json configs).

There is no network and the reference ships no fixtures, so tests and the bench
use generated data of the configured shape: ``n_patterns`` patterns (with secondary and
sequence patterns and context rules) and logs of ``n_lines`` realistic-looking lines into which
pattern triggers are planted at a controlled rate.
"""
from __future__ import annotations

import random
from datetime import datetime, timedelta
from typing import Dict, List, Optional, Tuple

from ..models.schema import PatternSet

LEVELS = ["INFO", "DEBUG", "WARN", "ERROR", "TRACE", "INFO", "INFO", "DEBUG"]
COMPONENTS = ["kubelet", "controller", "scheduler", "api-server", "etcd", "ingress", "app", "worker", "db-pool",
              "cache", "auth", "gateway"]
WORDS = ["request", "handled", "user", "session", "started", "completed", "processing", "batch", "queue", "item",
         "connection", "pool", "cache", "hit", "miss", "retry", "timeout", "latency", "bytes", "sent", "received",
         "config", "reload", "metrics", "flush", "checkpoint", "shard", "replica", "leader", "follower", "sync",
         "node", "pod", "container", "image", "pulled", "volume", "mounted", "probe", "ready", "healthy"]
SEVERITIES = ["CRITICAL", "HIGH", "MEDIUM", "LOW", "INFO"]
EXC = ["java.lang.NullPointerException", "java.io.IOException", "java.lang.IllegalStateException",
       "java.util.concurrent.TimeoutException", "java.lang.OutOfMemoryError"]


def _token(rng: random.Random, i: int) -> str:
    syl = ["ka", "ze", "tor", "vin", "qua", "mel", "dro", "pix", "lun", "sar", "bex", "fyr", "gol", "hup"]
    return "".join(rng.choice(syl) for _ in range(3)).capitalize() + str(i)


# letters that never start a 3-gram of the noise text (no vowels, no T/Z of the timestamps)
_CODE_LETTERS = "BCFGHJKMPQVWXY"


def _short_code(rng: random.Random, n: int) -> str:
    """3..6-byte error code (e.g. 'K42', 'QX7M1'): a short, realistic prefilter literal."""
    s = rng.choice(_CODE_LETTERS)
    while len(s) < n:
        s += rng.choice(_CODE_LETTERS + "0123456789")
    return s


def _literal_free(rng: random.Random, i: int) -> Tuple[str, str]:
    """A regex with no usable literal factor (every line must be scanned) + a matching sample.
    Parametrised by ``i`` so every regex of the library is a distinct string; shapes that the
    noise text of ``make_log`` never matches."""
    fam = i % 6
    a, b = 3 + (i // 6) % 3, 2 + (i // 18) % 6
    rx, sample = _literal_free_shape(rng, fam, a, b)
    if i >= 108:                     # past one cycle of shapes: an optional tail keeps them distinct
        rx += rf"(?:~{i // 108})?"
    return rx, sample


def _literal_free_shape(rng: random.Random, fam: int, a: int, b: int) -> Tuple[str, str]:
    up = "".join(rng.choice("ABCDEFGHJKLMNPQRSUVWXY") for _ in range(a + 1))
    dg = "".join(rng.choice("0123456789") for _ in range(b))
    if fam == 0:
        return rf"\b[A-Z]{{{a},}}_\d{{{b}}}\b", f"state {up}_{dg} entered"
    if fam == 1:
        return rf"\b[A-Z]{{2}}\d{{{a}}}[A-Z]{{{b}}}\b", \
            f"unit {up[:2]}{dg[:1] * a}{''.join(rng.choice('KMPQVX') for _ in range(b))} down"
    if fam == 2:
        m = 1 + b % 3
        return rf"\b\d{{1,3}}\.\d{{1,3}}\.\d{{{m},3}}\.\d+:\d{{{a + 1}}}\b", \
            f"peer 10.2.{'7' * m}.4:{'9' * (a + 1)} reset"
    if fam == 3:
        return rf"[^\s]+@[^\s]+\.[a-z]{{{b}}}\b", f"mail to ops@corp.{'x' * b} bounced"
    if fam == 4:
        return rf"\b[A-Z][a-z]+[A-Z][a-z]+\d{{{a}}}[A-Z]{{{b}}}\b", \
            f"got ShardLost{'5' * a}{'Q' * b} again"
    return rf"^\s+at\s+[a-z]+\.[A-Z]\w{{{a},}}\(\w*\.\w+:\d{{{b}}}\)", \
        f"\tat app.R{'x' * a}(Main.java:{'4' * b})"


def _bounded_gap(rng: random.Random, tok: str, i: int) -> Tuple[str, str, str, str]:
    """A bounded-gap regex (``X.{0,n}Y``: its DFA exceeds engine.dfa-max-states, so it runs as a
    bit-parallel Glushkov program) + a matching sample, and a bounded-gap secondary + its sample."""
    fam = i % 6
    g = (60, 80, 100, 120)[(i // 6) % 4]
    if fam == 0:
        rx, sm = rf"{tok} refused.{{0,{g}}}port \d+", f"{tok} refused by upstream 10.0.0.7 on port 8443"
    elif fam == 1:
        rx, sm = rf"pod .{{1,{g}}} in namespace {tok} .{{1,40}} failed", f"pod web-7f9c in namespace {tok} sync failed"
    elif fam == 2:
        rx, sm = rf"(?i)error.{{0,{g}}}{tok}.{{0,{g}}}retry", f"ERROR while calling {tok}, will retry in 5s"
    elif fam == 3:
        rx, sm = rf"(\w+\.){{2,}}{tok}Exception.{{0,{g}}}Caused by", f"com.acme.{tok}Exception: boom Caused by io"
    elif fam == 4:
        rx, sm = rf"{tok}.{{0,{g}}}(?:timed out|deadline exceeded)", f"{tok} call to db-0 deadline exceeded"
    else:
        rx, sm = rf"\b\d{{1,3}}(?:\.\d{{1,3}}){{3}}\b.{{0,{g}}}{tok} (?:refused|reset)", f"peer 10.1.2.3 said {tok} reset"
    srx, ssm = rf"{tok}Gap.{{0,{g // 2}}}code=\d+", f"{tok}Gap probe returned code=503"
    return rx, sm, srx, ssm


def _java_shape(rng: random.Random, tok: str, i: int) -> Tuple[str, str]:
    """The Java regex shapes a byte-DFA engine cannot hold, + a matching sample (planted after an
    ASCII noise prefix): wide bounded gaps (> 512 byte positions), Unicode properties, MULTILINE
    anchors inside a line (after U+2028), Unicode \\b, partial non-ASCII classes, UNICODE_CASE."""
    fam = i % 7
    if fam == 0:
        return rf"{tok} refused.{{0,600}}port \d+", f"{tok} refused by upstream 10.0.0.7 on port 8443"
    if fam == 1:
        return rf"(?i)error.{{0,300}}{tok}.{{0,300}}retry", f"ERROR while calling {tok} (état dégradé), will retry"
    if fam == 2:
        return rf"\p{{Lu}}\p{{L}}+{tok}Exception", f"caught Élan{tok}Exception in worker"
    if fam == 3:
        return rf"(?m)^\[{tok}\] (?:FATAL|ERROR)$", f"\u2028[{tok}] FATAL"
    if fam == 4:
        return rf"(?U)\b{tok}\w*Fehler\b", f"{tok}größeFehler erkannt"
    if fam == 5:
        return rf"[^\sé]+ {tok} échec", f"job-7 {tok} échec"
    return rf"(?iu){tok}: ÉCHEC .{{0,40}}Ä", f"{tok.upper()}: échec du contrôleur ä"


def make_library(n_patterns: int, seed: int = 0, n_sets: int = 4, secondary_rate: float = 0.7,
                 sequence_rate: float = 0.4, feature_mix: bool = True, short_literal_rate: float = 0.0,
                 literal_free_rate: float = 0.0, gap_rate: float = 0.0,
                 java_shape_rate: float = 0.0) -> Tuple[List[PatternSet], List[dict]]:
    """Returns (pattern sets, trigger descriptions used by ``make_log`` to plant matches).

    ``short_literal_rate`` / ``literal_free_rate`` / ``gap_rate`` / ``java_shape_rate``: shares of
    primaries whose only literal is a 3-6-byte code, that have no usable literal at all, that are
    bounded-gap regexes whose DFA blows up, or that use the Unicode / MULTILINE / wide-gap shapes of
    ``_java_shape`` (``realistic_library``)."""
    rng = random.Random(seed)
    sets = [{"metadata": {"library_id": f"synthetic-lib-{s}", "version": "1.0"}, "patterns": []}
            for s in range(n_sets)]
    triggers = []
    n_free = n_gap = n_java = 0
    for i in range(n_patterns):
        tok = _token(rng, i)
        style = rng.randrange(8) if feature_mix else 0
        u = rng.random()
        if u < literal_free_rate:
            style = 8
        elif u < literal_free_rate + short_literal_rate:
            style = 9
        elif u < literal_free_rate + short_literal_rate + gap_rate:
            style = 10
        elif u < literal_free_rate + short_literal_rate + gap_rate + java_shape_rate:
            style = 11
        gap_sec = None
        if style == 11:
            regex, sample = _java_shape(rng, tok, n_java)
            n_java += 1
        elif style == 10:
            regex, sample, srx, ssm = _bounded_gap(rng, tok, n_gap)
            gap_sec = (srx, ssm)
            n_gap += 1
        elif style == 8:
            regex, sample = _literal_free(rng, n_free)
            n_free += 1
        elif style == 9:
            code = _short_code(rng, 3 + i % 4)
            k = i % 3
            if k == 0:
                regex, sample = rf"\b{code}\b", f"fault {code} raised"
            elif k == 1:
                regex, sample = rf"(?i)\b{code}: \w+", f"{code.lower()}: aborted"
            else:
                regex, sample = rf"{code}\d*[a-z]?$", f"exit with {code}7"
        elif style == 0:
            regex, sample = tok + "Failure", f"{tok}Failure detected"
        elif style == 1:
            regex, sample = rf"(?i)\b{tok}\s+(crashed|aborted)\b", f"{tok.upper()} crashed unexpectedly"
        elif style == 2:
            regex, sample = rf"{tok}: code=\d{{3,5}}", f"{tok}: code={rng.randint(100, 99999)}"
        elif style == 3:
            regex, sample = rf"(Fatal|Severe) {tok} (state|status)", f"Fatal {tok} status reached"
        elif style == 4:
            regex, sample = rf"{tok}[A-Z]+Exception", f"caught {tok}PANICException in handler"
        elif style == 5:
            regex, sample = rf"^\[{tok}\] .*rejected", f"[{tok}] request was rejected"
        elif style == 6:
            regex, sample = rf"{tok}\.(conn|sock)[0-9]+ (lost|closed)$", f"{tok}.conn{rng.randint(0, 99)} lost"
        else:
            regex, sample = rf"{tok}-[a-f0-9]{{4}} timed? ?out", f"{tok}-{rng.randrange(16**4):04x} timed out"
        pat = {
            "id": f"pat-{i:05d}" if rng.random() > 0.02 else f"pat-{i // 2:05d}",
            "name": f"Synthetic failure {i}",
            "severity": rng.choice(SEVERITIES) if rng.random() > 0.03 else "weird",
            "primary_pattern": {"regex": regex, "confidence": round(rng.uniform(0.3, 0.95), 3)},
            "remediation": {"description": f"fix {tok}", "common_causes": ["synthetic"]},
        }
        secs, seqs, sec_samples = [], [], []
        if rng.random() < secondary_rate or gap_sec:
            for k in range(rng.randint(1, 3)):
                stok = f"{tok}Aux{k}"
                secs.append({"regex": stok if k else rf"(?i){stok}\b", "weight": round(rng.uniform(0.1, 0.9), 2),
                             "proximity_window": rng.choice([3, 5, 10, 20, 50, 200])})
                sec_samples.append(stok)
            if gap_sec:
                secs.append({"regex": gap_sec[0], "weight": 0.4, "proximity_window": 20})
                sec_samples.append(gap_sec[1])
            pat["secondary_patterns"] = secs
        if rng.random() < sequence_rate:
            evs = [{"regex": f"{tok}Step{k}"} for k in range(rng.randint(1, 3))]
            seqs.append({"description": f"{tok} lifecycle", "bonus_multiplier": round(rng.uniform(0.2, 1.5), 2),
                         "events": evs})
            pat["sequence_patterns"] = seqs
        if rng.random() < 0.8:
            pat["context_extraction"] = {"lines_before": rng.randint(0, 8), "lines_after": rng.randint(0, 6),
                                         "include_stack_trace": rng.random() < 0.5}
        sets[i % n_sets]["patterns"].append(pat)
        triggers.append({"sample": sample, "secondary": sec_samples,
                         "sequence": [e["regex"] for q in seqs for e in q["events"]]})
    return [PatternSet.model_validate(s) for s in sets], triggers


def backtracker_patterns(n: int, seed: int = 0) -> Tuple[PatternSet, List[dict]]:
    """``n`` primaries only a backtracker decides (backreferences, atomic groups /
    possessive quantifiers, lookarounds the automata do not express -- nested, or around a '$') +
    matching samples: n - 1 carry a pattern-specific literal (the device prefilter narrows them), the
    last one has none (its relaxed automaton runs in a literal-free scan group). The shapes real
    libraries use: a repeated id, "Fail" not followed by "ure", an error not preceded by "retrying",
    a restart loop of the same pod. (Plain lookaround clusters compile to DFAs: see
    ``lookaround_patterns``.)"""
    rng = random.Random(seed)
    pats, trig = [], []
    for i in range(n):
        tok = _token(rng, 10_000 + i)
        fam = i % 4
        if i == n - 1:
            rx, sm = r"^(\d{3})-(\d{4})-\2-\1$", "415-8812-8812-415"
        elif fam == 0:
            rx, sm = rf"(\w+) {tok}Loop \1\b", f"worker7 {tok}Loop worker7 again"
        elif fam == 1:
            rx, sm = rf"{tok}Fail(?!ure(?=\s))\w*", f"{tok}Failed to mount"
        elif fam == 2:
            rx, sm = rf"(?<!retrying )\b{tok}Err\b(?!.*done$)", f"fatal {tok}Err in worker"
        else:
            rx, sm = rf"(?i)(?>{tok}Lock)+\s+held", f"{tok.upper()}LOCK held by 7"
        pats.append({"id": f"bt-{i:04d}", "name": f"backtracker shape {i}", "severity": rng.choice(SEVERITIES),
                     "primary_pattern": {"regex": rx, "confidence": round(rng.uniform(0.3, 0.95), 3)}})
        trig.append({"sample": sm, "secondary": [], "sequence": []})
    ps = PatternSet.model_validate({"metadata": {"library_id": "backtracker", "version": "1.0"}, "patterns": pats})
    return ps, trig


def lookaround_patterns(n: int, seed: int = 0) -> Tuple[PatternSet, List[dict]]:
    """``n`` primaries with lookaround clusters used as line filters -- "Fail" not followed by "ure",
    an error not preceded by "retrying", ERROR with no "retry" later on the line, a token followed
    later by FATAL, an isolated word -- which compile to exact find() DFAs (jregex.cpp
    ``LookaroundDfa``), + matching samples."""
    rng = random.Random(seed)
    pats, trig = [], []
    for i in range(n):
        tok = _token(rng, 30_000 + i)
        fam = i % 5
        if fam == 0:
            rx, sm = rf"{tok}Fail(?!ure)\w*", f"{tok}Failed to mount"
        elif fam == 1:
            rx, sm = rf"(?<!retrying )\b{tok}Err\b", f"fatal {tok}Err in worker"
        elif fam == 2:
            rx, sm = rf"\b{tok}ERROR\b(?!.*retry)", f"{tok}ERROR disk full"
        elif fam == 3:
            rx, sm = rf"(?=.*FATAL){tok}Err", f"{tok}Err then FATAL"
        else:
            rx, sm = rf"(?<!\S){tok}x(?!\S)", f"got {tok}x here"
        pats.append({"id": f"la-{i:04d}", "name": f"lookaround shape {i}", "severity": rng.choice(SEVERITIES),
                     "primary_pattern": {"regex": rx, "confidence": round(rng.uniform(0.3, 0.95), 3)}})
        trig.append({"sample": sm, "secondary": [], "sequence": []})
    ps = PatternSet.model_validate({"metadata": {"library_id": "lookaround", "version": "1.0"}, "patterns": pats})
    return ps, trig


def counted_repeat_patterns(n: int, seed: int = 0) -> Tuple[PatternSet, List[dict]]:
    """``n`` primaries with a wide bounded repeat of one class (``X.{0,2100}Y``,
    ``X[^;]{0,5000}Y``, ``X\\S{0,20000}Y``): the regular shapes past the 2,048-position BPG limit
    that compile to a counted position (csrc/regex/jregex.cpp ``Glushkov`` counters) + matching
    samples."""
    rng = random.Random(seed)
    pats, trig = [], []
    shapes = ((r"{a}.{{0,2100}}{b}", "{a} then some text {b}"),
              (r"{a}[^;]{{0,5000}}{b}", "{a} waited {b}"),
              (r"{a}\S{{0,20000}}{b}", "{a}/x/y/{b}"))
    for i in range(n):
        a, b = _token(rng, 20_000 + 2 * i), _token(rng, 20_001 + 2 * i)
        rx, sm = shapes[i % len(shapes)]
        pats.append({"id": f"cr-{i:04d}", "name": f"counted repeat {i}", "severity": rng.choice(SEVERITIES),
                     "primary_pattern": {"regex": rx.format(a=a, b=b), "confidence": round(rng.uniform(0.3, 0.95), 3)}})
        trig.append({"sample": sm.format(a=a, b=b), "secondary": [], "sequence": []})
    ps = PatternSet.model_validate({"metadata": {"library_id": "counted", "version": "1.0"}, "patterns": pats})
    return ps, trig


def realistic_library(n_patterns: int, seed: int = 0, **kw):
    """The headline bench library: the synthetic mix plus ~10% primaries with only a 3-6-byte
    literal, ~5% literal-free primaries, ~1.5% bounded-gap primaries (``X.{0,120}Y``, each
    with a bounded-gap secondary) and ~1% Unicode / MULTILINE / wide-gap shapes
    (``X.{0,600}Y``, ``\\p{L}``, ``(?m)^..$``, ``(?U)\\b``, ``[^é]``, ``(?iu)``) -- the shapes real
    libraries have (short error codes, IP:port, `^\\s+at ...` stack frames, "refused ... port N")
    and the matcher's worst cases."""
    kw.setdefault("short_literal_rate", 0.10)
    kw.setdefault("literal_free_rate", 0.05)
    kw.setdefault("gap_rate", 0.015)
    kw.setdefault("java_shape_rate", 0.01)
    return make_library(n_patterns, seed=seed, **kw)


def _noise_line(rng: random.Random, i: int) -> str:
    lvl = rng.choice(LEVELS)
    comp = rng.choice(COMPONENTS)
    msg = " ".join(rng.choice(WORDS) for _ in range(rng.randint(4, 12)))
    return f"2025-09-19T12:{(i // 60) % 60:02d}:{i % 60:02d}.{i % 1000:03d}Z {lvl:5s} [{comp}] {msg} id={rng.randint(0, 1 << 30)}"


def make_log(n_lines: int, triggers: List[dict], seed: int = 0, hit_rate: float = 0.01,
             aux_rate: float = 0.01, stack_rate: float = 0.01, crlf_rate: float = 0.0) -> str:
    rng = random.Random(seed)
    out = []
    i = 0
    while i < n_lines:
        r = rng.random()
        if triggers and r < hit_rate:
            t = rng.choice(triggers)
            if t["sequence"] and rng.random() < 0.6:
                for ev in t["sequence"][:-1]:
                    out.append(f"INFO [app] {ev} reached")
                    i += 1
            if t["sample"][:1].isspace():          # anchored stack-frame shape: a line of its own
                out.append(t["sample"])
            else:
                out.append(_noise_line(rng, i)[:40] + " " + t["sample"])
            if t["sequence"] and rng.random() < 0.6:
                out.append(f"INFO [app] {t['sequence'][-1]} reached")
                i += 1
            if t["secondary"] and rng.random() < 0.7:
                out.append(f"WARN [app] saw {rng.choice(t['secondary'])} nearby")
                i += 1
        elif triggers and r < hit_rate + aux_rate:
            t = rng.choice(triggers)
            if t["secondary"]:
                out.append(f"DEBUG [app] {rng.choice(t['secondary'])} event")
            else:
                out.append(_noise_line(rng, i))
        elif r < hit_rate + aux_rate + stack_rate:
            out.append(f"ERROR [app] {rng.choice(EXC)}: boom")
            for k in range(rng.randint(1, 6)):
                out.append(f"\tat com.example.svc{k}.Handler$Inner.run(Handler.java:{rng.randint(1, 999)})")
                i += 1
        else:
            out.append(_noise_line(rng, i))
        i += 1
    sep = "\n"
    if crlf_rate > 0:
        parts = []
        for line in out:
            parts.append(line)
            parts.append("\r\n" if rng.random() < crlf_rate else "\n")
        return "".join(parts)
    return sep.join(out) + sep


def log_templates(n: int, seed: int = 0) -> List[str]:
    """``n`` distinct line templates with ``%d`` / ``%x`` fields: a level, a component, a few
    words that never hold a digit, one to four fields. About one in eight is an error line."""
    rng = random.Random(seed)
    out, seen = [], set()
    while len(out) < n:
        lvl = "ERROR" if rng.random() < 0.125 else rng.choice(("INFO", "DEBUG", "WARN", "TRACE"))
        words = [rng.choice(WORDS) for _ in range(rng.randint(3, 9))]
        for _ in range(rng.randint(1, 4)):
            words.insert(rng.randrange(len(words) + 1), rng.choice(("%d", "id=%d", "%dms", "0x%x", "node-%d")))
        t = "2025-09-19T12:%02d:%02d.%03dZ " + f"{lvl:5s} [{rng.choice(COMPONENTS)}] " + " ".join(words)
        key = t.replace("0x%x", "%d").replace("%dms", "%d")     # (fields that sign alike: one digit token)
        if key not in seen:
            seen.add(key)
            out.append(t)
    return out


def templated_log(n_lines: int, templates: List[str], seed: int = 0, crlf_rate: float = 0.0) -> str:
    """A log of ``n_lines`` lines drawn from ``templates`` (``log_templates``) with a skewed
    frequency (a few templates make most of the log, as real logs do) and random numbers in the
    fields: the set of line templates of the log is known by construction. The first three fields
    of a template are the stamp's minute, second and millisecond."""
    rng = random.Random(seed)
    weights = [1.0 / (k + 1) for k in range(len(templates))]
    parts = []
    for i, t in enumerate(rng.choices(templates, weights=weights, k=n_lines)):
        nf = t.count("%") - 3
        parts.append(t % ((i // 60) % 60, i % 60, i % 1000, *(rng.randrange(1, 1 << 20) for _ in range(nf))))
        parts.append("\r\n" if rng.random() < crlf_rate else "\n")
    return "".join(parts)


METRIC_TEMPLATE = "2025-09-19T12:%02d:%02d.%03dZ INFO  [gateway] served request in %dms"


def metric_log(n_lines: int, templates: List[str], seed: int = 0, burst_at: float = 0.8,
               burst_lines: int = 20) -> Tuple[str, List[int]]:
    """A ``templated_log`` with one extra template, ``INFO  [gateway] served request in %dms``, on
    about a tenth of its lines. Its value is uniform in 5..50, except on ``burst_lines``
    consecutive occurrences of the template from line ``burst_at * n_lines`` on, where it is
    uniform in 30000..60000: a latency peak that every report which drops the numbers cannot
    see. Returns (text, the lines of the burst, 0-based and ascending) -- known by construction."""
    rng = random.Random(seed)
    lines = templated_log(n_lines, templates, seed=seed).split("\n")[:n_lines]
    start = int(burst_at * n_lines)
    burst: List[int] = []
    for i in range(n_lines):
        if rng.random() >= 0.1:
            continue
        slow = i >= start and len(burst) < burst_lines
        if slow:
            burst.append(i)
        ms = rng.randint(30000, 60000) if slow else rng.randint(5, 50)
        lines[i] = METRIC_TEMPLATE % ((i // 60) % 60, i % 60, i % 1000, ms)
    return "".join(line + "\n" for line in lines), burst


VARIANT_TEMPLATE = "2025-09-19T12:%02d:%02d.%03dZ INFO  [proxy] upstream returned status %d to worker %d for request %d"


def variant_log(n_lines: int, templates: List[str], seed: int = 0, rare_from: float = 0.7, rare_to: float = 0.8,
                crlf_rate: float = 0.0) -> Tuple[str, dict]:
    """``metric_log``'s templated log with one extra template, ``INFO  [proxy] upstream returned
    status %d to worker %d for request %d``, on about a tenth of its lines, and three planted
    fields on it: field 0, the status, is ``200`` except on about a fifth of the template's lines
    in [``rare_from * n_lines``, ``rare_to * n_lines``), where it is ``503``; field 1, the worker,
    goes round ``0..7``; field 2 is a request id that never repeats. Returns (text, facts) with
    ``facts``: ``template`` (the line behind its stamp, the fields still ``%d``), ``lines`` (the
    template's lines), ``common`` / ``rare`` (the two status tokens), ``rareLines`` (the lines
    that hold the rare one, 0-based and ascending), ``rareRange`` (the [lo, hi) they were confined
    to), ``workers`` -- known by construction. ``crlf_rate``: the share of lines that end in
    ``\\r\\n``."""
    rng = random.Random(seed)
    lines = templated_log(n_lines, templates, seed=seed).split("\n")[:n_lines]
    lo, hi = int(rare_from * n_lines), int(rare_to * n_lines)
    planted, rare = 0, []
    for i in range(n_lines):
        if rng.random() >= 0.1:
            continue
        odd = lo <= i < hi and rng.random() < 0.2
        if odd:
            rare.append(i)
        lines[i] = VARIANT_TEMPLATE % ((i // 60) % 60, i % 60, i % 1000, 503 if odd else 200, planted % 8, 1000000 + i)
        planted += 1
    text = "".join(line + ("\r\n" if rng.random() < crlf_rate else "\n") for line in lines)
    return text, {"template": VARIANT_TEMPLATE.split("Z ", 1)[1], "lines": planted, "common": "200", "rare": "503",
                  "rareLines": rare, "rareRange": (lo, hi), "workers": 8}


SPAN_HOST = "node0042x7"
# (opening line, work lines, closing line) of a kind of span; %s: the id
SPAN_KINDS = (
    ("req", "INFO  [http] request %s started on route /api/orders",
     ("DEBUG [db] query for %s took a while", "DEBUG [cache] lookup for %s missed"),
     "INFO  [http] request %s completed with status ok"),
    ("job", "INFO  [sched] job %s picked up by a worker",
     ("DEBUG [sched] job %s made progress", "DEBUG [store] job %s wrote a checkpoint"),
     "INFO  [sched] job %s finished"),
    ("conn", "INFO  [net] connection %s accepted",
     ("DEBUG [net] connection %s received a frame",),
     "INFO  [net] connection %s closed by the peer"),
)


def span_log(n_lines: int, seed: int = 0, concurrency: int = 8, step_ms: int = 7, crlf_rate: float = 0.0) -> Tuple[str, dict]:
    """A log of exactly ``n_lines`` (>= 64) lines of interleaved requests of three kinds
    (``SPAN_KINDS``): every request has an id of its own -- ``req0000017``, ``job0000018``, ... --
    on its opening line, its work lines and its closing line; up to ``concurrency`` are open at a
    time, and all of them are closed before the log ends. The stamps advance ``step_ms`` per line
    from ``TREND_T0_MS``. Planted: one ``req`` that opens and works like the others and never
    closes (``unfinished``); one ``req`` that opens near the start and closes near the end
    (``long``: far longer than the rest); the token ``SPAN_HOST`` on every line; about one line
    in fifty is an unstamped continuation line that names the request of the line before it; about
    one stamped line in two hundred carries the stamp of twenty lines before. Returns (text,
    facts): ``long`` / ``unfinished`` (the ids), ``host``, ``ids`` (requests opened), ``kinds``."""
    if n_lines < 64:
        raise ValueError("span_log: n_lines must be at least 64")
    rng = random.Random(seed)
    serial = [0]

    def new_id(kind: int) -> Tuple[int, str]:
        serial[0] += 1
        return kind, "%s%07d" % (SPAN_KINDS[kind][0], serial[0])

    def stamp(i: int, back: bool) -> str:
        ms = i * step_ms + 43200000 - (20 * step_ms if back else 0)
        d, ms = divmod(ms, 86400000)
        return "2025-09-%02dT%02d:%02d:%02d.%03dZ" % (19 + d % 10, ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)

    out: List[str] = []

    def emit(body: str) -> None:
        out.append("%s %s host=%s" % (stamp(len(out), len(out) > 8 and rng.random() < 0.005), body, SPAN_HOST))

    long_at, long_end, unf_at = max(2, n_lines // 50), n_lines - max(4, n_lines // 50), n_lines // 2
    long_id = unf_id = None
    unf_work = 0
    active: List[Tuple[int, str]] = []
    while len(out) < n_lines:
        i, left = len(out), n_lines - len(out)
        owe = len(active) + (long_id is not None and i <= long_end)     # closing lines still to come
        if long_id is None and i >= long_at:
            long_id = new_id(0)
            emit(SPAN_KINDS[0][1] % long_id[1])
        elif long_id is not None and i == long_end:
            emit(SPAN_KINDS[0][3] % long_id[1])
        elif left <= owe + 1 and active:
            kind, sid = active.pop(rng.randrange(len(active)))
            emit(SPAN_KINDS[kind][3] % sid)
        elif unf_id is None and i >= unf_at:
            unf_id = new_id(0)
            emit(SPAN_KINDS[0][1] % unf_id[1])
        elif unf_id is not None and unf_work < 3 and rng.random() < 0.2:
            unf_work += 1
            emit(SPAN_KINDS[0][2][unf_work % 2] % unf_id[1])
        elif len(active) < concurrency and left > owe + 3 and (not active or rng.random() < 0.3):
            active.append(new_id(rng.randrange(len(SPAN_KINDS))))
            emit(SPAN_KINDS[active[-1][0]][1] % active[-1][1])
        elif active:
            k = rng.randrange(len(active))
            kind, sid = active[k]
            if rng.random() < 0.25:
                active.pop(k)
                emit(SPAN_KINDS[kind][3] % sid)
            else:
                emit(rng.choice(SPAN_KINDS[kind][2]) % sid)
                if rng.random() < 0.02 and n_lines - len(out) > owe + 2:
                    out.append("    ... still waiting on %s host=%s" % (sid, SPAN_HOST))
        else:
            emit("INFO  [main] idle tick")
    text = "".join(line + ("\r\n" if rng.random() < crlf_rate else "\n") for line in out)
    return text, {"long": long_id[1], "unfinished": unf_id[1], "host": SPAN_HOST, "ids": serial[0],
                  "kinds": len(SPAN_KINDS)}


TREND_T0_MS = 1758283200000        # 2025-09-19T12:00:00Z
TREND_STOPPED = "INFO  [lease] heartbeat: renewed leader lease, sequence %d"
TREND_STARTED = "ERROR [net] connection reset by peer while reading from upstream %d"
TREND_SURGED = "WARN  [gc] pause of %dms exceeded the budget"


def trend_log(n_lines: int, templates: List[str], seed: int = 0, step_ms: int = 100,
              change_at: float = 0.75) -> Tuple[str, Tuple[str, str, str]]:
    """A log whose content changes at one line: line ``i`` is stamped ``TREND_T0_MS + i *
    step_ms`` (a clock of its own that never wraps). The bulk is ``templates``
    (``log_templates``) with the skewed weights of ``templated_log``; about 3 % of the lines are
    unstamped ``\\tat ...`` frames. Three templates are planted around the change line ``c`` =
    ``change_at * n_lines``, moved down to a whole minute of the clock where that leaves a line
    before it (so it is a bucket boundary of every width that divides a minute): a heartbeat on
    every 20th line before ``c`` and never after, an error on about 5 % of the lines from ``c`` on
    and never before, and a line on about 1 % of the lines before and 10 % after. Returns (text,
    (the heartbeat, the error, the surging line)) -- each as it stands in the log behind the stamp,
    with its number field still ``%d``."""
    rng = random.Random(seed)
    weights = [1.0 / (k + 1) for k in range(len(templates))]
    c = int(change_at * n_lines)
    per_minute = max(1, 60000 // step_ms)
    if c // per_minute:
        c = c // per_minute * per_minute
    epoch = datetime(1970, 1, 1)
    parts = []
    for i, t in enumerate(rng.choices(templates, weights=weights, k=n_lines)):
        d = epoch + timedelta(milliseconds=TREND_T0_MS + i * step_ms)
        stamp = "%04d-%02d-%02dT%02d:%02d:%02d.%03dZ " % (d.year, d.month, d.day, d.hour, d.minute, d.second,
                                                          d.microsecond // 1000)
        r = rng.random()
        if i < c and i % 20 == 0:
            line = stamp + TREND_STOPPED % (i // 20)
        elif r < 0.03:
            line = "\tat com.example.worker.Task.run(Task.java:%d)" % rng.randrange(10, 400)
        elif i >= c and r < 0.08:
            line = stamp + TREND_STARTED % rng.randrange(1, 64)
        elif r >= 1.0 - (0.01 if i < c else 0.10):
            line = stamp + TREND_SURGED % rng.randrange(200, 5000)
        else:
            body = t.split(" ", 1)[1]       # (behind the template's own stamp)
            line = stamp + body % tuple(rng.randrange(1, 1 << 20) for _ in range(body.count("%")))
        parts.append(line + "\n")
    return "".join(parts), (TREND_STOPPED, TREND_STARTED, TREND_SURGED)


PAUSE_BEFORE = "INFO  [pool] waiting for a free connection, %d in use"      # what the log says before it goes quiet
PAUSE_AFTER = "WARN  [pool] connection acquired after a wait, attempt %d"     # and when it wakes up


def pause_log(n_lines: int, templates: List[str], seed: int = 0, pauses: int = 6) -> Tuple[str, List[Tuple[int, int, int]]]:
    """A log with planted silences. Stamped lines follow each other by 1..400 ms (a clock of its
    own from ``TREND_T0_MS`` that never wraps); about 3 % of the lines are unstamped ``\\tat ...``
    frames. At ``pauses`` places, spread over the log, a ``PAUSE_BEFORE`` line is followed --
    behind 0..2 unstamped frames -- by a ``PAUSE_AFTER`` line whose stamp is 5 s, 7 s, 9 s ...
    later, a different length at every place. The bulk is ``templates`` (``log_templates``) with
    the skewed weights of ``templated_log``. Returns (text, [(ms, from-line, to-line), ...] of the
    planted pauses, lines 0-based, the longest first) -- known by construction."""
    rng = random.Random(seed)
    weights = [1.0 / (k + 1) for k in range(len(templates))]
    places = {(k + 1) * n_lines // (pauses + 1): k for k in range(pauses)} if n_lines > 4 * pauses else {}
    epoch = datetime(1970, 1, 1)
    t = TREND_T0_MS
    parts: List[str] = []
    planted: List[Tuple[int, int, int]] = []
    pending = None                      # (ms, from-line): the silence the next stamped line ends
    frames = 0                          # unstamped lines still to come inside it
    bulk = iter(rng.choices(templates, weights=weights, k=n_lines))
    for i in range(n_lines):
        body = next(bulk).split(" ", 1)[1]      # (behind the template's own stamp)
        if frames or (pending is None and i not in places and i and rng.random() < 0.03):
            frames = max(0, frames - 1)
            parts.append("\tat com.example.worker.Task.run(Task.java:%d)\n" % rng.randrange(10, 400))
            continue
        if pending is not None:
            t += pending[0]
            planted.append((pending[0], pending[1], i))
            line, pending = PAUSE_AFTER % rng.randrange(1, 9), None
        elif i in places:
            t += rng.randrange(1, 401)
            pending, frames = (5000 + 2000 * places[i], i), places[i] % 3
            line = PAUSE_BEFORE % rng.randrange(1, 64)
        else:
            t += rng.randrange(1, 401)
            line = body % tuple(rng.randrange(1, 1 << 20) for _ in range(body.count("%")))
        d = epoch + timedelta(milliseconds=t)
        parts.append("%04d-%02d-%02dT%02d:%02d:%02d.%03dZ %s\n" % (d.year, d.month, d.day, d.hour, d.minute, d.second,
                                                                  d.microsecond // 1000, line))
    return "".join(parts), sorted(planted, reverse=True)


CADENCE_HOLE = "INFO  [watchdog] fed the watchdog, tick %d"                  # every 5 s, with one hole
CADENCE_STOPPED = "INFO  [lease] renewed the leader lease, term %d"          # every 30 s, until it stops
CADENCE_STEADY = "DEBUG [health] liveness probe answered, check %d"          # every 12 s, all the way
CADENCE_HOLE_MS = 90_000


def cadence_log(n_lines: int, templates: List[str], seed: int = 0) -> Tuple[str, Dict[str, dict]]:
    """A log with three periodic lines among a bulk that is not. Stamped lines follow each other by
    1..400 ms (the clock of ``pause_log``); about 3 % of the lines are unstamped ``\\tat ...``
    frames; the bulk is ``templates`` (``log_templates``) with the skewed weights of
    ``templated_log``. A plant takes the place of a bulk line when its next beat is due: the
    ``CADENCE_HOLE`` line every 5 s +- 10 %, except that at two fifths of the log its next beat
    comes ``CADENCE_HOLE_MS`` late (once); the ``CADENCE_STOPPED`` line every 30 s +- 10 % and never
    from line ``11 * n_lines // 20`` on; the ``CADENCE_STEADY`` line every 12 s +- 10 % to the
    end. Returns (text, {"hole" | "stopped" | "steady": the plant's numbers}) -- ``template``,
    ``lines``, ``beats``, ``sumMs``, ``maxMs``, ``fromLine``, ``toLine`` (of the first largest
    beat), ``typicalMs``, ``missedBeats``, ``firstLine``, ``lastLine`` and ``lastMs`` (its last
    stamp); lines 0-based, all known by construction."""
    rng = random.Random(seed)
    weights = [1.0 / (k + 1) for k in range(len(templates))]
    epoch = datetime(1970, 1, 1)
    t = TREND_T0_MS
    plants = [{"name": "hole", "text": CADENCE_HOLE, "period": 5000, "due": t + 2500, "at": []},
              {"name": "stopped", "text": CADENCE_STOPPED, "period": 30000, "due": t + 4000, "at": []},
              {"name": "steady", "text": CADENCE_STEADY, "period": 12000, "due": t + 7000, "at": []}]
    hole_line, stop_line = 2 * n_lines // 5, 11 * n_lines // 20
    holed = False
    parts: List[str] = []
    bulk = iter(rng.choices(templates, weights=weights, k=n_lines))
    for i in range(n_lines):
        body = next(bulk).split(" ", 1)[1]      # (behind the template's own stamp)
        if i and rng.random() < 0.03:
            parts.append("\tat com.example.worker.Task.run(Task.java:%d)\n" % rng.randrange(10, 400))
            continue
        t += rng.randrange(1, 401)
        if i >= hole_line and not holed:
            plants[0]["due"] += CADENCE_HOLE_MS
            holed = True
        due = [p for p in plants if t >= p["due"] and not (p["name"] == "stopped" and i >= stop_line)]
        if due:
            p = due[0]
            line = p["text"] % len(p["at"])
            p["at"].append((i, t))
            p["due"] = t + p["period"] * rng.randrange(90, 111) // 100
        else:
            line = body % tuple(rng.randrange(1, 1 << 20) for _ in range(body.count("%")))
        d = epoch + timedelta(milliseconds=t)
        parts.append("%04d-%02d-%02dT%02d:%02d:%02d.%03dZ %s\n" % (d.year, d.month, d.day, d.hour, d.minute, d.second,
                                                                  d.microsecond // 1000, line))
    known: Dict[str, dict] = {}
    for p in plants:
        at = p["at"]
        beats = [(b[1] - a[1], a[0], b[0]) for a, b in zip(at, at[1:])]
        row = {"template": p["text"], "lines": len(at), "beats": len(beats), "firstLine": at[0][0] if at else None,
               "lastLine": at[-1][0] if at else None, "lastMs": at[-1][1] if at else None}
        if len(beats) >= 2:
            mx = max(beats, key=lambda b: (b[0], -b[2]))
            total = sum(b[0] for b in beats)
            typical = (total - mx[0]) // (len(beats) - 1)
            row.update({"sumMs": total, "maxMs": mx[0], "fromLine": mx[1], "toLine": mx[2], "typicalMs": typical,
                        "missedBeats": mx[0] // typical - 1})
        known[p["name"]] = row
    return "".join(parts), known


CORRELATED_FAIL ="request aborted: upstream deadline exceeded"     # what the last line of a failing request says


def correlated_log(n_lines: int, templates: List[str], n_requests: int, seed: int = 0, fail_rate: float = 0.25,
                   crlf_rate: float = 0.0) -> Tuple[str, Dict[str, List[int]]]:
    """A ``templated_log`` whose lines carry a `` rid=<16 hex>`` field: the ids come from a pool of
    ``n_requests`` requests, each spanning a random stretch of the log (about eight are under way
    at any line, so their lines interleave), and a line takes the id of one of the requests under
    way, or none where there is none. About ``fail_rate`` of the requests *fail*: the last line of
    their stretch is theirs and is an ERROR line that says ``CORRELATED_FAIL``; so is the first,
    so that a failing request has at least two lines. Returns (text, {id of a failing request:
    its lines, 0-based and ascending, the failing line last}) -- known by construction."""
    rng = random.Random(seed)
    lines = templated_log(n_lines, templates, seed=seed).split("\n")[:n_lines]
    span = max(4, 16 * n_lines // max(1, n_requests))
    ids, reqs = set(), []
    forced: Dict[int, int] = {}                     # line -> request that owns it whatever else is under way
    starts: List[List[int]] = [[] for _ in range(n_lines)]
    for r in range(n_requests):
        rid = "%016x" % rng.getrandbits(64)
        while rid in ids or rid.isalpha():          # (an id holds a digit)
            rid = "%016x" % rng.getrandbits(64)
        ids.add(rid)
        a = rng.randrange(max(1, n_lines - 1))
        b = min(n_lines - 1, a + rng.randint(1, span))
        fails = rng.random() < fail_rate and a < b and a not in forced and b not in forced
        if fails:
            forced[a] = forced[b] = r
        reqs.append((rid, a, b, fails))
        starts[a].append(r)
    failing: Dict[str, List[int]] = {rid: [] for rid, _, _, fails in reqs if fails}
    active: List[int] = []
    out = []
    for i, line in enumerate(lines):
        active += starts[i]
        active = [r for r in active if reqs[r][2] >= i]
        r = forced.get(i, rng.choice(active) if active else None)
        if r is not None:
            rid, _, b, fails = reqs[r]
            if fails and i == b:
                line = "2025-09-19T12:%02d:%02d.%03dZ ERROR [gateway] %s" % ((i // 60) % 60, i % 60, i % 1000,
                                                                            CORRELATED_FAIL)
            line += " rid=" + rid
            if fails:
                failing[rid].append(i)
        out.append(line)
        out.append("\r\n" if rng.random() < crlf_rate else "\n")
    return "".join(out), failing


def trace_sites(n: int, seed: int = 0) -> List[Tuple[str, List[str]]]:
    """``n`` places that throw: (head template, run templates) with ``%d`` fields -- 2..12 ``at``
    frames, for most sites a chain of one to three ``Caused by:`` (with frames and ``... n more``),
    for some a ``Suppressed:`` entry. Distinct sites differ in their frames."""
    rng = random.Random(seed)
    excs = ("java.lang.IllegalStateException", "java.lang.OutOfMemoryError", "java.io.IOException",
            "java.util.concurrent.TimeoutException", "com.acme.db.DeadlockError", "java.lang.NullPointerException")
    out = []
    for k in range(n):
        pkg = "com.acme.%s" % rng.choice(WORDS)
        run = ["\tat %s.S%d.call%d(S%d.java:%%d)" % (pkg, k, j, k) for j in range(rng.randint(2, 12))]
        for c in range(rng.choice((0, 1, 1, 2, 3))):
            run.append("Caused by: %s: %s %%d" % (rng.choice(excs), rng.choice(WORDS)))
            run += ["\tat %s.C%d.step%d(C%d.java:%%d)" % (pkg, k, j, c) for j in range(rng.randint(1, 4))]
            run.append("\t... %d more")
        if k % 5 == 4:
            run += ["\tSuppressed: %s.CloseFailed: %%d" % pkg, "\t\tat %s.Closer.close(Closer.java:%%d)" % pkg]
        out.append(("2025-09-19T12:%02d:%02d.%03dZ ERROR [w-%d] " + "%s: %s failed" % (rng.choice(excs), pkg), run))
    return out


def traced_log(n_lines: int, templates: List[str], sites: List[Tuple[str, List[str]]], seed: int = 0,
               trace_share: float = 0.1, crlf_rate: float = 0.0) -> str:
    """About ``n_lines`` lines: ``templated_log`` lines with traces of ``sites`` (``trace_sites``)
    planted among them until about ``trace_share`` of the lines belong to a trace."""
    rng = random.Random(seed)
    plain = templated_log(n_lines, templates, seed=seed, crlf_rate=crlf_rate).splitlines(keepends=True)
    mean = sum(len(run) + 1 for _, run in sites) / max(len(sites), 1)
    n_traces = int(n_lines * trace_share / mean)
    keep = max(1, n_lines - int(n_traces * mean))
    at = sorted(rng.randrange(keep) for _ in range(n_traces))
    out, a = [], 0
    for i, pos in enumerate(at):
        out += plain[a:pos]
        a = pos
        head, run = sites[rng.randrange(len(sites))]
        eol = "\r\n" if rng.random() < crlf_rate else "\n"
        out.append(head % ((i // 60) % 60, i % 60, i % 1000, rng.randrange(64)) + eol)
        out += [(x % rng.randrange(1, 2000) if "%d" in x else x) + eol for x in run]
    out += plain[a:keep]
    return "".join(out)
