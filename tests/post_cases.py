"""Helpers and case tables of tests/test_post_oracle.py: a numpy oracle of the post-match stage
(candidates -> sorted unique hits -> events -> frequency ranks -> context coverage), hand-built
pattern tables and segment layouts, and builders of candidate arrays with chosen live-key and
event counts. No tests here.

The oracle is written from the rules, not from the kernels (it imports nothing native):

* a candidate ``regex << 32 | line`` is a hit when it is not dropped (``-1``) and either sits in the
  pre-verified region (index >= pre_from) or its (regex, line) truly matches; hits are the sorted
  unique keys;
* a hit gives one event per pattern whose primary regex it is, on lines its segment owns; events
  come line first, pattern second (AnalysisService.java:89-113);
* the segment of a line is the LAST segment whose ``lo <= line`` (a document without kept lines has
  ``lo == hi`` and never wins over the next one);
* an event's rank is the number of earlier events of its frequency key, ``-1`` without a key
  (penalty before record, ScoringService.java:84-88);
* an event's context window is ``[max(lo, x - before), min(hi, x + 1 + after))`` of its segment, the
  line alone when the pattern has no context rules (AnalysisService.java:132-156).
"""
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

BIG = 1 << 21          # a context window larger than any text used here


# ------------------------------------------------------------------------------------------------
# the oracle
def seg_of(lo: np.ndarray, x: np.ndarray) -> np.ndarray:
    """Last segment whose lo <= x (lo ascending)."""
    return np.maximum(np.searchsorted(lo, x, side="right") - 1, 0)


def oracle(cand, pre_from: int, matches, tabs: Dict[str, np.ndarray], segs, L: int, nkeys: int) -> dict:
    """``matches``: int64 keys of the (regex, line) pairs that truly match. ``segs`` = (lo, hi, own_lo,
    own_hi). Everything returned is an exact integer array (coverage: bool per line)."""
    cand = np.asarray(cand, np.int64)
    lo, hi, olo, ohi = (np.asarray(a, np.int64) for a in segs)
    prim_off = np.asarray(tabs["prim_off"], np.int64)
    R = prim_off.size - 1
    live = cand >= 0
    pre = np.arange(cand.size) >= pre_from
    ok = live & (pre | np.isin(cand, np.asarray(matches, np.int64)))
    hits = np.unique(cand[ok])
    reg, line = hits >> 32, hits & 0xFFFFFFFF
    out = {"hits": hits, "hit_line": line, "nh": int(hits.size),
           "hit_off": np.searchsorted(reg, np.arange(R + 1), side="left")}
    s = seg_of(lo, line)
    owned = (olo[s] <= line) & (line < ohi[s]) if hits.size else np.zeros(0, bool)
    fan = (prim_off[1:] - prim_off[:-1])[reg]
    ev_cnt = np.where(owned, fan, 0)
    out["ev_cnt"], out["ev_end"] = ev_cnt, np.cumsum(ev_cnt)
    ne = int(ev_cnt.sum())
    out["ne"] = ne
    # one event per (hit, pattern of its regex), then line-major, pattern-minor
    h = np.repeat(np.arange(hits.size), ev_cnt)
    within = np.arange(ne) - np.repeat(out["ev_end"] - ev_cnt, ev_cnt)
    e_line = line[h]
    e_pat = np.asarray(tabs["prim_pats"], np.int64)[prim_off[reg[h]] + within]
    order = np.lexsort((e_pat, e_line))
    e_line, e_pat = e_line[order], e_pat[order]
    e_seg = seg_of(lo, e_line)
    out["ev_line"], out["ev_pat"], out["ev_seg"] = e_line, e_pat, e_seg
    # ranks: position among the events of the same key, in event order
    fk = np.asarray(tabs["freq_key"], np.int64)[e_pat]
    rank = np.full(ne, -1, np.int64)
    keyed = np.flatnonzero(fk >= 0)
    if keyed.size:
        o = keyed[np.argsort(fk[keyed], kind="stable")]
        fs = fk[o]
        rank[o] = np.arange(o.size) - np.searchsorted(fs, fs, side="left")
    out["ev_rank"], out["ev_fkey"] = rank, np.where(fk >= 0, fk, -1)
    out["freq_counts"] = np.bincount(fk[fk >= 0], minlength=max(nkeys, 1))[:max(nkeys, 1)]
    # coverage
    before = np.asarray(tabs["ctx_before"], np.int64)[e_pat]
    after = np.asarray(tabs["ctx_after"], np.int64)[e_pat]
    a = np.where(before < 0, e_line, np.maximum(lo[e_seg], e_line - before))
    b = np.where(before < 0, e_line + 1, np.minimum(hi[e_seg], e_line + 1 + after))
    diff = np.zeros(L + 1, np.int64)
    keep = a < b
    np.add.at(diff, a[keep], 1)
    np.add.at(diff, b[keep], -1)
    out["cov"] = np.cumsum(diff)[:L] > 0
    return out


# ------------------------------------------------------------------------------------------------
# hand-built pattern tables over the R regexes of a real library. Regexes 0..3 are the library's four
# context regexes (never a primary role); the user regexes U0.. = 4.. get an invented fan-out.
NCTX = 4
WIDE, BIGW, EDGE, NOROLE, TRI, BARE, DUO, ONE = range(NCTX, NCTX + 8)
DEFAULT_FAN = {WIDE: 8, BIGW: 1, EDGE: 1, NOROLE: 0, TRI: 3, BARE: 1, DUO: 2, ONE: 1}
EDGE_AFTER = 2          # EDGE's pattern: before 1, after 2 -- a hit on hi - 3 ends its window on hi


def make_tables(R: int, fan: Optional[dict] = None, keys: str = "mixed", seed: int = 0) -> dict:
    """prim_off / prim_pats / freq_key / ctx_before / ctx_after as numpy arrays, plus P and nkeys.

    Always present: regexes without a primary role (the context regexes and NOROLE), the 8-pattern
    regex WIDE, patterns without a key, several patterns on one key, a pattern without context rules
    (-1), one with before = after = 0, one whose window exceeds every segment on both sides (BIGW's), one
    with (1, EDGE_AFTER). ``keys``: "mixed", "one" (every pattern on key 0), "own" (a key per pattern),
    "half" (every other pattern without a key). Pattern ids are shuffled over the regexes, so the
    pattern order inside a regex is not the id order of its neighbours."""
    assert R >= NCTX + 8
    f = dict(DEFAULT_FAN)
    f.update(fan or {})
    cnt = np.zeros(R, np.int64)
    for r, c in f.items():
        cnt[r] = c
    P = int(cnt.sum())
    prim_off = np.zeros(R + 1, np.int64)
    np.cumsum(cnt, out=prim_off[1:])
    rng = np.random.default_rng(seed)
    prim_pats = rng.permutation(P).astype(np.int32)
    # (a regex's patterns ascend, as a stable argsort of the patterns' regexes leaves them)
    for r in range(R):
        prim_pats[prim_off[r]:prim_off[r + 1]].sort()
    pat_of = lambda r, j: int(prim_pats[prim_off[r] + j])  # noqa: E731
    before = rng.integers(0, 4, P).astype(np.int32)
    after = rng.integers(0, 4, P).astype(np.int32)
    before[pat_of(WIDE, 0)] = -1
    after[pat_of(WIDE, 0)] = 0
    before[pat_of(WIDE, 1)] = after[pat_of(WIDE, 1)] = 0
    before[pat_of(WIDE, 5)], after[pat_of(WIDE, 5)] = 2, 3         # (a WIDE hit on hi - 1 reaches past hi)
    before[pat_of(BIGW, 0)] = after[pat_of(BIGW, 0)] = BIG
    before[pat_of(EDGE, 0)], after[pat_of(EDGE, 0)] = 1, EDGE_AFTER
    before[pat_of(BARE, 0)] = -1
    if keys == "one":
        fk, nkeys = np.zeros(P, np.int32), 3
    elif keys == "own":
        fk, nkeys = rng.permutation(P).astype(np.int32), P
    elif keys == "half":
        fk = np.where(np.arange(P) % 2 == 0, rng.integers(0, 5, P), -1).astype(np.int32)
        nkeys = 5
    elif keys == "burst":         # WIDE's patterns alone on key 0
        nkeys = 6
        fk = rng.integers(1, nkeys, P).astype(np.int32)
        fk[prim_pats[prim_off[WIDE]:prim_off[WIDE + 1]]] = 0
    else:
        nkeys = 6
        fk = rng.integers(0, nkeys - 1, P).astype(np.int32)      # (key nkeys - 1 stays unused: count 0)
        fk[pat_of(WIDE, 2)] = fk[pat_of(WIDE, 3)] = fk[pat_of(BIGW, 0)] = 0     # shared key
        fk[pat_of(WIDE, 4)] = fk[pat_of(BARE, 0)] = -1                           # no key
    return {"prim_off": prim_off, "prim_pats": prim_pats, "freq_key": fk, "ctx_before": before,
            "ctx_after": after, "P": P, "nkeys": int(nkeys), "R": R}


# ------------------------------------------------------------------------------------------------
# segment layouts: (lo, hi, own_lo, own_hi)
def make_segments(layout: str, L: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    if layout == "one" or L < 16:
        return tuple(np.array(v, np.int32) for v in ([0], [L], [0], [L]))
    c1, c2 = sorted(int(c) for c in rng.choice(np.arange(5, L - 5), 2, replace=False))
    b = [0, c1, c2, L]
    if layout == "halo":          # halos on both sides of every segment (tests/test_post.py _segments)
        lo, hi = b[:3], b[1:]
        olo = [min(lo[i] + int(rng.integers(0, 6)), hi[i]) for i in range(3)]
        ohi = [max(hi[i] - int(rng.integers(0, 6)), olo[i]) for i in range(3)]
    elif layout == "three":       # halo in front only: every segment owns its last line
        lo, hi = b[:3], b[1:]
        olo, ohi = [0, min(c1 + 3, c2), min(c2 + 2, L)], list(hi)
    elif layout == "zero":        # a document without kept lines between two others
        lo, hi = [0, c1, c1], [c1, c1, L]
        olo, ohi = list(lo), list(hi)
    elif layout == "noown":       # the middle segment owns nothing
        lo, hi = b[:3], b[1:]
        olo, ohi = [0, c1, c2], [c1, c1, L]
    else:
        raise ValueError(layout)
    return tuple(np.array(v, np.int32) for v in (lo, hi, olo, ohi))


def key(r, x):
    return (np.asarray(r, np.int64) << 32) | np.asarray(x, np.int64)


def owned_lines(segs, L: int) -> np.ndarray:
    lo, hi, olo, ohi = (np.asarray(a, np.int64) for a in segs)
    x = np.arange(L)
    s = seg_of(lo, x)
    return x[(olo[s] <= x) & (x < ohi[s])]


def edge_hits(segs, L: int) -> np.ndarray:
    """Hits on the first and the last line of every segment (EDGE, and NOROLE / BARE), on line 0 and
    L - 1, one whose window ends exactly on hi (EDGE on hi - 1 - EDGE_AFTER) and one with a window larger
    than its segment (BIGW in the middle of the largest segment)."""
    lo, hi = (np.asarray(a, np.int64) for a in segs[:2])
    ks = [key(EDGE, 0), key(EDGE, L - 1), key(NOROLE, 0), key(BARE, L - 1)]
    for a, b in zip(lo, hi):
        if b > a:
            ks += [key(EDGE, a), key(EDGE, b - 1), key(NOROLE, b - 1), key(BARE, a)]
            if b - 1 - EDGE_AFTER >= a:
                ks.append(key(EDGE, b - 1 - EDGE_AFTER))
    big = int(np.argmax(hi - lo))
    ks.append(key(BIGW, (lo[big] + hi[big]) // 2))
    return np.unique(np.array(ks, np.int64))


# ------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One input of the post-match stage. ``text`` None: L empty lines (nothing matches there, so
    only pre-verified candidates survive)."""
    cand: np.ndarray
    pre_from: int
    tabs: dict
    segs: tuple
    L: int
    matches: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    text: Optional[bytes] = None          # real text: line starts / lengths come from ls / ll
    ls: Optional[np.ndarray] = None
    ll: Optional[np.ndarray] = None

    def expect(self) -> dict:
        return oracle(self.cand, self.pre_from, self.matches, self.tabs, self.segs, self.L, self.tabs["nkeys"])


def shuffled(keys: np.ndarray, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).permutation(np.asarray(keys, np.int64))


def pad_to(cand: np.ndarray, n: int, seed: int = 0) -> np.ndarray:
    """The same live keys among -1 (dropped) entries, n entries in all, in a shuffled order."""
    assert cand.size <= n
    return shuffled(np.concatenate([cand, np.full(n - cand.size, -1, np.int64)]), seed)


def distinct_keys(count: int, L: int, seed: int, regs=(WIDE, BIGW, EDGE, NOROLE, TRI, BARE, DUO, ONE),
                  exclude: Optional[np.ndarray] = None) -> np.ndarray:
    """`count` distinct (regex, line) keys of the user regexes, none of `exclude`."""
    rng = np.random.default_rng(seed)
    regs = np.asarray(regs, np.int64)
    total = regs.size * L
    want = count + (0 if exclude is None else exclude.size)
    assert want <= total
    flat = rng.choice(total, want, replace=False)
    ks = key(regs[flat // L], flat % L)
    if exclude is not None:
        ks = ks[~np.isin(ks, exclude)]
    return ks[:count]


def live_keys_case(count: int, dup: str, layout: str, L: int, R: int, seed: int = 0) -> Case:
    """Exactly `count` live, pre-verified candidates. dup: "none" (all distinct), "twice" (every key
    twice), "fill" (one key repeated), with the layout's edge hits among them when they fit."""
    segs = make_segments(layout, L, seed)
    tabs = make_tables(R, seed=seed)
    if dup == "fill":
        ks = np.full(count, key(WIDE, owned_lines(segs, L)[-1]), np.int64)
    else:
        nd = count if dup == "none" else (count + 1) // 2
        base = edge_hits(segs, L)
        base = base[:nd] if base.size > nd else base
        ks = np.concatenate([base, distinct_keys(nd - base.size, L, seed + 1, exclude=base)])
        if dup == "twice":
            ks = np.concatenate([ks, ks])[:count]
    return Case(shuffled(ks, seed + 2), 0, tabs, segs, L)


def events_case(ne: Optional[int], layout: str, L: int, R: int, keys: str = "mixed", seed: int = 0, fan=None,
                extra: Optional[np.ndarray] = None) -> Case:
    """Hits chosen so that exactly `ne` events come out (checked by the tests against the oracle's own
    count): the layout's edge hits when their events fit, WIDE hits (8 events each) on owned lines,
    ONE hits for the remainder. Every hit appears one to three times, all pre-verified."""
    segs = make_segments(layout, L, seed)
    tabs = make_tables(R, fan=fan, keys=keys, seed=seed)
    probe = lambda ks: Case(ks, 0, tabs, segs, L).expect()["ne"]  # noqa: E731
    base = edge_hits(segs, L) if extra is None else np.unique(np.concatenate([edge_hits(segs, L), extra]))
    own = owned_lines(segs, L)
    if ne is None:                # no target: the edge hits, up to five WIDE hits and three ONE hits
        ne = probe(base) + 8 * min(5, own.size) + min(3, own.size)
    if probe(base) > ne:
        base = np.array([key(NOROLE, 0)], np.int64)
    rest = ne - probe(base)
    wide_fan, one_fan = int(np.diff(tabs["prim_off"])[WIDE]), int(np.diff(tabs["prim_off"])[ONE])
    assert one_fan == 1
    nw = min(rest // wide_fan, own.size)
    n1 = rest - nw * wide_fan
    assert n1 <= own.size, "not enough owned lines for this many events"
    rng = np.random.default_rng(seed + 3)
    # WIDE hits from the end of the owned lines (so the last owned line has events), ONE from the front
    ks = np.concatenate([base, key(WIDE, own[own.size - nw:]), key(ONE, own[:n1])])
    ks = np.concatenate([ks, ks[rng.random(ks.size) < 0.5], ks[rng.random(ks.size) < 0.25]])
    return Case(shuffled(ks, seed + 4), 0, tabs, segs, L)


# ------------------------------------------------------------------------------------------------
# a real, small library and text for the unverified region: eight user regexes (every one a plain
# DFA regex, so `dfa_find` on the host and Python's `re` both decide a (regex, line) pair)
REAL_PATTERNS = [r"alpha\d", "bravo failed", r"charlie\s+down", "delta|omega", "echo [a-f]+ lost", "foxtrot",
                 "golf$", "^hotel"]
_PHRASES = ["alpha7 up", "bravo failed again", "charlie   down", "an omega event", "echo abc lost", "xx foxtrot xx",
            "played golf", "hotel first", "alpha x", "bravo fail", "charliedown", "delta and alpha1", "echo xyz lost",
            "golf club", "the hotel", "", "nothing here", "foxtrot golf"]


def real_library_spec() -> dict:
    pats = [{"id": f"p{i}", "name": f"pattern {i}", "severity": "HIGH",
             "primary_pattern": {"regex": rx, "confidence": 0.5}} for i, rx in enumerate(REAL_PATTERNS)]
    return {"metadata": {"library_id": "post-oracle", "version": "1"}, "patterns": pats}


def real_lines(L: int = 48):
    phrase = [_PHRASES[i % len(_PHRASES)] for i in range(L)]
    return [("" if p in ("", "hotel first") else f"{i:02d} ") + p for i, p in enumerate(phrase)]


def mixed_region_case(count: int, truth: np.ndarray, L: int, R: int, text: bytes, ls, ll, layout: str = "one",
                      seed: int = 0, pad1: int = 0) -> Case:
    """Unverified and pre-verified copies over real text, `count` live keys after verification: the
    unverified region holds matching pairs (some twice) and pairs that do not match; the pre-verified
    region holds copies of matching pairs of the first region, a matching pair of its own and two
    NON-matching pairs (kept: a pre-verified copy is trusted), one of which the unverified region
    holds too. ``pad1``: dropped (-1) entries mixed into the unverified region."""
    rng = np.random.default_rng(seed)
    pairs = key(np.repeat(np.arange(NCTX, NCTX + 8), L), np.tile(np.arange(L), 8))
    yes = pairs[np.isin(pairs, truth)]
    no = pairs[~np.isin(pairs, truth)]
    assert yes.size > 8 and no.size > 8
    only_pre, lone_no, both_no = yes[-1], no[-1], no[-2]
    yes, no = yes[:-1], no[:-2]
    n_pre = max(3, count // 3)
    n_ver = count - n_pre
    ver = np.concatenate([rng.choice(yes, n_ver), rng.choice(no, max(1, count // 4)), [both_no, both_no],
                          np.full(pad1, -1, np.int64)])
    pre = np.concatenate([[only_pre, lone_no, both_no], rng.choice(ver[:n_ver], n_pre - 3)])
    ver, pre = shuffled(ver, seed + 1), shuffled(pre, seed + 2)
    return Case(np.concatenate([ver, pre]), int(ver.size), make_tables(R, seed=seed), make_segments(layout, L, seed),
                L, matches=truth, text=text, ls=np.asarray(ls, np.int64), ll=np.asarray(ll, np.int32))


# ------------------------------------------------------------------------------------------------
# skew: bursts in a 2^20-line text of empty lines, every candidate pre-verified
LBIG = 1 << 20
QUIET = 8192            # no background hit on the first or the last QUIET lines


def background(n: int, seed: int, regs=(NOROLE, BARE, DUO, ONE, EDGE)) -> np.ndarray:
    """About n evenly spread hits of other regexes, none within QUIET lines of either end."""
    rng = np.random.default_rng(seed)
    x = QUIET + (np.arange(n) * (LBIG - 2 * QUIET)) // n + rng.integers(0, 8, n)
    return np.unique(key(np.asarray(regs, np.int64)[np.arange(n) % len(regs)], x))


def end_burst(lines: int, copies: int) -> np.ndarray:
    """TRI on the last `lines` lines of the text, line LBIG - 1 included, `copies` candidates each."""
    return np.tile(key(TRI, np.arange(LBIG - lines, LBIG)), copies)


def hit_burst_case(m: int, R: int, seed: int = 0, keys: str = "mixed") -> Case:
    """m candidates of WIDE on m // 4 consecutive lines from line 100 on, 3 to 5 copies of each, a
    second burst (TRI, 3 copies of each of the last 1500 lines) and the background."""
    nd = m // 4
    copies = np.full(nd, 4, np.int64)
    copies[:m - 4 * nd] += 1
    copies[nd // 2] -= 1        # ... one line 3 times, another 5 times
    copies[nd // 2 + 1] += 1
    assert copies.sum() == m and copies.min() >= 3 and copies.max() <= 5
    burst = np.repeat(key(WIDE, 100 + np.arange(nd)), copies)
    ks = np.concatenate([burst, end_burst(1500, 3), background(20000, seed), [key(BIGW, LBIG // 2)]])
    return Case(shuffled(ks, seed + 1), 0, make_tables(R, keys=keys, seed=seed), make_segments("one", LBIG), LBIG)


def event_burst_case(target: int, R: int, seed: int = 0, keys: str = "mixed", bg: int = 20000) -> Case:
    """`target` events on the first lines of the text: WIDE on target // 8 consecutive lines from line
    0, ONE on the next target % 8 lines; nothing else below line QUIET. A second burst of 700 x 3 events
    on the last lines, and the background."""
    nw, n1 = target // 8, target % 8
    ks = np.concatenate([key(WIDE, np.arange(nw)), key(ONE, nw + np.arange(n1)), end_burst(700, 2),
                         background(bg, seed, regs=(NOROLE, BARE, DUO, EDGE)), [key(BIGW, LBIG // 2)]])
    ks = np.concatenate([ks, ks[::3]])
    return Case(shuffled(ks, seed + 1), 0, make_tables(R, keys=keys, seed=seed), make_segments("one", LBIG), LBIG)


def many_keys_case(R: int, seed: int = 0) -> Case:
    """20,000 patterns, each with its own frequency key, over the user regexes; three owned lines
    hit by every regex: 60,000 events, every key with ranks 0, 1, 2."""
    fan = {r: 3332 for r in (BIGW, EDGE, TRI, BARE, DUO, ONE)}
    tabs = make_tables(R, fan=fan, keys="own", seed=seed)
    assert tabs["P"] == 20000 and tabs["nkeys"] == 20000
    L = 1000
    segs = make_segments("three", L, seed)
    own = owned_lines(segs, L)
    lines = own[[0, own.size // 2, own.size - 1]]
    ks = key(np.repeat(np.arange(NCTX, NCTX + 8), 3), np.tile(lines, 8))
    return Case(shuffled(np.concatenate([ks, ks[::2]]), seed), 0, tabs, segs, L)


def many_buckets_case(R: int, seed: int = 0, distinct: int = 50000) -> Case:
    """Just over (16384 - R) * 512 pre-verified candidates drawn with heavy repetition from `distinct`
    (regex, line) pairs of a 2^16-line text: the hit planner's sub-bucket capacity passes 16384."""
    L = 1 << 16
    n = (16384 - R) * 512 + 1024
    pool = distinct_keys(distinct, L, seed)
    rng = np.random.default_rng(seed + 1)
    return Case(pool[rng.integers(0, pool.size, n)], 0, make_tables(R, seed=seed), make_segments("three", L, seed), L)
