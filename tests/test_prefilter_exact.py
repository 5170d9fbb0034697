"""Literal prefilter and verify against an exact search (golden.literal_candidates), for the host twin
and for every k_prefilter / k_pf_verify variant on the device.

The contract: the candidates of ops.kernels.prefilter are, as a MULTISET of keys regex << 32 | line,
one key per (literal, overlapping occurrence in the ASCII-lower-cased text, regex of the literal),
with line = the last line start <= the occurrence's first byte. The texts below sit on the edges of
that code: the text's first and last bytes, 16-byte units, block iterations (512 or 1024 lanes x 16
bytes, x 4 when unrolled), 4 KiB line blocks, literal lengths in every residue mod 16, the bytes next
to A..Z, lines longer than a block and hundreds of lines inside one, more hits per block iteration
than the LDS staging buffer holds, and capacities far too small (cap = 64: every buffer re-runs).

Which case reaches what: k_prefilter<GM, S, TD> = the rows bloom_s4 / s2 / s1 (16, S, no Teddy), gram3
(24, 1), teddy_only (0, Teddy), teddy_s4 / s2 / g34 (16 / 16 / 24 with Teddy); PF_UNROLL = 1 in
test_device_candidates_*, 4 in test_bulk_variants_* (64 MiB); k_pf_verify<16> in every small test,
<16 / 4 / 2 / 1> in the bulk test; the LDS staging spill of k_prefilter in the dense cases at grid 1
and in the bulk text's dense stretch, that of k_pf_verify in the dense fan-out texts (1024 hits x 40
regexes; at 1 lane a block takes 256 hits per iteration); the byte-wise context load (a hit at
p < 4) in the "at 0..3" texts and, at every PV_LANES, at byte 0 of the bulk text.

Every text buffer is zero padded to ops.kernels.padded_len: the kernels read past nbytes by design."""
import collections
import functools
import re

import numpy as np
import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.models import compiled as C
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.native import N
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import ScoringParams

CPU = torch.device("cpu")
BORDERS = (16, 4096, 8192, 16384, 32768, 65536)      # 16384 = the Teddy variant's block span, 1024 x 16


# ------------------------------------------------------------------ libraries
def _rx(lit: bytes, ci: bool = False) -> str:
    """Regex (valid for the Java front end and for Python's re) that matches the bytes `lit` literally."""
    out = []
    for ch in lit.decode("utf-8"):
        if ch.isalnum() or ch == " ":
            out.append(ch)
        elif " " < ch < "\x7f":
            out.append("\\" + ch)
        else:
            out.append("\\x%02x" % ord(ch))
    return ("(?i)" if ci else "") + "".join(out)


def _compile(regexes, teddy, smax, full_lits=None):
    """`full_lits`: the regex front end keeps at most 32 bytes of a literal, the prefilter tables and
    kernels have no such limit: each regex's literal is replaced by the one of `full_lits` it starts,
    and the prefilter tables are built again (prefilter-only libraries: the DFAs keep the regexes)."""
    doc = {"metadata": {"library_id": "exact"}, "patterns": [
        {"id": "p%d" % i, "name": "literal %d" % i, "severity": "HIGH",
         "primary_pattern": {"regex": r, "confidence": 0.9}} for i, r in enumerate(regexes)]}
    old = C.PF_STRIDE_MAX, C.PF_TEDDY
    try:
        C.PF_STRIDE_MAX, C.PF_TEDDY = smax, teddy
        lib = C.CompiledLibrary([PatternSet.model_validate(doc)], ScoringParams())
        if full_lits:
            for ri in lib.regexes:
                ri.literals = [next(f for f in full_lits if f.startswith(l)) for l in ri.literals]
            lib._build_prefilter()
            lib._device_cache.clear()
            assert sorted(lib.literals) == sorted(full_lits)         # every literal at its full length
        return lib
    finally:
        C.PF_STRIDE_MAX, C.PF_TEDDY = old


LONG = [b"segfault at", b"kernel panic - not syncing", b"disk quota 9 exceeded"]


def _row(lits, teddy, smax, **expect):
    """One variant row: plain-literal regexes (every second one (?i)) + what lib.pf must show."""
    return dict(regexes=[_rx(l, ci=i % 2 == 1) for i, l in enumerate(lits)], teddy=teddy, smax=smax, expect=expect)


ROWS = {
    "bloom_s4": _row(LONG, False, 4, gmask=16, stride=4, teddy_lits=0),
    "bloom_s2": _row(LONG, False, 2, gmask=16, stride=2, teddy_lits=0),
    "bloom_s1": _row(LONG, False, 1, gmask=16, stride=1, teddy_lits=0),
    "gram3": _row([b"oom", b"out of memory: kill"], False, 4, gmask=24, stride=1, teddy_lits=0),
    "teddy_only": _row([b"OOMKil", b"qx7"], True, 4, gmask=0, teddy_lits=2),
    "teddy_s4": _row([b"qx7", b"segfault at", b"kernel panic - not syncing"], True, 4,
                     gmask=16, stride=4, teddy_lits=1),
    # a NUL keeps a short literal off the Teddy tier: 5 bytes on the bloom tier -> stride 2
    "teddy_s2": _row([b"ab\x00cd", b"qx7", b"verylongliteral"], True, 4, gmask=16, stride=2, teddy_lits=1),
    "teddy_g34": _row([b"a\x00b", b"qx7", b"one long literal"], True, 4, gmask=24, stride=1, teddy_lits=1),
}


def _mix(lit: bytes) -> bytes:
    """Mixed case: every second ASCII letter upper-cased."""
    return bytes(c - 32 if 97 <= c <= 122 and i % 2 == 0 else c for i, c in enumerate(lit))


# ------------------------------------------------------------------ texts
def _start_end_texts(lit):
    """The text's first and last bytes: (label, text, holds no occurrence)."""
    for p in range(20):
        yield "at %d" % p, b"x" * p + lit + b" tail\nnext line\n", False
    yield "whole text", lit, False
    for n in range(40):
        yield "ends the text, %d before" % n, b"x" * n + _mix(lit), False
        yield "cut off by the text end, %d before" % n, b"x" * n + _mix(lit)[:-1], True
        yield "after %d empty lines" % n, b"\n" * n + lit + b"\n\n\n", False


def _border_texts(lit):
    """For every j one text with an occurrence starting at B - j for every border B, each on a line of its own."""
    size = BORDERS[-1] + len(lit) + 40
    fill = bytearray(b"z" * size)
    fill[96::97] = b"\n" * len(fill[96::97])
    for j in range(len(lit) + 1):
        buf = bytearray(fill)
        for B in BORDERS:
            s = B - j
            if s < 0:
                continue
            if s:
                buf[s - 1] = 10
            buf[s:s + len(lit)] = _mix(lit) if j % 2 else lit
            buf[s + len(lit)] = 10
        yield "borders - %d" % j, bytes(buf), False


def _line_texts(lit):
    gap = (20480 - 3 * len(lit)) // 2
    long_line = lit + b"y" * gap + _mix(lit) + b"y" * (20480 - 3 * len(lit) - gap) + lit
    yield "20 KiB line", b"short\n" + long_line + b"\nafter " + lit + b"\n", False
    yield "3000 two-byte lines", b"a\n" * 3000 + lit + b"\nend\n", False
    yield "empty lines and CRLF", b"\n\n" + lit + b"\r\n\r\n" + _mix(lit) + b"\n\r\n\nx" + lit + b"\r\n", False
    yield "unterminated last line", b"first\nsecond\n" + lit, False


def _row_texts(lits):
    out = []
    for lit in lits:
        for build in (_start_end_texts, _border_texts, _line_texts):
            out += [("%r %s" % (lit, label), text, empty) for label, text, empty in build(lit)]
    return out


def _length_lits():
    """Literals of every length 7..40 and one of 300 bytes; none is part of another (the digits)."""
    def body(n, k):
        return bytes(97 + (k * 7 + i * (3 + k % 5)) % 26 for i in range(n))
    return [b"k%02d" % n + body(n - 3, n) for n in range(7, 41)] + [b"w300 " + body(295, 1)]


def _flip(lit, i):
    """`lit` with byte i replaced by one that differs from it in either case."""
    return lit[:i] + (b"_" if lit[i:i + 1] != b"_" else b"-") + lit[i + 1:]


def _length_texts(lits):
    lines = []
    for k, lit in enumerate(lits):                   # every alignment mod 16 of start and end
        lines.append(b"p" * (k % 17) + (_mix(lit) if k % 2 else lit) + b"q" * (k % 3))
        lines.append(b"p" * ((5 * k) % 16) + _flip(lit, len(lit) - 1) + lit[-1:])     # last byte wrong
        lines.append(_flip(lit, 0) + b" " + lit[:-1])                               # first byte wrong / cut
    hits = b"\n".join(lines)
    l40 = lits[40 - 7]
    assert len(l40) == 40
    miss = b"\n".join(b"r" * (i % 16) + _flip(l40, i) for i in range(40))
    return [("every length", hits, False), ("one byte off", miss, True),
            ("one byte off + the literal", miss + b"\n" + l40, False)]


CASE_LITS = [b"err{code}", b"tick`mark", b"user@host", b"a[bc]de fgh", b"a{b", b"q@z", b"caf\xc3\xa9 latte"]
_SWAP = bytes.maketrans(b"{}`@[]", b"[]@`{}")


def _case_texts(lits):
    lines = []
    for lit in lits:
        lines += [lit, lit.upper(), _mix(lit), lit.translate(_SWAP), lit.upper().translate(_SWAP),
                  b"\xe9" + lit + b"\xe9", b"\xc9" + lit.upper() + b"\xc9", b"x\xe9" + lit[:-1] + b"\xe9"]
    lines.append(b"CAF\xc3\x89 LATTE and caf\xc3\x89 latte and CAF\xc3\xa9 LATTE")    # only the last one folds
    return [("case neighbours", b"\n".join(lines), False)]


def _dense_texts(_lits):
    return [("64 KiB of a", b"a" * 65536, False), ("AB repeated", b"AB" * 32768, False)]


CROWD_LITS = [b"error %02d happened" % i for i in range(100)]


def _crowd_texts(lits):
    lines = [(_mix(l) if i % 3 == 0 else l) + b" #%d" % i for i, l in enumerate(lits)]
    lines += [b"error 1x happened", b"error 100 happened", b"eRRor 07 happene", b"error 42 happenederror 43 happened"]
    return [("crowded bucket", b"\n".join(lines), False)]


FAN_REGEXES = ["(shared literal|uniq%03dzz)" % i for i in range(40)]
FAN_DENSE = b"shared literal. "                   # 16 bytes


def _fan_texts(_lits):
    lines = [b"a shared literal", b"uniq007zz", b"SHARED LITERAL shared literal", b"shared litera",
             b"uniq039zz uniq000zz"]
    # 1024 hits x 40 regexes: more candidates per k_pf_verify block iteration than its LDS buffer holds
    return [("fan-out", b"\n".join(lines), False), ("fan-out, dense", FAN_DENSE * 1024 + b"\n", False)]


def _lits_case(lits, teddy, smax, texts, full=False, **expect):
    return dict(regexes=[_rx(l, ci=i % 2 == 1) for i, l in enumerate(lits)], teddy=teddy, smax=smax,
                expect=expect, texts=texts, full_lits=lits if full else None)


CASES = {name: dict(row, texts=_row_texts) for name, row in ROWS.items()}
CASES.update({
    "lengths_s4": _lits_case(_length_lits(), True, 4, _length_texts, full=True, gmask=16, stride=4, teddy_lits=0),
    "lengths_s1": _lits_case(_length_lits(), True, 1, _length_texts, full=True, gmask=16, stride=1, teddy_lits=0),
    "case_teddy": _lits_case(CASE_LITS, True, 4, _case_texts, gmask=16, stride=4, teddy_lits=2),
    "case_s1": _lits_case(CASE_LITS, False, 1, _case_texts, gmask=24, stride=1, teddy_lits=0),
    "dense_s1": _lits_case([b"aaaaaaaaa", b"abababababab"], False, 1, _dense_texts, gmask=16, stride=1),
    "dense_s2": _lits_case([b"aaaaaaaaa", b"abababababab"], False, 2, _dense_texts, gmask=16, stride=2),
    "dense_s4": _lits_case([b"aaaaaaaaa", b"abababababab"], True, 4, _dense_texts, gmask=16, stride=4),
    "crowded": _lits_case(CROWD_LITS, True, 4, _crowd_texts, gmask=16, stride=4),
    # (bulk text too: with the two literals that start and end that text)
    "crowded10": _lits_case(CROWD_LITS[:10] + LONG[:2], True, 4, _crowd_texts, gmask=16, stride=4),
    "fanout": dict(regexes=FAN_REGEXES, teddy=True, smax=4, expect=dict(gmask=16, stride=4), texts=_fan_texts),
})


class Case:
    """A compiled library, its texts and (computed once, shared by the CPU and GPU tests) their oracles."""

    def __init__(self, name):
        spec = CASES[name]
        self.name, self.regexes = name, spec["regexes"]
        self.lib = _compile(spec["regexes"], spec["teddy"], spec["smax"], spec.get("full_lits"))
        self.expect = spec["expect"]
        self.texts = spec["texts"](self.lib.literals)
        self._want = {}

    def check_variant(self):
        """The library reached the kernel variant this case is about."""
        for k, v in self.expect.items():
            assert self.lib.pf[k] == v, (self.name, k, self.lib.pf[k])
        assert all(l == l.lower() for l in self.lib.literals)

    def want(self, i):
        if i not in self._want:
            _, data, empty = self.texts[i]
            t = _text(data)
            ls, _ = K.split_lines(t, len(data))
            w = golden.literal_candidates(self.lib, data, ls)
            assert bool(w) != empty, (self.name, self.texts[i][0])
            self._want[i] = (w, ls)
        return self._want[i]


@functools.lru_cache(maxsize=None)
def _case(name) -> Case:
    return Case(name)


def _text(data: bytes, dev=None):
    t = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return t if dev is None else t.to(dev)


def _explain(got, want):
    def keys(c):
        return [(k >> 32, k & 0xFFFFFFFF, n) for k, n in sorted(c.items())[:8]]
    return "missing (regex, line, n) %s, extra %s" % (keys(want - got), keys(got - want))


def _assert_same(got, want, what):
    assert set(got) == set(want), "%s: key sets differ: %s" % (what, _explain(got, want))
    assert got == want, "%s: multiplicities differ: %s" % (what, _explain(got, want))


# ------------------------------------------------------------------ CPU: the host twin
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_candidates_equal_the_exact_search(name):
    case = _case(name)
    case.check_variant()
    pf = case.lib.device_tables(CPU)["pf"]
    total = 0
    for i, (label, data, _) in enumerate(case.texts):
        want, ls = case.want(i)
        t = _text(data)
        got = collections.Counter(K.prefilter(t, len(data), pf, ls, 64).tolist())
        _assert_same(got, want, "%s / %s" % (name, label))
        total += sum(want.values())
    assert total > 0


def test_crowded_bucket_and_fan_out_are_what_they_claim():
    assert int(_case("crowded").lib.pf["ht_cnt"].max()) > 16           # a bucket far larger than PV_LANES
    assert int(_case("crowded10").lib.pf["ht_cnt"].max()) > 4          # larger than the bulk step's PV_LANES
    fan = _case("fanout").lib
    i = fan.literals.index(b"shared literal")
    assert int(fan.pf["lit_reg_off"][i + 1] - fan.pf["lit_reg_off"][i]) == 40
    want, _ = _case("fanout").want(0)
    assert sum(want.values()) == 3 * 40 + 3
    dense = _case("dense_s1")
    assert sum(dense.want(0)[0].values()) == 65536 - 8 and sum(dense.want(1)[0].values()) == 32768 - 5


def _occurrences(lib, data):
    low = data.lower()
    for i, lit in enumerate(lib.literals):
        p = low.find(lit)
        while p >= 0:
            yield i, p
            p = low.find(lit, p + 1)


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if not n.startswith("dense")])
def test_fingerprints_pass_every_occurrence_of_the_texts(name):
    """k_pf_verify drops a bucket entry whose fingerprint (the literal's bytes in the 4 text positions
    before and the 4 after the indexed window, models/compiled.py _fingerprint) disagrees with the
    lower-cased text, where bytes outside the text read as 0. The host twin has no fingerprints, so this
    is a model of that comparison (keep it in step with k_pf_verify's t8) run on the tables: no entry of
    a literal may reject an occurrence of it, at the text's ends and next to bytes >= 0x80 as well."""
    case = _case(name)
    pf, lits = case.lib.pf, case.lib.literals
    ents = {}
    ntb = int(pf["tb_off"][-1])
    for tab, fps, gs, n in ((pf["gram_lits"], pf["gram_fp"], pf["gram_g"], len(pf["gram_lits"]) if pf["gmask"] else 0),
                            (pf["tb_lits"], pf["tb_fp"], [3] * ntb, ntb)):
        for j in range(n):
            e = int(tab[j])
            ents.setdefault(e & ((1 << C.LIT_OFF_SHIFT) - 1), []).append(
                (e >> C.LIT_OFF_SHIFT, int(gs[j]), int(fps[2 * j]), int(fps[2 * j + 1])))
    assert set(ents) == set(range(len(lits)))
    checked = 0
    for _, data, _ in case.texts:
        low = data.lower()

        def byte(x):
            return low[x] if 0 <= x < len(low) else 0
        for i, st in _occurrences(case.lib, data):
            for off, g, fp, mask in ents[i]:
                p = st + off
                t8 = sum(byte(p - 4 + k) << (8 * k) for k in range(4)) | \
                    sum(byte(p + g + k) << (32 + 8 * k) for k in range(4))
                assert (t8 ^ fp) & mask == 0, (name, lits[i], st, off)
                checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", ["bloom_s4", "teddy_s4", "gram3"])
def test_locate_line_with_the_block_index_equals_a_search_of_all_lines(name):
    """lp_core.h locate_line with the coarse 4 KiB block index (the device verify's line lookup): equal
    to a search over all line starts, at every occurrence, line start and block border of the texts."""
    case = _case(name)
    n_pos = 0
    for i, (label, data, _) in enumerate(case.texts):
        _, ls = case.want(i)
        n = len(data)
        blk = K.line_block_index(ls, n)
        lsn = ls.numpy()
        pos = [p for _, p in _occurrences(case.lib, data)] + lsn.tolist() + (lsn - 1).tolist()
        for b in range(0, n + 4096, 4096):
            pos += [b - 1, b, b + 1]
        pos = torch.tensor(sorted(set(p for p in pos if 0 <= p < n)), dtype=torch.int64)
        want = np.maximum(np.searchsorted(lsn, pos.numpy(), side="right") - 1, 0)
        for b in (blk.data_ptr(), 0):
            out = torch.empty_like(pos)
            N.locate_lines_host(ls.data_ptr(), ls.numel(), b, pos.data_ptr(), pos.numel(), out.data_ptr())
            np.testing.assert_array_equal(out.numpy(), want, err_msg="%s / %s" % (name, label))
        n_pos += pos.numel()
    assert n_pos > 1000


# ------------------------------------------------------------------ large sparse texts
def _filler(n, seed):
    """a-z with a '\\n' about every 80 bytes: a literal holding a digit or a blank cannot occur by chance."""
    rng = np.random.default_rng(seed)
    a = rng.integers(97, 123, n, dtype=np.uint8)
    a[rng.integers(0, n, n // 80)] = 10
    return a


def _plant(a, pos, lit):
    """`lit` at `pos`, on a line of its own."""
    n = len(a)
    assert 0 <= pos and pos + len(lit) <= n
    if pos:
        a[pos - 1] = 10
    a[pos:pos + len(lit)] = np.frombuffer(lit, np.uint8)
    if pos + len(lit) < n:
        a[pos + len(lit)] = 10


def _first_window(lib):
    """Per literal: the smallest offset of an indexed window (bloom tier), or its Teddy window's."""
    pf, out = lib.pf, {}
    ntb = int(pf["tb_off"][-1])
    for tab, n in ((pf["gram_lits"], len(pf["gram_lits"]) if pf["gmask"] else 0), (pf["tb_lits"], ntb)):
        for e in tab[:n].tolist():
            i, o = e & ((1 << C.LIT_OFF_SHIFT) - 1), e >> C.LIT_OFF_SHIFT
            out[lib.literals[i]] = min(o, out.get(lib.literals[i], o))
    return out


def _sparse_text(n, lits, seed, window_at=(), first_window=None, dense=(), first=None, last=None):
    """Filler with an occurrence across every 4 KiB border (start = border - j, j cycling through
    0..len), `first` (default: lits[0]) at byte 0 and `last` (lits[-1]) ending on the last byte; at
    every position of `window_at` an occurrence whose first indexed window (`first_window`) starts
    exactly there; `dense`: (position, 16-byte unit, length) stretches of the unit repeated."""
    a = _filler(n, seed)
    taken = np.zeros(n, bool)
    for i, B in enumerate(sorted(set(window_at))):
        lit = lits[i % len(lits)]
        s = B - first_window[lit]
        if taken[s - 1:s + len(lit) + 1].any():
            continue
        taken[s - 64:s + len(lit) + 64] = True
        _plant(a, s, lit)
    for i, B in enumerate(range(4096, n - 4096, 4096)):
        if any(at - 4096 <= B <= at + size + 4096 for at, _, size in dense):
            continue
        lit = lits[i % len(lits)]
        j = (i // len(lits) + i // 16 + i // 64) % (len(lit) + 1)
        if not taken[B - j - 1:B - j + len(lit) + 1].any():
            _plant(a, B - j, _mix(lit) if i % 5 == 0 else lit)
    for at, unit, size in dense:
        assert len(unit) == 16 and size % 16 == 0
        a[at:at + size] = np.frombuffer(unit * (size // 16), np.uint8)
    first, last = first or lits[0], last or lits[-1]
    _plant(a, 0, first)
    _plant(a, n - len(last), last)
    return a


BIG_N = (9 << 20) + 3                        # odd halves, thirds, ...: chunk borders off the stride


@functools.lru_cache(maxsize=None)
def _big_cpu(name):
    lib = _case(name).lib
    chunks = [BIG_N * t // T for T in range(2, 17) for t in range(1, T)]       # host_parallel's chunk borders
    a = _sparse_text(BIG_N, lib.literals, 7, window_at=chunks, first_window=_first_window(lib))
    t = torch.zeros(K.padded_len(BIG_N), dtype=torch.uint8)
    t[:BIG_N] = torch.from_numpy(a)
    ls, _ = K.split_lines(t, BIG_N)
    return t, ls, a.tobytes()


@pytest.mark.parametrize("name", ["bloom_s4", "bloom_s2", "bloom_s1", "teddy_s4"])
def test_host_candidates_on_9_mib_across_chunk_and_vector_borders(name):
    """The host twin's worker chunks (host_parallel: the text cut into 2..16 equal parts) and the
    AVX-512 steps' tails (prefilter_cpu.cpp): an occurrence across every 4 KiB border, one ending the
    text, and at every possible chunk border one whose first indexed window starts exactly there (a
    chunk that tested its first byte off the stride would report it twice)."""
    case = _case(name)
    case.check_variant()
    t, ls, data = _big_cpu(name)
    want = golden.literal_candidates(case.lib, data, ls)
    assert sum(want.values()) > 2000
    got = collections.Counter(K.prefilter(t, BIG_N, case.lib.device_tables(CPU)["pf"], ls, 64).tolist())
    _assert_same(got, want, name)


# ------------------------------------------------------------------ GPU: the kernels directly
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_candidates_equal_the_exact_search(gpu_device, name):
    """k_prefilter + k_pf_verify (16 lanes) with cap = 64, so the gram-hit and the candidate buffer
    both re-run: one block looping over the whole text (grid 1: the flush threshold across
    iterations), a ragged grid (3) and the default."""
    case = _case(name)
    case.check_variant()
    pf = case.lib.device_tables(gpu_device)["pf"]
    for i, (label, data, _) in enumerate(case.texts):
        want, _ = case.want(i)
        t = _text(data, gpu_device)
        ls, _ = K.split_lines(t, len(data))
        for grid in (1, 3, 2048):
            got = collections.Counter(K.prefilter(t, len(data), pf, ls, 64, grid).tolist())
            _assert_same(got, want, "%s / %s / grid %d" % (name, label, grid))


# ------------------------------------------------------------------ GPU: the arena path
def _re_events(regexes, data):
    """(line, pattern) of every plain-literal pattern found in a line, with Python's re (bytes: (?i)
    folds ASCII only, as Java does without (?u)); lines as Java's split("\\r?\\n") gives them."""
    lines = re.split(rb"\r?\n", data)
    while lines and not lines[-1]:
        lines.pop()
    pats = [re.compile(r.encode("latin-1")) for r in regexes]
    return [(x, p) for x, line in enumerate(lines) for p, pat in enumerate(pats) if pat.search(line)]


def _arena_text(case):
    """One ASCII text per row: lines and borders of every literal, and enough occurrences (700) to
    overflow an arena that starts from nothing."""
    parts = []
    for lit in case.lib.literals:
        parts += [t for _, t, _ in _line_texts(lit)]
        parts.append(list(_border_texts(lit))[len(lit) // 2][1])
    parts.append(b"\n".join([case.lib.literals[0], _mix(case.lib.literals[-1])] * 350))
    return b"\n".join(parts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_engine_events_equal_python_re_per_line(gpu_device, name):
    """Engine.run (match_and_hits: device-side counts, 16-lane verify, DFA verify of the candidates)
    and Engine.run_document (EarlyPrefilter) on the device: the (line, pattern) events are those of
    Python's re applied to every line. Row teddy_s4 starts from arena rates of 1e-6: the first
    attempt overflows and re-runs."""
    from log_parser_amd.engine import Engine, Segments
    from log_parser_amd.utils.config import Config
    case = _case(name)
    case.check_variant()
    data = _arena_text(case)
    want = _re_events(case.regexes, data)
    assert len(want) > 300
    ids = [p.id for p in case.lib.patterns]
    eng = Engine(case.lib, Config.load(overrides={"engine.device": str(gpu_device)}), device=gpu_device)
    t = _text(data, gpu_device)
    ls, ll = K.split_lines(t, len(data))
    if name == "teddy_s4":
        eng.arena.rate = {k: 1e-6 for k in eng.arena.rate}
    res = eng.run(t, len(data), ls, ll, Segments.single(ls.numel(), gpu_device), eng.freq_carry())
    if name == "teddy_s4":
        assert eng.arena.last["gram_hits"] > 512 + 1 and eng.arena.rate["gram"] > 1e-4      # it did overflow
    doc = eng.run_document(t, len(data), record=False)
    for r in (res, doc):
        got = [(int(x), int(ids[int(p)][1:])) for x, p in zip(r.ev_line.cpu(), r.ev_pat.cpu())]
        assert sorted(got) == want


# ------------------------------------------------------------------ GPU: the bulk variants
BULK_N = (64 << 20) + 53                     # the smallest size that selects PF_UNROLL = 4 and PV_LANES < 16
BULK_CASES = sorted(ROWS) + ["crowded10", "fanout"]
BULK_ALL_LANES = ("bloom_s4", "teddy_s4", "crowded10", "fanout")   # every PV_LANES; the other rows: the default
BULK_FIRST, BULK_LAST = LONG[0], LONG[1]     # literals of bloom_s4, teddy_s4 and crowded10 alike


@pytest.fixture(scope="module")
def bulk(gpu_device):
    """One 64 MiB text for every row, uploaded once: occurrences across every 4 KiB border (so across
    every 16 KiB border and every unrolled block span, 512 x 4 x 16 and 1024 x 4 x 16 bytes); at byte
    0 and ending on the last byte (nbytes % 16 = 5: a ragged last unit) two literals that bloom_s4,
    teddy_s4 and crowded10 share; a 64 KiB stretch with two literals every 16 bytes (more than 1024
    gram hits per k_prefilter block iteration) and 16 KiB of the literal that 40 regexes share (more
    than 1024 candidates per k_pf_verify block iteration)."""
    lits = sorted(set(l for r in BULK_CASES for l in _case(r).lib.literals))
    a = _sparse_text(BULK_N, lits, 11, first=BULK_FIRST, last=BULK_LAST,
                     dense=[(40 << 20, b"segfault at qx7 ", 65536), (48 << 20, FAN_DENSE, 16384)])
    t = torch.zeros(K.padded_len(BULK_N), dtype=torch.uint8)
    t[:BULK_N] = torch.from_numpy(a)
    td = t.to(gpu_device)
    ls, _ = K.split_lines(td, BULK_N)
    return dict(text=td, ls=ls, ls_host=ls.cpu(), data=a.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("name", BULK_CASES)
def test_bulk_variants_equal_the_exact_search(gpu_device, bulk, name):
    """k_prefilter<.., PF_UNROLL = 4> and k_pf_verify<16 / 4 / 2 / 1> (nbytes >= 64 MiB) against the
    exact search, the oracle computed once per row."""
    case = _case(name)
    case.check_variant()
    want = golden.literal_candidates(case.lib, bulk["data"], bulk["ls_host"])
    assert sum(want.values()) > 2000
    if name in BULK_ALL_LANES[:3]:           # the text's first and last bytes belong to this row's literals
        pfn, last_line = case.lib.pf, bulk["ls_host"].numel() - 1
        for lit, line in ((BULK_FIRST, 0), (BULK_LAST, last_line)):
            r = int(pfn["lit_reg"][int(pfn["lit_reg_off"][case.lib.literals.index(lit)])])
            assert want[(r << 32) | line] == 1, (name, lit, line)
        assert bulk["data"].lower().startswith(BULK_FIRST) and bulk["data"].lower().endswith(BULK_LAST)
    pf = case.lib.device_tables(gpu_device)["pf"]
    try:
        for lanes in (16, 4, 2, 1) if name in BULK_ALL_LANES else (4,):
            N.set_pf_verify_lanes(lanes)
            got = collections.Counter(K.prefilter(bulk["text"], BULK_N, pf, bulk["ls"], 64).tolist())
            _assert_same(got, want, "%s / %d lanes" % (name, lanes))
    finally:
        N.set_pf_verify_lanes(4)
