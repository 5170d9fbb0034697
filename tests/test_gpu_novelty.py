"""GPU: the novelty kernel (csrc/kernels/novelty.hip k_novel_sig: sign, probe, compact in one pass)
and k_gap_contains against their host twins, and the whole report GPU engine == CPU engine ==
golden.novelty for a document, a stream in small chunks and a resident log."""
import random

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd import novelty as NV
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, templated_log

pytestmark = pytest.mark.gpu

CRAFTED = [0, 1, 15, 16, 17, 1023, 1024, 1025, 5000]
_M64 = (1 << 64) - 1


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


def _gt_hash(sig: int) -> int:
    """csrc/kernels/gap_table.h gt_hash."""
    h = sig & _M64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & _M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & _M64
    return h ^ (h >> 33)


def _lines(L: int, seed: int):
    """``L`` lines of a dozen templates with varying numbers; from 63 lines on, the crafted
    lengths, blank runs, bytes >= 0x80, digit tokens at the end and a pair that differs only past
    byte 1024 are among them (at fixed places, the last line included)."""
    rng = random.Random(seed)
    temps = [b"INFO unit %d of %d served", b"ERROR unit %d failed: code=%d", b"WARN \t slow  disk sd%d %dms",
             b"DEBUG h\xc3\xa9artbeat %d from node-%d", b"%d %d", b"trace %d id=%d"] + \
            [b"INFO template number %s says %%d and %%d" % w for w in (b"one", b"two", b"three", b"four", b"five", b"six")]
    lines = [rng.choice(temps) % (rng.randrange(10000), rng.randrange(10000)) for _ in range(L)]
    if L >= 63:
        special = [bytes(rng.choice(b"ab1 9\tZ-.:") for _ in range(n)) for n in CRAFTED]
        special += [b"a \t\t  b\t \tc", b"a b c", b"caf\xc3\xa9 \xff\xfe 42 \x80\x80abc1\x80", bytes(range(128, 256)) * 3,
                    b"retry in 30", b"retry in 7", b"x" * 1020 + b" tail AAAA", b"x" * 1020 + b" tail BBBB"]
        at = [0, L - 1] + rng.sample(range(1, L - 1), len(special) - 2)
        for i, s in zip(at, special):
            lines[i] = s
    return lines


def _index(lines, shift: int):
    """(text, ls, ll) on the CPU: the first line starts at byte ``shift`` (mod 16) of the text and
    the last line ends with the text's last byte -- no line end and NO padding after it."""
    lead = b"" if shift == 0 else b"p" * (shift - 1) + b"\n"
    data = lead + b"\n".join(lines)
    padded = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    padded[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    ls, ll = K.split_chunk_lines(padded, len(data))
    if shift:
        ls, ll = ls[1:].contiguous(), ll[1:].contiguous()
    assert ls.numel() == len(lines) and int(ls[0]) == shift and int(ls[-1]) + int(ll[-1]) == len(data)
    return padded[:len(data)].clone(), ls, ll


def _tables(sig: torch.Tensor, cap, dev):
    """The same table on the CPU and on the GPU."""
    return K.GapTable.from_signatures("cpu", sig, cap=cap), K.GapTable.from_signatures(dev, sig, cap=cap)


def _compare(cpu, gpu, tabs, feat, evm, cap, per_block, name):
    (text, ls, ll), (dtext, dls, dll) = cpu, gpu
    dev = dtext.device
    wl, ws, wf, wc = K.novel_lines(text, ls, ll, tabs[0], feat, evm, cap=cap)
    gl, gs, gf, gc = K.novel_lines(dtext, dls, dll, tabs[1], None if feat is None else feat.to(dev),
                                   None if evm is None else evm.to(dev), cap=cap, per_block=per_block)
    assert gc == wc and gl.numel() == wl.numel() == wc[1], name
    assert gl.dtype == torch.int32 and gs.dtype == torch.int64 and gf.dtype == torch.uint8
    gl, o = torch.sort(gl.cpu())                                  # (the GPU's order is unspecified)
    assert torch.equal(gl, wl) and torch.equal(gs.cpu()[o], ws) and torch.equal(gf.cpu()[o], wf), name
    return wc


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049, 4097])
def test_novel_kernel_matches_twin(gpu_device, L):
    rng = random.Random(L)
    lines = _lines(L, seed=L)
    cpu = _index(lines, shift=L % 16)
    gpu = tuple(t.to(gpu_device) for t in cpu)
    assert gpu[0].numel() == cpu[0].numel() and gpu[0].data_ptr() % 16 == 0
    sigs = [_signed(golden.line_signature(x)) for x in lines]
    assert K.line_signatures(*cpu).tolist() == sigs              # (the twin is tied to the oracle on the CPU)
    distinct = sorted(set(sigs))
    feat = torch.tensor([rng.choice((0, 1, 2, 4, 5, 8, 9, 12)) for _ in range(L)], dtype=torch.uint8)
    evm = torch.tensor([rng.random() < 0.2 for _ in range(L)], dtype=torch.uint8)
    n_cand = sum((f & 9) != 0 and (f & 4) == 0 for f in feat.tolist())
    # the baselines. all: nothing is novel; most: the lines of a few signatures are (a few percent
    # for the large L: the templates repeat, the crafted lines do not); none: an empty table, every
    # line comes out; half: exactly half full with fillers that are no line's signature; two: a
    # FULL table of two slots whose keys share their home slot, so one of them sits past the wrap
    rare = set(rng.sample(distinct, max(1, len(distinct) // 8)))
    most = [s for s in distinct if s not in rare]
    fill = [s for s in (rng.randrange(-(1 << 63), 1 << 63) for _ in range(4096)) if s not in set(distinct)]
    half = (most + fill)[:2048]
    home = {}
    for s in distinct + fill:
        home.setdefault(_gt_hash(s) & 1, []).append(s)
    two = home[1][:2]
    assert len(two) == 2
    bases = {"all": (distinct, None), "most": (most, None), "none": ([], None), "half": (half, 4096), "two": (two, 2)}
    for name, (held, tcap) in bases.items():
        tabs = _tables(torch.tensor(held, dtype=torch.int64), tcap, gpu_device)
        assert tabs[1].cap == tabs[0].cap == (tcap or 4096) and tabs[1].used == len(held)
        want_novel = sum(s not in set(held) for s in sigs)
        for f, e in ((feat, evm), (None, None), (feat, None), (None, evm)):
            for per_block in (0, K.NV_MAX_LINES):
                cnt = _compare(cpu, gpu, tabs, f, e, None, per_block, (name, per_block))
                assert cnt[:2] == (n_cand if f is not None else 0, want_novel)
        if name in ("most", "none"):
            _compare(cpu, gpu, tabs, feat, evm, 1, 0, (name, "cap=1"))                    # the capacity re-run
            _compare(cpu, gpu, tabs, feat, evm, max(1, want_novel - 1), 256, (name, "one short"))
        if name == "all":
            assert want_novel == 0
        if name == "none":
            assert want_novel == L


def test_first_line_at_every_alignment(gpu_device):
    lines = _lines(65, seed=7)
    sigs = sorted({_signed(golden.line_signature(x)) for x in lines})
    tabs = _tables(torch.tensor(sigs[::2], dtype=torch.int64), None, gpu_device)
    feat = torch.tensor([9, 0, 4] * 22, dtype=torch.uint8)[:65].contiguous()
    for shift in range(16):
        cpu = _index(lines, shift)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        assert int(gpu[1][0]) % 16 == shift and gpu[0].data_ptr() % 16 == 0
        cnt = _compare(cpu, gpu, tabs, feat, None, None, 0, shift)
        assert 0 < cnt[1] < 65


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_contains_matches_twin(gpu_device, n):
    rng = random.Random(n)
    E = K.GT_EMPTY
    keys = [rng.randrange(-(1 << 63), 1 << 63) for _ in range(1500)]
    ask = [rng.choice(keys) if rng.random() < 0.5 else rng.randrange(-(1 << 63), 1 << 63) for _ in range(n)]
    ask[0] = E
    ask[-1] = E if n > 1 else ask[-1]
    for with_marker in (False, True):
        held = torch.tensor(keys + ([E] if with_marker else []), dtype=torch.int64)
        for cap in (None, 2048):                                  # at most half full; 73 % full: long probe chains
            cpu, gpu = _tables(held, cap, gpu_device)
            want = cpu.contains(torch.tensor(ask, dtype=torch.int64))
            got = gpu.contains(torch.tensor(ask, dtype=torch.int64, device=gpu_device))
            assert got.dtype == torch.bool and got.is_cuda and torch.equal(got.cpu(), want)
            assert want.tolist() == [a in set(held.tolist()) for a in ask]
            assert bool(want[0]) == with_marker
    assert gpu.contains(torch.empty(0, dtype=torch.int64, device=gpu_device)).numel() == 0


# ---- the reports

def _library():
    return [PatternSet.model_validate({"metadata": {"library_id": "novelty"}, "patterns": [
        {"id": "oom", "name": "oom", "severity": "CRITICAL",
         "primary_pattern": {"regex": r"OutOfMemoryError", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "flush", "name": "flush", "severity": "HIGH",
         "primary_pattern": {"regex": r"checkpoint .*flush|flush .*checkpoint", "confidence": 0.8}},
        {"id": "dup", "name": "backref", "severity": "LOW",
         "primary_pattern": {"regex": r"(\w+)Dup \1", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


@pytest.fixture(scope="module")
def report_case():
    """40 templates, 10 of them held out of the healthy log, plus three planted shapes (an event
    line, a stack frame, a backreference match); 4000 failing lines with some CRLF line ends; the
    CPU parser, its baseline and its report with every group -- shared by the tests below."""
    temps = log_templates(40, seed=5)
    healthy = templated_log(3000, temps[::4] + temps[1::4] + temps[2::4], seed=6, crlf_rate=0.05)
    log = templated_log(4000, temps + ["%02d:%02d:%03d java.lang.OutOfMemoryError: Java heap space %d",
                                       "%02d%02d%03d\tat com.acme.Pool.grow(Pool.java:%d)",
                                       "%02d:%02d:%03d ERROR fooDup foo happened %d times"], seed=7, crlf_rate=0.1)
    cpu = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    base = cpu.baseline()
    base.add_document(healthy)
    want = cpu.novelty(log, base, top=None)
    assert want == golden.novelty(log, [healthy], _library(), cpu.config.scoring, None)
    assert want["templates"] >= 10 and want["events"] > 0 and 0 < want["errorTemplates"] < want["templates"]
    assert 0 < want["novelLines"] < want["totalLines"] // 4 and any(g["eventLines"] for g in want["top"])
    return healthy, log, cpu, base, want


@pytest.fixture(scope="module")
def gpu_parser(gpu_device):
    return LogParser(_library(), config=Config.load(overrides={"engine.device": str(gpu_device)}))


def test_baseline_gpu_equals_cpu(gpu_device, gpu_parser, report_case, tmp_path):
    healthy, log, cpu, base, _ = report_case
    a = gpu_parser.baseline()
    a.add_document(healthy)
    b = gpu_parser.baseline()
    b.add_stream(healthy.encode(), chunk_bytes=4096)
    c = gpu_parser.baseline()
    c.add_resident(gpu_parser.load_resident(healthy.encode(), chunk_bytes=8192))
    want = base.signatures().tolist()
    for x in (a, b, c):
        assert x.table.device.type == "cuda" and x.signatures().cpu().tolist() == want
        assert (x.lines, x.documents, x.templates) == (base.lines, 1, base.templates)
    # saved on one device, loaded on the other, then continued
    g, h = str(tmp_path / "gpu.npz"), str(tmp_path / "cpu.npz")
    a.save(g)
    base.save(h)
    on_cpu, on_gpu = cpu.load_baseline(g), gpu_parser.load_baseline(h)
    assert on_cpu.signatures().tolist() == want == on_gpu.signatures().cpu().tolist()
    assert on_gpu.table.device.type == "cuda" and (on_gpu.lines, on_gpu.documents) == (base.lines, 1)
    sigs, n_lines, _ = golden.baseline_signatures([healthy, log])
    for x in (on_cpu, on_gpu):
        x.add_document(log)
        assert (x.lines, x.documents, x.templates) == (n_lines, 2, len(sigs))
        assert x.signatures().cpu().tolist() == sorted(_signed(s) for s in sigs)
    with pytest.raises(ValueError):
        gpu_parser.novelty(log, base)                             # a baseline on another device


def test_report_gpu_equals_cpu_and_golden(gpu_device, gpu_parser, report_case):
    healthy, log, cpu, _, want = report_case
    base = gpu_parser.baseline()
    base.add_document(healthy)
    data = log.encode()
    before = gpu_parser.frequency_statistics()
    assert gpu_parser.novelty(log, base, top=None) == want                                   # a document
    for c in (4096, 1 << 16):
        assert gpu_parser.novelty_stream(data, base, chunk_bytes=c, top=None) == want, c     # a stream in small chunks
    res = gpu_parser.load_resident(data, chunk_bytes=8192)
    assert len(res.chunks) > 3 and gpu_parser.novelty_resident(res, base, top=None) == want  # a resident log
    for order in ("count", "first"):
        for errors_only in (False, True):
            kw = {"top": 5, "order": order, "errors_only": errors_only}
            got = gpu_parser.novelty(log, base, **kw)
            assert got == cpu.novelty(log, report_case[3], **kw)
            assert got == gpu_parser.novelty_stream(data, base, chunk_bytes=4096, **kw)
    assert gpu_parser.frequency_statistics() == before
