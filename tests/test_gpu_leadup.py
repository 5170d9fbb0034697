"""GPU: the lead-up kernel (csrc/kernels/leadup.hip k_lead_sig: sign every line, mark the lines
before an event, compact them) against its host twin, and the whole report GPU engine == CPU
engine == golden.leadup for a document, a stream in small chunks and a resident log."""
import random

import numpy as np
import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, templated_log

pytestmark = pytest.mark.gpu

CRAFTED = [0, 1, 15, 16, 17, 1023, 1024, 1025, 5000]


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


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


def _event_sets(L: int, rng):
    """name -> sorted distinct event lines below L (a set that is empty at this L only once)."""
    sets = {"empty": [], "first": [0], "last": [L - 1], "255..257": [e for e in (255, 256, 257) if e < L],
            "every": list(range(L)), "1%": sorted(rng.sample(range(L), max(1, L // 100)))}
    return {k: v for k, v in sets.items() if v or k == "empty"}


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049, 4097])
def test_lead_kernel_matches_twin(gpu_device, L):
    rng = random.Random(L)
    lines = _lines(L, seed=L)
    sigs = [_signed(golden.line_signature(x)) for x in lines]
    x = np.arange(L, dtype=np.int64)
    for shift in (0, 1, 15):
        cpu = _index(lines, shift)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        assert gpu[0].numel() == cpu[0].numel() and gpu[0].data_ptr() % 16 == 0 and int(gpu[1][0]) % 16 == shift
        for name, events in _event_sets(L, rng).items():
            ev = torch.tensor(events, dtype=torch.int32)
            dev_ev = ev.to(gpu_device) if events else None        # (no events: a null pointer on the GPU, an empty list on the CPU)
            for W in (1, 50, 4096):
                ws, wlead, wl, wp, wn = K.lead_lines(*cpu, ev, W, cap=L)
                # the twin is tied to the oracle on the CPU: signatures, and the predicate by a search of its own
                e = np.asarray(events, dtype=np.int64)
                j = np.searchsorted(e, x + 1)
                want = (j < e.size) & (e[np.minimum(j, max(e.size - 1, 0))] <= x + W) if e.size else np.zeros(L, bool)
                assert ws.tolist() == sigs and wlead.tolist() == want.astype(int).tolist() and wn == int(want.sum())
                assert wl.tolist() == np.nonzero(want)[0].tolist() and wp.tolist() == [sigs[i] for i in wl.tolist()]
                for per_block in (0, 256, 2048):
                    for cap in (None, 0, wn, wn - 1):
                        if cap is not None and cap < 0:
                            continue
                        gs, glead, gl, gp, gn = K.lead_lines(*gpu, dev_ev, W, cap=cap, per_block=per_block)
                        what = (shift, name, W, per_block, cap)
                        assert gs.dtype == torch.int64 and glead.dtype == torch.uint8 and gl.dtype == torch.int32, what
                        assert gp.dtype == torch.int64 and gs.is_cuda and gn == wn == gl.numel() == gp.numel(), what
                        assert torch.equal(gs.cpu(), ws) and torch.equal(glead.cpu(), wlead), what
                        gl, o = torch.sort(gl.cpu())              # (the GPU's order is unspecified)
                        assert torch.equal(gl, wl) and torch.equal(gp.cpu()[o], wp), what


def test_no_lines_launch_nothing(gpu_device):
    text = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    none = torch.empty(0, dtype=torch.int64, device=gpu_device), torch.empty(0, dtype=torch.int32, device=gpu_device)
    sig, lead, line, psig, n = K.lead_lines(text, *none, None, 50)
    assert (sig.numel(), lead.numel(), line.numel(), psig.numel(), n) == (0, 0, 0, 0, 0) and sig.is_cuda
    with pytest.raises(ValueError):
        K.lead_lines(text, *none, torch.zeros(1, dtype=torch.int32), 50)          # events on another device


# ---- the reports

def _library():
    return [PatternSet.model_validate({"metadata": {"library_id": "leadup"}, "patterns": [
        {"id": "oom", "name": "oom", "severity": "CRITICAL",
         "primary_pattern": {"regex": r"OutOfMemoryError", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "dup", "name": "backref", "severity": "LOW",
         "primary_pattern": {"regex": r"(\w+)Dup \1", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


@pytest.fixture(scope="module")
def report_case():
    """20 templates plus two planted shapes that are events (one a backreference match on the host
    side path); 400 lines with some CRLF line ends, so that chunks of 64 bytes hold one line each;
    the CPU parser and its report with every group -- shared by the tests below."""
    temps = log_templates(20, seed=5) + ["%02d:%02d:%03d java.lang.OutOfMemoryError: Java heap space %d",
                                         "%02d:%02d:%03d ERROR fooDup foo happened %d times"]
    log = templated_log(400, temps, seed=7, crlf_rate=0.1)
    cpu = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    want = cpu.leadup(log, window=12, top=None, min_count=1)
    assert want == golden.leadup(log, _library(), cpu.config.scoring, 12, None, "share", 1)
    assert want["eventLines"] > 3 and 24 < want["leadLines"] < 300 and want["templates"] > 5
    assert any(g["count"] < g["total"] for g in want["top"])
    return log, cpu, want


@pytest.fixture(scope="module")
def gpu_parser(gpu_device):
    return LogParser(_library(), config=Config.load(overrides={"engine.device": str(gpu_device)}))


def test_report_gpu_equals_cpu_and_golden(gpu_device, gpu_parser, report_case):
    log, cpu, want = report_case
    data = log.encode()
    kw = {"window": 12, "top": None, "min_count": 1}
    before = gpu_parser.frequency_statistics()
    assert gpu_parser.leadup(log, **kw) == want                                              # a document
    for c in (64, 4096):
        assert gpu_parser.leadup_stream(data, chunk_bytes=c, **kw) == want, c                # one-line chunks; ~40-line chunks
    res = gpu_parser.load_resident(data, chunk_bytes=8192)
    assert len(res.chunks) > 3 and gpu_parser.leadup_resident(res, **kw) == want             # a resident log
    for order in ("share", "count", "first"):
        kw = {"window": 50, "top": 5, "order": order, "min_count": 2}
        got = gpu_parser.leadup(log, **kw)
        assert got == cpu.leadup(log, **kw) == golden.leadup(log, _library(), cpu.config.scoring, 50, 5, order, 2)
        assert got == gpu_parser.leadup_stream(data, chunk_bytes=4096, **kw)
    assert gpu_parser.frequency_statistics() == before
