"""GPU: the template-signature kernel (csrc/kernels/gaps.hip k_gap_sig) against its host twin, the
all-lines context features against theirs, and the whole gap report GPU engine == CPU engine ==
golden.gaps."""
import random

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.engine import Engine
from log_parser_amd.models.compiled import CompiledLibrary
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config, ScoringParams
from log_parser_amd.utils.synth import make_library, make_log

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 5000]


def _stage(data: bytes) -> torch.Tensor:
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return text


def _index(data: bytes, dev):
    """(cpu text, ls, ll) and their device copies; the line index comes from the host twin."""
    text = _stage(data)
    ls, ll = K.split_lines(text, len(data))
    return (text, ls, ll), (text.to(dev), ls.to(dev), ll.to(dev))


def _engine(lib, dev):
    return Engine(lib, Config.load(overrides={"engine.device": str(dev)}), device=torch.device(dev))


def test_sig_listed_lines_match_twin(gpu_device):
    rng = random.Random(3)
    lines = []
    for n in LENGTHS:
        lines.append(bytes(rng.choice(b"ab1 9\tZ-.:") for _ in range(n)))
    lines += [b"q" * k for k in range(1, 18)]                     # line starts at every offset mod 16
    lines += [b"." * k + b" tok9en" + b"!" * (16 - k) for k in range(16)]     # tokens across 16-byte load boundaries
    lines.append(b"x" * 1020 + b" abc9defgh tail")              # a token with a digit across byte 1024
    lines.append(b"y" * 1020 + b" abcdefgh9 tail")              # ... whose digit lies past the limit
    lines.append(b"1234567890" * 7)                              # all digits
    lines.append(b"caf\xc3\xa9 \xff\xfe 42 \x80\x80abc1\x80")    # bytes >= 0x80
    lines.append(bytes(range(128, 256)) * 9)
    data = b"\n".join(lines) + b"\n"
    # the text ends with its last line, exactly at a multiple of the line-index tile: the last
    # aligned load of the last line ends where the text's padding begins
    last = b"the last line ends the text 9"
    fill = -(len(data) + 64) % K.NL_TILE + 64
    lines += [b"f" * (fill - len(last) - 1), last]
    data += lines[-2] + b"\n" + last
    assert len(data) % K.NL_TILE == 0
    (text, ls, ll), (dtext, dls, dll) = _index(data, gpu_device)
    assert ls.numel() == len(lines) and int(ls[-1]) + int(ll[-1]) == len(data)
    assert sorted(set((ls % 16).tolist())) == list(range(16))
    want = K.line_signatures(text, ls, ll)
    assert want[0].item() == golden.line_signature(b"") - (1 << 64)          # (the twin is tied to the oracle on the CPU)
    assert torch.equal(K.line_signatures(dtext, dls, dll).cpu(), want)
    L = len(lines)
    for n in (0, 1, 63, 64, 65, 257):
        sel = torch.tensor([rng.randrange(L) for _ in range(n)], dtype=torch.int32)
        if n >= 63:
            sel[-1] = L - 1
        got = K.line_signatures(dtext, dls, dll, sel.to(gpu_device))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want[sel.long()])


@pytest.mark.parametrize("L", [1, 255, 256, 257, 4096, 4097])
def test_sig_self_selecting_matches_twin(gpu_device, L):
    rng = random.Random(L)
    lines = [b"ERROR unit %d of %s failed" % (rng.randrange(1000), rng.choice((b"alpha", b"b2", b"\xc3\xa9"))) for _ in range(L)]
    data = b"\n".join(lines)
    (text, ls, ll), (dtext, dls, dll) = _index(data, gpu_device)
    assert ls.numel() == L
    run = torch.zeros(L, dtype=torch.uint8)
    run[min(250, L - 1):262] = 8                                  # a selected run across the first block boundary
    run[L - 1] = 9
    some = torch.tensor([rng.choice((0, 1, 2, 4, 5, 8, 9, 12)) for _ in range(L)], dtype=torch.uint8)
    cov = torch.tensor([rng.random() < 0.4 for _ in range(L)], dtype=torch.uint8)
    stack = torch.full((L,), 5, dtype=torch.uint8)                # candidates' bits with the stack bit: none selected
    cases = [("all", torch.ones(L, dtype=torch.uint8), None, 1 << 13),
             ("none", stack, None, 16),
             ("none-covered", torch.ones(L, dtype=torch.uint8), torch.ones(L, dtype=torch.uint8), 16),
             ("run", run, torch.zeros(L, dtype=torch.uint8), 64),
             ("mixed", some, cov, 1 << 13),
             ("overflow", some, None, 1)]                         # cap = 1: the capacity re-run
    for name, feat, c, cap in cases:
        wl, ws, wc = K.gap_lines(text, ls, ll, feat, c, cap)
        gl, gs, gc = K.gap_lines(dtext, dls, dll, feat.to(gpu_device), None if c is None else c.to(gpu_device), cap)
        assert gc == wc and gl.numel() == wl.numel(), name
        gl, o = torch.sort(gl.cpu())
        assert torch.equal(gl, wl) and torch.equal(gs.cpu()[o], ws), name
        if name == "all":
            assert wl.numel() == L
        if name.startswith("none"):
            assert wl.numel() == 0 and wc == (0 if name == "none" else L)


@pytest.fixture(scope="module")
def report_case():
    """make_library(64, seed=1), a 20k-line log with CRLF line ends, ~300 spliced lines of 6 fixed
    templates (numbers vary), and the CPU engine's report -- shared by the tests below."""
    sets, trig = make_library(64, seed=1)
    rng = random.Random(21)
    lines = make_log(20000, trig, seed=8, hit_rate=0.02, crlf_rate=0.1).split("\n")
    templates = ["ERROR payment gateway timeout after %dms for order %d",
                 "FATAL replica %d diverged at offset %d",
                 "worker-%d crashed: SegmentationError code=%d",
                 "CRITICAL \t lease %d expired on node-%d",
                 "upstream 10.1.%d.%d returned SocketTimeoutException",
                 "SEVERE héap usage %d%% above limit %d"]
    for k in range(300):
        t = templates[min(5, int(6 * rng.random() ** 2))]        # uneven counts
        at = rng.randrange(len(lines) - 1)
        lines.insert(at, t % (rng.randrange(10000), rng.randrange(10000)) + ("\r" if lines[at].endswith("\r") else ""))
    log = "\n".join(lines)
    lib = CompiledLibrary(sets, ScoringParams())
    return sets, lib, log, _engine(lib, "cpu").gaps_bytes(log.encode("utf-8"), top=None)


def test_context_features_all_match_twin(gpu_device, report_case):
    _, lib, _, _ = report_case
    _, trig = make_library(64, seed=1)
    data = make_log(20000, trig, seed=3, hit_rate=0.02, stack_rate=0.05).encode("utf-8")
    (text, ls, ll), (dtext, dls, dll) = _index(data, gpu_device)
    want = K.context_features_all(text, ls, ll, lib.device_tables(torch.device("cpu"))["dfa"], lib.ctx_dfa_extent)
    got = K.context_features_all(dtext, dls, dll, lib.device_tables(gpu_device)["dfa"], lib.ctx_dfa_extent)
    assert got.dtype == torch.uint8 and got.numel() == ls.numel()
    assert torch.equal(got.cpu(), want)
    assert len(set(want.tolist())) >= 4                           # (errors, warnings, frames, exceptions all occur)


def test_report_gpu_equals_cpu_and_golden(gpu_device, report_case):
    sets, lib, log, cpu = report_case
    eng = _engine(lib, gpu_device)
    before = eng.freq.statistics()
    for cover in ("context", "events"):
        want = cpu if cover == "context" else _engine(lib, "cpu").gaps_bytes(log.encode("utf-8"), top=None, cover=cover)
        assert eng.gaps_bytes(log.encode("utf-8"), top=None, cover=cover) == want
    assert eng.gaps_bytes(log.encode("utf-8"), top=3)["top"] == cpu["top"][:3]
    assert eng.freq.statistics() == before
    assert cpu["templates"] >= 6 and cpu["uncoveredErrorLines"] >= 250
    assert cpu == golden.gaps(log, sets, ScoringParams(), None, "context")
