"""GPU: the value kernel (csrc/kernels/values.hip k_line_vals: template signature of every line and
its numeric fields as compacted (line, key, value) triples, 0..8 per line) against its host twin,
the twin against ``golden.line_values``, and the whole report GPU engine == CPU engine ==
golden.values for a document, a stream in small chunks and a resident log."""
import random
from collections import Counter

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.native import N
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, metric_log
from values_cases import HAND, index, random_lines

pytestmark = pytest.mark.gpu

CANARY_LINE, CANARY_KEY, CANARY_VAL = -77, 0x5A5A5A5A5A5A5A5A, -99


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


def _lines(L: int, seed: int):
    """``L`` lines: random ones (values_cases.random_lines) and, from 63 lines on, the hand-written
    lines at fixed places, the first and the last line included."""
    lines = random_lines(L - 1, seed)
    if L >= 63:
        rng = random.Random(seed)
        special = [x for x, _ in HAND]
        at = [0, L - 1] + rng.sample(range(1, L - 1), len(special) - 2)
        for i, s in zip(at, special):
            lines[i] = s
    return lines


def _raw(idx, cap: int, room: int, per_block: int):
    """One launch, no re-run: triple buffers of ``room`` >= cap entries filled with canaries, the
    signatures, the two counters."""
    text, ls, ll = idx
    dev = text.device
    sig = torch.full((ls.numel(),), CANARY_KEY, dtype=torch.int64, device=dev)
    out_line = torch.full((room,), CANARY_LINE, dtype=torch.int32, device=dev)
    out_key = torch.full((room,), CANARY_KEY, dtype=torch.int64, device=dev)
    out_val = torch.full((room,), CANARY_VAL, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    N.line_vals(text.data_ptr(), text.numel(), ls.data_ptr(), ll.data_ptr(), ls.numel(), sig.data_ptr(), out_line.data_ptr(),
                out_key.data_ptr(), out_val.data_ptr(), cap, cnt.data_ptr(), K._s(text), text.is_cuda, per_block)
    return sig.cpu(), out_line.cpu(), out_key.cpu(), out_val.cpu(), cnt.tolist()


def _sorted_triples(line, key, value):
    return sorted(zip(line.tolist(), key.tolist(), value.tolist()))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_value_kernel_matches_twin(gpu_device, L):
    lines = _lines(L, seed=L)
    sigs = [golden.line_signature(x) for x in lines]
    golden_triples = sorted((i, _signed(golden.val_key(sigs[i], j)), v) for i, x in enumerate(lines)
                            for j, v in golden.line_values(x))
    for shift in (0, 1, 15):
        cpu = index(lines, shift)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        assert gpu[0].numel() == cpu[0].numel() and gpu[0].data_ptr() % 16 == 0 and int(gpu[1][0]) % 16 == shift
        wsig, wl, wk, wv, (wn, wheld) = K.line_values(*cpu)
        want = _sorted_triples(wl, wk, wv)
        # the twin is tied to the specification on the CPU
        assert want == golden_triples and wsig.tolist() == [_signed(s) for s in sigs]
        assert wn == len(want) and wheld == sum(1 for x in lines if golden.line_values(x)) and 0 < wn
        for per_block in (256, 2048):
            for cap in (None, 0, wn - 1, wn, wn + 7):
                what = (shift, per_block, cap)
                gsig, gl, gk, gv, (gn, gheld) = K.line_values(*gpu, cap=cap, per_block=per_block)
                assert (gsig.dtype, gl.dtype, gk.dtype, gv.dtype) == (torch.int64, torch.int32, torch.int64, torch.int32), what
                assert gl.is_cuda and (gn, gheld) == (wn, wheld) and gl.numel() == gk.numel() == gv.numel() == wn, what
                assert torch.equal(gsig.cpu(), wsig), what
                assert _sorted_triples(gl, gk, gv) == want, what                  # (the GPU's order is unspecified)
                if cap is None:
                    continue
                # one launch with that capacity: the count is exact, the first min(cap, n) slots hold
                # that many of the triples, and nothing is written past `cap`
                rsig, rl, rk, rv, rcnt = _raw(gpu, cap, wn + 64, per_block)
                assert rcnt == [wn, wheld] and torch.equal(rsig, wsig), what
                assert (rl[cap:] == CANARY_LINE).all() and (rk[cap:] == CANARY_KEY).all() and (rv[cap:] == CANARY_VAL).all(), what
                m = min(cap, wn)
                assert (rl[m:] == CANARY_LINE).all() and (rk[m:] == CANARY_KEY).all() and (rv[m:] == CANARY_VAL).all(), what
                head = _sorted_triples(rl[:m], rk[:m], rv[:m])
                assert len(head) == m and not Counter(head) - Counter(want) and (cap < wn or head == want), what


def test_full_and_empty_rounds(gpu_device):
    """Rounds at the bounds of the LDS stage: every one of 256 lanes emits 8 triples (2048, the
    stage exactly full), and rounds in which no lane emits any -- alone, and next to a full one."""
    full = [b" ".join(b"%dms" % (1000 * i + k) for k in range(9)) for i in range(600)]    # nine fields: the ninth is ignored
    none = [b"INFO nothing to see here x%dy" % i for i in range(600)]                      # a field without a value
    cases = {"full": full[:256], "none": none[:256], "full, none, full": full[:256] + none[:256] + full[256:512],
             "none, full, ragged": none[:256] + full[:256] + full[256:300], "alternating": [x for p in zip(full, none) for x in p][:700]}
    for name, lines in cases.items():
        cpu = index(lines, 1)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        wsig, wl, wk, wv, wcnt = K.line_values(*cpu)
        n_full = sum(1 for x in lines if x[:1] != b"I")
        assert wcnt == (8 * n_full, n_full)
        for per_block in (0, 256, 512, 2048):
            gsig, gl, gk, gv, gcnt = K.line_values(*gpu, per_block=per_block)
            assert gcnt == wcnt and torch.equal(gsig.cpu(), wsig), (name, per_block)
            assert _sorted_triples(gl, gk, gv) == _sorted_triples(wl, wk, wv), (name, per_block)


def test_no_lines_launch_nothing(gpu_device):
    text = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    none = torch.empty(0, dtype=torch.int64, device=gpu_device), torch.empty(0, dtype=torch.int32, device=gpu_device)
    sig, line, key, value, cnt = K.line_values(text, *none)
    assert (sig.numel(), line.numel(), key.numel(), value.numel(), cnt) == (0, 0, 0, 0, (0, 0)) and line.is_cuda
    ls, ll = torch.zeros(1, dtype=torch.int64, device=gpu_device), torch.full((1,), 8, dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError):
        K.line_values(text, ls, ll, per_block=4096)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        K.line_values(text[1:], ls, ll)


# ---- the reports

@pytest.fixture(scope="module")
def report_case():
    """The 4000-line metric log with some CRLF line ends and a few lines that the filters drop; the
    CPU parser and its report with every field -- shared by the tests below."""
    log, burst = metric_log(4000, log_templates(30, 1), seed=2)
    lines = log.split("\n")
    for i in range(7, 4000, 11):
        lines[i] += "\r"
    log = "\n".join(lines) + "retry 5 of 5\n" * 8 + "".join("ptr 0x%x\r\n" % (v << 4 | 0xf) for v in range(16))
    cpu = LogParser([], config=Config.load(overrides={"engine.device": "cpu"}))
    kw = {"top": None, "min_count": 1, "min_fill": 0.0, "varying": False}
    want = cpu.values(log, **kw)
    assert want == golden.values(log, **kw) and want["totalLines"] == 4024 and want["fields"] > 50
    assert "served request in" in cpu.values(log)["top"][0]["example"] and cpu.values(log)["top"][0]["maxLine"] - 1 in burst
    return log, cpu, want


@pytest.fixture(scope="module")
def gpu_parser(gpu_device):
    return LogParser([], config=Config.load(overrides={"engine.device": str(gpu_device)}))


def test_report_gpu_equals_cpu_and_golden(gpu_device, gpu_parser, report_case):
    log, cpu, want = report_case
    data = log.encode()
    kw = {"top": None, "min_count": 1, "min_fill": 0.0, "varying": False}
    before = gpu_parser.frequency_statistics()
    assert gpu_parser.values(log, **kw) == want                                               # a document
    for c in (4096, 1 << 20):
        assert gpu_parser.values_stream(data, chunk_bytes=c, **kw) == want, c                 # ~40-line chunks; one chunk
    head = "".join(log.splitlines(keepends=True)[:150])                                       # one-line chunks
    assert gpu_parser.values_stream(head.encode(), chunk_bytes=64, **kw) == cpu.values(head, **kw)
    res = gpu_parser.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3 and gpu_parser.values_resident(res, **kw) == want              # a resident log
    acc = gpu_parser.value_accumulator()                                                      # one log in two parts
    acc.add_document(data[:data.index(b"\n", len(data) // 2) + 1])
    acc.add_stream(data[data.index(b"\n", len(data) // 2) + 1:], 50000)
    assert acc.report(**kw) == want
    for order in ("peak", "max", "count", "first"):
        kw = {"top": 5, "order": order, "min_count": 9, "min_fill": 0.95}
        got = gpu_parser.values(log, **kw)
        assert got == cpu.values(log, **kw) == golden.values(log, **kw)
        assert got == gpu_parser.values_stream(data, chunk_bytes=65536, **kw) == gpu_parser.values_resident(res, **kw)
        assert len(got["top"]) == 5
    assert gpu_parser.frequency_statistics() == before
