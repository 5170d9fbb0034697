"""GPU: the spans text kernel (csrc/kernels/spans.hip k_span_keys: stamp, template signature and the
sampled keys of every line with the places of their tokens, 0..8 compacted triples per line)
against its host twin, the twin against ``golden``, ``sig`` / ``ts`` against ``K.line_stamps``,
and the whole report GPU engine == CPU engine == golden.spans for a document, a stream, a resident
log and an accumulator fed in two parts, at ``max_ids`` 16 and at the default."""
import random
from collections import Counter

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.native import N
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import SPAN_HOST, span_log
from spans_cases import SPAN_HAND, sorted_triples, want_span_keys
from values_cases import index, random_lines

pytestmark = pytest.mark.gpu

CANARY_LINE, CANARY_KEY = -77, 0x5A5A5A5A5A5A5A5A


def _lines(L: int, seed: int):
    """``L`` lines: random ones (values_cases.random_lines) and, from 63 lines on, this report's
    hand-written lines at fixed places, the first and the last line included (the one that ends
    in CR left out: the splitter takes CR LF as the line end)."""
    lines = random_lines(L - 1, seed)
    special = [x for x in SPAN_HAND if not x.endswith(b"\r") and x]
    if L >= 63:
        rng = random.Random(seed)
        at = [0, L - 1] + rng.sample(range(1, L - 1), len(special) - 2)
        for i, s in zip(at, special):
            lines[i] = s
    return lines


def _raw(idx, shift: int, cap: int, room: int, per_block: int):
    """One launch, no re-run: triple buffers of ``room`` >= cap entries filled with canaries."""
    text, ls, ll = idx
    dev = text.device
    sig = torch.full((ls.numel(),), CANARY_KEY, dtype=torch.int64, device=dev)
    ts = torch.full((ls.numel(),), CANARY_KEY, dtype=torch.int64, device=dev)
    out_line = torch.full((room,), CANARY_LINE, dtype=torch.int32, device=dev)
    out_key = torch.full((room,), CANARY_KEY, dtype=torch.int64, device=dev)
    out_tok = torch.full((room,), CANARY_LINE, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    lvl = torch.zeros(K.SPAN_LEVELS, dtype=torch.int64, device=dev)
    N.span_keys(text.data_ptr(), text.numel(), ls.data_ptr(), ll.data_ptr(), ls.numel(), 8, shift, sig.data_ptr(), ts.data_ptr(),
                out_line.data_ptr(), out_key.data_ptr(), out_tok.data_ptr(), cap, cnt.data_ptr(), lvl.data_ptr(), K._s(text),
                text.is_cuda, per_block)
    return sig.cpu(), ts.cpu(), out_line.cpu(), out_key.cpu(), out_tok.cpu(), cnt.tolist(), lvl.tolist()


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_kernel_matches_twin(gpu_device, L):
    lines = _lines(L, seed=L)
    wants = {shift: want_span_keys(lines, 8, shift) for shift in (0, 1, 3)}     # the specification, once per sample
    for shift_bytes in (0, 1, 15):
        cpu = index(lines, shift_bytes)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        assert gpu[0].numel() == cpu[0].numel() and gpu[0].data_ptr() % 16 == 0 and int(gpu[1][0]) % 16 == shift_bytes
        lsig, lts = K.line_stamps(*gpu)
        for shift in (0, 1, 3):
            sigs, stamps, triples, held, levels = wants[shift]
            wsig, wts, wl, wk, wt, (wn, wheld) = K.span_keys(*cpu, shift=shift)
            want = sorted_triples(wl, wk, wt)
            # the twin is tied to the specification on the CPU
            assert want == sorted(triples) and wsig.tolist() == sigs and wts.tolist() == stamps and (wn, wheld) == (len(want), held)
            for per_block in (256, 2048):
                for cap in (None, 0, max(wn - 1, 0), wn, wn + 7):
                    what = (shift_bytes, shift, per_block, cap)
                    got_levels = torch.zeros(K.SPAN_LEVELS, dtype=torch.int64, device=gpu_device)
                    gsig, gts, gl, gk, gt, (gn, gheld) = K.span_keys(*gpu, shift=shift, cap=cap, per_block=per_block,
                                                                     levels=got_levels)
                    assert (gsig.dtype, gts.dtype, gl.dtype, gk.dtype, gt.dtype) == \
                        (torch.int64, torch.int64, torch.int32, torch.int64, torch.int32), what
                    assert gl.is_cuda and (gn, gheld) == (wn, wheld) and gl.numel() == gk.numel() == gt.numel() == wn, what
                    assert torch.equal(gsig.cpu(), wsig) and torch.equal(gts.cpu(), wts), what
                    assert torch.equal(gsig, lsig) and torch.equal(gts, lts), what     # what k_line_stamps computes
                    assert sorted_triples(gl, gk, gt) == want and got_levels.tolist() == levels, what
                    if cap is None:
                        continue
                    # one launch with that capacity: the counters are exact, the first min(cap, n) slots
                    # hold that many of the triples, and nothing is written past `cap`
                    rsig, rts, rl, rk, rt, rcnt, rlvl = _raw(gpu, shift, cap, wn + 64, per_block)
                    assert rcnt == [wn, wheld] and rlvl == levels and torch.equal(rsig, wsig) and torch.equal(rts, wts), what
                    m = min(max(cap, 0), wn)
                    assert (rl[m:] == CANARY_LINE).all() and (rk[m:] == CANARY_KEY).all() and (rt[m:] == CANARY_LINE).all(), what
                    head = sorted_triples(rl[:m], rk[:m], rt[:m])
                    assert len(head) == m and not Counter(head) - Counter(want) and (cap < wn or head == want), what


def test_full_and_empty_rounds(gpu_device):
    """Rounds at the bounds of the LDS stage: every one of 256 lanes emits 8 triples (2,048, the
    stage exactly full), and rounds in which no lane emits any -- alone, and next to a full one."""
    full = [b" ".join(b"key%05dx%d" % (i, k) for k in range(9)) for i in range(600)]        # nine ids: the ninth is ignored
    none = [b"INFO nothing to see here, line after line" for i in range(600)]
    cases = {"full": full[:256], "none": none[:256], "full, none, full": full[:256] + none[:256] + full[256:512],
             "none, full, ragged": none[:256] + full[:256] + full[256:300], "alternating": [x for p in zip(full, none) for x in p][:700]}
    for name, lines in cases.items():
        cpu = index(lines, 1)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        want = K.span_keys(*cpu)
        n_full = sum(1 for x in lines if x[:1] != b"I")
        assert want[5] == (8 * n_full, n_full)
        for per_block in (0, 256, 512, 2048):
            got = K.span_keys(*gpu, per_block=per_block)
            assert got[5] == want[5] and torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (name, per_block)
            assert sorted_triples(*got[2:5]) == sorted_triples(*want[2:5]), (name, per_block)


def test_no_lines_and_misaligned_text(gpu_device):
    text = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    none = torch.empty(0, dtype=torch.int64, device=gpu_device), torch.empty(0, dtype=torch.int32, device=gpu_device)
    out = K.span_keys(text, *none)
    assert [t.numel() for t in out[:5]] == [0] * 5 and out[5] == (0, 0) and out[2].is_cuda
    ls, ll = torch.zeros(1, dtype=torch.int64, device=gpu_device), torch.full((1,), 8, dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError):
        K.span_keys(text, ls, ll, per_block=4096)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        K.span_keys(text[1:], ls, ll)


# ---- the reports

EVERY = {"top": None, "kinds": None, "min_lines": 1, "max_share": 1.0}


@pytest.fixture(scope="module")
def report_case():
    """The 4,000-line span log behind an unstamped prefix with some CR LF line ends; the CPU parser
    and its reports with every span listed at ``max_ids`` 16 and at the default -- shared by the
    tests below."""
    log, facts = span_log(4000, seed=2, crlf_rate=0.05)
    log = "starting up on %s\n" % SPAN_HOST + log
    cpu = LogParser([], config=Config.load(overrides={"engine.device": "cpu"}))
    want = {m: cpu.spans(log, max_ids=m, **EVERY) for m in (16, 1 << 22)}
    for m in (16, 1 << 22):
        assert want[m] == golden.spans(log, max_ids=m, **EVERY) and want[m]["totalLines"] == 4001
    assert want[16]["sampleShift"] > 0 == want[1 << 22]["sampleShift"] and 4 <= want[16]["ids"] <= 16
    top = cpu.spans(log)
    assert top["top"][0]["key"] == facts["long"] and top["kinds"][0]["unfinished"] == 1
    return log, cpu, want, facts


@pytest.fixture(scope="module")
def gpu_parser(gpu_device):
    return LogParser([], config=Config.load(overrides={"engine.device": str(gpu_device)}))


@pytest.mark.parametrize("max_ids", [16, 1 << 22])
def test_report_gpu_equals_cpu_and_golden(gpu_device, gpu_parser, report_case, max_ids):
    log, cpu, wants, facts = report_case
    want, data = wants[max_ids], log.encode()
    kw = dict(EVERY, max_ids=max_ids)
    before = gpu_parser.frequency_statistics()
    assert gpu_parser.spans(log, **kw) == want                                                # a document
    for c in (4096, 1 << 20):
        assert gpu_parser.spans_stream(data, chunk_bytes=c, **kw) == want, c                  # ~40-line chunks; one chunk
    head = "".join(log.splitlines(keepends=True)[:150])                                       # one-line chunks
    assert gpu_parser.spans_stream(head.encode(), chunk_bytes=64, **kw) == cpu.spans(head, **kw) == golden.spans(head, **kw)
    res = gpu_parser.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3 and gpu_parser.spans_resident(res, **kw) == want               # a resident log
    acc = gpu_parser.span_accumulator(max_ids=max_ids)                                        # one log in two parts
    acc.add_document(data[:data.index(b"\n", len(data) // 2) + 1])
    acc.add_stream(data[data.index(b"\n", len(data) // 2) + 1:], 50000)
    assert acc.report(**EVERY) == want
    assert acc.table.used == want["ids"] and acc.shift == want["sampleShift"]
    for order in ("duration", "lines", "first"):
        for unfinished_only in (False, True):
            kw = {"top": 5, "order": order, "min_ms": 20, "max_ids": max_ids, "unfinished_only": unfinished_only, "kinds": 2}
            got = gpu_parser.spans(log, **kw)
            assert got == cpu.spans(log, **kw) == golden.spans(log, **kw)
            assert got == gpu_parser.spans_stream(data, chunk_bytes=65536, **kw) == gpu_parser.spans_resident(res, **kw)
            assert len(got["top"]) <= 5
    if max_ids > 16:
        assert gpu_parser.spans(log)["top"][0]["key"] == facts["long"]
        assert [r["key"] for r in gpu_parser.spans(log, unfinished_only=True)["top"]] == [facts["unfinished"]]
    assert gpu_parser.frequency_statistics() == before
