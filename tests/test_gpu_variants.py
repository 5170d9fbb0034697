"""GPU: the variants kernel (csrc/kernels/variants.hip k_line_vars: template signature of every line
and the token hashes of its fields as compacted (line, field, value) triples, 0..8 per line) against
its host twin, the twin against ``golden.line_fields`` / ``var_hash``, and the whole report GPU
engine == CPU engine == golden.variants for a document, a stream, a resident log and an accumulator
fed in two parts, at D = 4 and D = 64."""
import random
from collections import Counter

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.native import N
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import log_templates, variant_log
from values_cases import HAND, index, random_lines
from variants_cases import VAR_HAND, want_triples

pytestmark = pytest.mark.gpu

CANARY_LINE, CANARY_KEY = -77, 0x5A5A5A5A5A5A5A5A


def _lines(L: int, seed: int):
    """``L`` lines: random ones (values_cases.random_lines) and, from 63 lines on, the hand-written
    lines of both case files at fixed places, the first and the last line included (the ones that
    end in CR left out: the splitter takes CR LF as the line end)."""
    lines = random_lines(L - 1, seed)
    special = [x for x, _ in HAND] + [x for x, _ in VAR_HAND if not x.endswith(b"\r")]
    if L >= 63:
        rng = random.Random(seed)
        special = special[:L - 1]
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
    out_field = torch.full((room,), CANARY_KEY, dtype=torch.int64, device=dev)
    out_value = torch.full((room,), CANARY_KEY, dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    N.line_vars(text.data_ptr(), text.numel(), ls.data_ptr(), ll.data_ptr(), ls.numel(), sig.data_ptr(), out_line.data_ptr(),
                out_field.data_ptr(), out_value.data_ptr(), cap, cnt.data_ptr(), K._s(text), text.is_cuda, per_block)
    return sig.cpu(), out_line.cpu(), out_field.cpu(), out_value.cpu(), cnt.tolist()


def _sorted_triples(line, field, value):
    return sorted(zip(line.tolist(), field.tolist(), value.tolist()))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_kernel_matches_twin(gpu_device, L):
    lines = _lines(L, seed=L)
    sigs, triples, held = want_triples(lines)
    golden_triples = sorted(triples)
    for shift in (0, 1, 15):
        cpu = index(lines, shift)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        assert gpu[0].numel() == cpu[0].numel() and gpu[0].data_ptr() % 16 == 0 and int(gpu[1][0]) % 16 == shift
        wsig, wl, wf, wv, (wn, wheld) = K.line_vars(*cpu)
        want = _sorted_triples(wl, wf, wv)
        # the twin is tied to the specification on the CPU
        assert want == golden_triples and wsig.tolist() == sigs and (wn, wheld) == (len(want), held) and 0 < wn
        for per_block in (256, 2048):
            for cap in (None, 0, wn - 1, wn, wn + 7):
                what = (shift, per_block, cap)
                gsig, gl, gf, gv, (gn, gheld) = K.line_vars(*gpu, cap=cap, per_block=per_block)
                assert (gsig.dtype, gl.dtype, gf.dtype, gv.dtype) == (torch.int64, torch.int32, torch.int64, torch.int64), what
                assert gl.is_cuda and (gn, gheld) == (wn, wheld) and gl.numel() == gf.numel() == gv.numel() == wn, what
                assert torch.equal(gsig.cpu(), wsig), what
                assert _sorted_triples(gl, gf, gv) == want, what                  # (the GPU's order is unspecified)
                if cap is None:
                    continue
                # one launch with that capacity: the count is exact, the first min(cap, n) slots hold
                # that many of the triples, and nothing is written past `cap`
                rsig, rl, rf, rv, rcnt = _raw(gpu, cap, wn + 64, per_block)
                assert rcnt == [wn, wheld] and torch.equal(rsig, wsig), what
                m = min(cap, wn)
                assert (rl[m:] == CANARY_LINE).all() and (rf[m:] == CANARY_KEY).all() and (rv[m:] == CANARY_KEY).all(), what
                head = _sorted_triples(rl[:m], rf[:m], rv[:m])
                assert len(head) == m and not Counter(head) - Counter(want) and (cap < wn or head == want), what


def test_full_and_empty_rounds(gpu_device):
    """Rounds at the bounds of the LDS stage: every one of 256 lanes emits 8 triples (2048, the
    stage exactly full), and rounds in which no lane emits any -- alone, and next to a full one."""
    full = [b" ".join(b"k%dx%d" % (i, k) for k in range(9)) for i in range(600)]           # nine fields: the ninth is ignored
    none = [b"INFO nothing to see here, line after line" for i in range(600)]
    cases = {"full": full[:256], "none": none[:256], "full, none, full": full[:256] + none[:256] + full[256:512],
             "none, full, ragged": none[:256] + full[:256] + full[256:300], "alternating": [x for p in zip(full, none) for x in p][:700]}
    for name, lines in cases.items():
        cpu = index(lines, 1)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        wsig, wl, wf, wv, wcnt = K.line_vars(*cpu)
        n_full = sum(1 for x in lines if x[:1] != b"I")
        assert wcnt == (8 * n_full, n_full)
        for per_block in (0, 256, 512, 2048):
            gsig, gl, gf, gv, gcnt = K.line_vars(*gpu, per_block=per_block)
            assert gcnt == wcnt and torch.equal(gsig.cpu(), wsig), (name, per_block)
            assert _sorted_triples(gl, gf, gv) == _sorted_triples(wl, wf, wv), (name, per_block)


def test_no_lines_and_misaligned_text(gpu_device):
    text = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    none = torch.empty(0, dtype=torch.int64, device=gpu_device), torch.empty(0, dtype=torch.int32, device=gpu_device)
    sig, line, field, value, cnt = K.line_vars(text, *none)
    assert (sig.numel(), line.numel(), field.numel(), value.numel(), cnt) == (0, 0, 0, 0, (0, 0)) and line.is_cuda
    ls, ll = torch.zeros(1, dtype=torch.int64, device=gpu_device), torch.full((1,), 8, dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError):
        K.line_vars(text, ls, ll, per_block=4096)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        K.line_vars(text[1:], ls, ll)


# ---- the reports

EVERY = {"top": None, "min_count": 1, "min_fill": 0.0, "varying": False}


@pytest.fixture(scope="module")
def report_case():
    """The 4000-line variant log with some CRLF line ends and a few lines that the filters drop; the
    CPU parser and its reports with every field at D = 4 and D = 64 -- shared by the tests below."""
    log, facts = variant_log(4000, log_templates(30, 1), seed=2, crlf_rate=0.05)
    log = log + "retry 5 of 5\n" * 8 + "".join("peer 0x%s up\r\n" % ("AB" if v % 3 else "ab") for v in range(16))
    cpu = LogParser([], config=Config.load(overrides={"engine.device": "cpu"}))
    want = {D: cpu.variants(log, max_distinct=D, **EVERY) for D in (4, 64)}
    for D in (4, 64):
        assert want[D] == golden.variants(log, max_distinct=D, **EVERY) and want[D]["totalLines"] == 4024
    assert want[4]["unboundedFields"] > want[64]["unboundedFields"] > 0 and len(want[64]["top"]) > 30
    top = cpu.variants(log)["top"][0]
    assert "upstream returned status" in top["example"] and top["values"][-1]["token"] == facts["rare"]
    assert top["values"][-1]["firstLine"] - 1 == facts["rareLines"][0]
    return log, cpu, want


@pytest.fixture(scope="module")
def gpu_parser(gpu_device):
    return LogParser([], config=Config.load(overrides={"engine.device": str(gpu_device)}))


@pytest.mark.parametrize("D", [4, 64])
def test_report_gpu_equals_cpu_and_golden(gpu_device, gpu_parser, report_case, D):
    log, cpu, wants = report_case
    want, data = wants[D], log.encode()
    kw = dict(EVERY, max_distinct=D)
    before = gpu_parser.frequency_statistics()
    assert gpu_parser.variants(log, **kw) == want                                             # a document
    for c in (4096, 1 << 20):
        assert gpu_parser.variants_stream(data, chunk_bytes=c, **kw) == want, c               # ~40-line chunks; one chunk
    head = "".join(log.splitlines(keepends=True)[:150])                                       # one-line chunks
    assert gpu_parser.variants_stream(head.encode(), chunk_bytes=64, **kw) == cpu.variants(head, **kw) == \
        golden.variants(head, **kw)
    res = gpu_parser.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3 and gpu_parser.variants_resident(res, **kw) == want            # a resident log
    acc = gpu_parser.variant_accumulator(D)                                                   # one log in two parts
    acc.add_document(data[:data.index(b"\n", len(data) // 2) + 1])
    acc.add_stream(data[data.index(b"\n", len(data) // 2) + 1:], 50000)
    assert acc.report(**EVERY) == want
    assert acc.table.used == sum(r["distinct"] for r in want["top"]) and len(acc.unbounded) == want["unboundedFields"]
    for order in ("odd", "count", "distinct", "first"):
        kw = {"top": 5, "order": order, "min_count": 9, "min_fill": 0.95, "max_distinct": D, "show": 2}
        got = gpu_parser.variants(log, **kw)
        assert got == cpu.variants(log, **kw) == golden.variants(log, **kw)
        assert got == gpu_parser.variants_stream(data, chunk_bytes=65536, **kw) == gpu_parser.variants_resident(res, **kw)
        assert 1 <= len(got["top"]) <= 5
    assert gpu_parser.frequency_statistics() == before
