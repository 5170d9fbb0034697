"""GPU: the key kernel (csrc/kernels/correlate.hip k_line_keys: the keys of lines as compacted (line,
key) pairs, 0..8 per line, optionally of a list of lines and filtered by a device table) against
its host twin, and the whole report GPU engine == CPU engine == golden.correlate for a document, a
stream in small chunks and a resident log."""
import random
from collections import Counter

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.models.schema import PatternSet
from log_parser_amd.native import N
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import correlated_log, log_templates

pytestmark = pytest.mark.gpu

H = golden.fnv1a64
CANARY_LINE, CANARY_KEY = -77, 0x5A5A5A5A5A5A5A5A


def _signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


def _lines(L: int, seed: int):
    """(``L`` lines, the pool of 40 ids on them): words, short numbers and 0..3 ids per line in
    either letter case; from 63 lines on, at fixed places (the first and the last line included):
    tokens of 7 / 8 / 64 / 65 bytes, a token without a digit, tokens cut by byte 1024 to a key and
    to none, 8 / 9 / 20 ids on a line, repeats, bytes >= 0x80, an empty line, a line of 5000 bytes."""
    rng = random.Random(seed)
    pool = [("%016x" % rng.getrandbits(64)).encode() for _ in range(30)] + [b"node%05d" % i for i in range(10)]
    lines = []
    for _ in range(L):
        words = [rng.choice([b"INFO", b"served", b"in", b"%dms" % rng.randrange(999), b"0x%x" % rng.getrandbits(16),
                             b"id=%d" % rng.randrange(1 << rng.choice((10, 40)))]) for _ in range(rng.randrange(1, 7))]
        for _ in range(rng.choice((0, 0, 1, 1, 2, 3))):
            x = rng.choice(pool)
            words.insert(rng.randrange(len(words) + 1), rng.choice((b"rid=", b"", b"[")) + rng.choice((x, x.upper())))
        lines.append(rng.choice((b" ", b"\t", b" - ")).join(words))
    if L >= 63:
        ids = [b"id%06dxx" % i for i in range(20)]
        special = [b"rid=" + pool[0], pool[1].upper(), b"x abcdef7 y", b"x abcdefg7 y", b"blob 9" + b"b" * 63 + b".",
                   b"blob 9" + b"b" * 64 + b".", b"level abcdefghijklmnopqrstuvwxyz reached", b"",
                   b"caf\xc3\xa9abcd1234\xff\x80 \x80zz99zz99", bytes(range(128, 256)) * 3,
                   b"rid=ABCDEF0123 again rid=abcdef0123 and AbCdEf0123.", b"x" * 1013 + b" abcdefgh12345678",
                   b"x" * 1015 + b" abcdefgh12345678", b"x" * 1023 + b" abcdefgh12345678", b"x" * 963 + b" 7" + b"c" * 70,
                   b"x" * 1013 + b" abcdefgh12345678 tail9999 " + pool[2] * 300, b" ".join(ids[:8]), b" ".join(ids[:9]),
                   b" ".join(ids), b" ".join(ids[:4] + ids[:4] + ids[4:8] + ids[:2] + ids[8:10]),
                   b" ".join(pool[:7]) + b" " + pool[3].upper() + b" " + pool[8] + b" " + pool[9]]
        at = [0, L - 1] + rng.sample(range(1, L - 1), len(special) - 2)
        for i, s in zip(at, special):
            lines[i] = s
    return lines, pool


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


def _table(device, keys):
    return K.GapTable.from_signatures(device, torch.tensor([_signed(k) for k in keys], dtype=torch.int64), cap=64)


def _raw(idx, sel, tab, cap: int, room: int, per_block: int):
    """One launch, no re-run: (line, key) buffers of ``room`` >= cap entries filled with canaries,
    hit, the two counters."""
    text, ls, ll = idx
    dev = text.device
    n = ls.numel() if sel is None else sel.numel()
    out_line = torch.full((room,), CANARY_LINE, dtype=torch.int32, device=dev)
    out_key = torch.full((room,), CANARY_KEY, dtype=torch.int64, device=dev)
    hit = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    N.line_keys(text.data_ptr(), text.numel(), ls.data_ptr(), ll.data_ptr(), ls.numel(), 0 if sel is None else sel.data_ptr(),
                n, None if tab is None else tab._tab(), 8, out_line.data_ptr(), out_key.data_ptr(), hit.data_ptr(), cap,
                cnt.data_ptr(), K._s(text), text.is_cuda, per_block)
    return out_line.cpu(), out_key.cpu(), hit.cpu(), cnt.tolist()


def _sorted_pairs(line, key):
    return sorted(zip(line.tolist(), key.tolist()))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_key_kernel_matches_twin(gpu_device, L):
    rng = random.Random(L)
    lines, pool = _lines(L, seed=L)
    held = [H(x) for x in pool[::2]] + [H(b"abcdefgh12"), H(b"id000003xx"), H(b"id000008xx")] + [H(b"absent%d" % i) for i in range(20)]
    forms = {"plain": (None, False), "sel": (sorted(rng.sample(range(L), max(1, L // 3))) + [L - 1, 0, 0], False),
             "table": (None, True), "sel+table": (list(range(L))[::-1], True)}
    golden_pairs = sorted((x, _signed(k)) for x, s in enumerate(lines) for k in golden.line_keys(s))
    for shift in (0, 1, 15):
        cpu = _index(lines, shift)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        assert gpu[0].numel() == cpu[0].numel() and gpu[0].data_ptr() % 16 == 0 and int(gpu[1][0]) % 16 == shift
        tabs = _table("cpu", held), _table(gpu_device, held)
        for name, (sel, filt) in forms.items():
            s_cpu = None if sel is None else torch.tensor(sel, dtype=torch.int32)
            s_gpu = None if sel is None else s_cpu.to(gpu_device)
            wl, wk, whit, (wn, wheld) = K.line_keys(*cpu, sel=s_cpu, table=tabs[0] if filt else None)
            want = _sorted_pairs(wl, wk)
            if name == "plain":                 # the twin is tied to the specification on the CPU
                assert want == golden_pairs and whit.tolist() == [int(bool(golden.line_keys(s))) for s in lines]
            assert wn == len(want) and wheld == int(whit.sum()) and (L < 63 or 0 < wn)
            for per_block in (0, 256, 2048):
                for cap in (None, 0, wn, wn - 1):
                    if cap is not None and cap < 0:
                        continue
                    what = (shift, name, per_block, cap)
                    gl, gk, ghit, (gn, gheld) = K.line_keys(*gpu, sel=s_gpu, table=tabs[1] if filt else None, cap=cap,
                                                            per_block=per_block)
                    assert gl.dtype == torch.int32 and gk.dtype == torch.int64 and ghit.dtype == torch.uint8 and gl.is_cuda, what
                    assert (gn, gheld) == (wn, wheld) and gl.numel() == gk.numel() == wn, what
                    assert torch.equal(ghit.cpu(), whit), what
                    assert _sorted_pairs(gl, gk) == want, what                    # (the GPU's order is unspecified)
                    if cap is None:
                        continue
                    # one launch with that capacity: the count is exact, the first `cap` slots hold
                    # `cap` of the pairs, and nothing is written past them
                    rl, rk, rhit, rcnt = _raw(gpu, s_gpu, tabs[1] if filt else None, cap, wn + 64, per_block)
                    assert rcnt == [wn, wheld] and torch.equal(rhit, whit), what
                    assert (rl[cap:] == CANARY_LINE).all() and (rk[cap:] == CANARY_KEY).all(), what
                    head = _sorted_pairs(rl[:cap], rk[:cap])
                    assert len(head) == cap and not Counter(head) - Counter(want) and (cap < wn or head == want), what


def test_full_and_empty_rounds(gpu_device):
    """Rounds at the bounds of the LDS stage: every one of 256 lanes emits 8 pairs (2048 pairs, the
    stage exactly full), and rounds in which no lane emits any -- alone, and next to a full one."""
    ids = [b"%08x" % (0x10000000 + i) for i in range(9 * 600)]
    full = [b" ".join(ids[9 * i:9 * i + 9]) for i in range(600)]                   # nine ids: the ninth is ignored
    none = [b"INFO nothing to see here %d" % i for i in range(600)]
    cases = {"full": full[:256], "none": none[:256], "full, none, full": full[:256] + none[:256] + full[256:512],
             "none, full, ragged": none[:256] + full[:256] + full[256:300], "alternating": [x for p in zip(full, none) for x in p][:700]}
    for name, lines in cases.items():
        cpu = _index(lines, 1)
        gpu = tuple(t.to(gpu_device) for t in cpu)
        wl, wk, whit, wcnt = K.line_keys(*cpu)
        n_full = sum(1 for x in lines if x in set(full))
        assert wcnt == (8 * n_full, n_full) and whit.tolist() == [int(x[:1] != b"I") for x in lines]
        for per_block in (0, 256, 512, 2048):
            gl, gk, ghit, gcnt = K.line_keys(*gpu, per_block=per_block)
            assert gcnt == wcnt and torch.equal(ghit.cpu(), whit), (name, per_block)
            assert _sorted_pairs(gl, gk) == _sorted_pairs(wl, wk), (name, per_block)
        # with a table that holds one id in nine: every lane emits, one pair each
        keys = [H(x) for x in ids[::9]]
        tabs = [K.GapTable.from_signatures(d, torch.tensor([_signed(k) for k in keys], dtype=torch.int64)) for d in ("cpu", gpu_device)]
        wl, wk, whit, wcnt = K.line_keys(*cpu, table=tabs[0])
        gl, gk, ghit, gcnt = K.line_keys(*gpu, table=tabs[1], per_block=256)
        assert gcnt == wcnt == (n_full, n_full) and torch.equal(ghit.cpu(), whit) and _sorted_pairs(gl, gk) == _sorted_pairs(wl, wk)


def test_no_lines_launch_nothing(gpu_device):
    text = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    none = torch.empty(0, dtype=torch.int64, device=gpu_device), torch.empty(0, dtype=torch.int32, device=gpu_device)
    line, key, hit, cnt = K.line_keys(text, *none)
    assert (line.numel(), key.numel(), hit.numel(), cnt) == (0, 0, 0, (0, 0)) and line.is_cuda
    ls, ll = torch.zeros(1, dtype=torch.int64, device=gpu_device), torch.full((1,), 8, dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError):
        K.line_keys(text, ls, ll, sel=torch.zeros(1, dtype=torch.int32))            # sel on another device
    with pytest.raises(ValueError):
        K.line_keys(text, ls, ll, table=K.GapTable("cpu"))                          # the table on another device
    with pytest.raises(ValueError):
        K.line_keys(text, ls, ll, sel=torch.ones(1, dtype=torch.int32, device=gpu_device))      # a line that is not there


# ---- the reports

def _library():
    return [PatternSet.model_validate({"metadata": {"library_id": "correlate"}, "patterns": [
        {"id": "aborted", "name": "request aborted", "severity": "HIGH",
         "primary_pattern": {"regex": r"request aborted:", "confidence": 0.9},
         "context_extraction": {"lines_before": 0, "lines_after": 2}},
        {"id": "dup", "name": "duplicate", "severity": "LOW",
         "primary_pattern": {"regex": r"\w+Dup foo", "confidence": 0.5},
         "context_extraction": {"lines_before": 1, "lines_after": 0}}]})]


@pytest.fixture(scope="module")
def report_case():
    """4000 lines of 150 interleaved requests, some CRLF line ends; every 500th line is an event of
    a second pattern and carries a node name that many lines share (keys with several event
    lines); the CPU parser and its report with every key -- shared by the tests below."""
    log, failing = correlated_log(4000, log_templates(20, seed=5), 150, seed=9, crlf_rate=0.1)
    lines = log.split("\n")
    taken = {i for at in failing.values() for i in at}
    for i in range(250, 4000, 500):
        while i in taken:                       # (not a line of a failing request: those stay as constructed)
            i += 1
        lines[i] = "WARN fooDup foo on node%05d again" % (i % 3) + ("\r" if lines[i].endswith("\r") else "")
    for i in range(100, 4000, 40):
        lines[i] = lines[i].rstrip("\r") + " host=node%05d" % (i % 3) + ("\r" if lines[i].endswith("\r") else "")
    log = "\n".join(lines)
    cpu = LogParser(_library(), config=Config.load(overrides={"engine.device": "cpu"}))
    want = cpu.correlate(log, top=None, min_lines=1, max_share=1.0)
    assert want == golden.correlate(log, _library(), cpu.config.scoring, top=None, min_lines=1, max_share=1.0)
    assert want["eventLines"] > 20 and want["keys"] > 20 and want["eventLines"] < want["keyLines"] < 3000
    assert {r["key"] for r in want["top"]} >= set(failing) | {"node00000", "node00001", "node00002"}
    assert any(r["eventLines"] > 1 for r in want["top"]) and any(r["lastLine"] > r["firstEventLine"] for r in want["top"])
    return log, cpu, want


@pytest.fixture(scope="module")
def gpu_parser(gpu_device):
    return LogParser(_library(), config=Config.load(overrides={"engine.device": str(gpu_device)}))


def test_report_gpu_equals_cpu_and_golden(gpu_device, gpu_parser, report_case):
    log, cpu, want = report_case
    data = log.encode()
    kw = {"top": None, "min_lines": 1, "max_share": 1.0}
    before = gpu_parser.frequency_statistics()
    assert gpu_parser.correlate(log, **kw) == want                                            # a document
    for c in (4096, 1 << 20):
        assert gpu_parser.correlate_stream(data, chunk_bytes=c, **kw) == want, c              # ~40-line chunks; one chunk
    head = "".join(log.splitlines(keepends=True)[:150])                                       # one-line chunks
    assert gpu_parser.correlate_stream(head.encode(), chunk_bytes=64, **kw) == cpu.correlate(head, **kw)
    res = gpu_parser.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3 and gpu_parser.correlate_resident(res, **kw) == want           # a resident log
    for order in ("events", "lines", "first"):
        kw = {"min_len": 9, "top": 5, "order": order, "min_lines": 3, "max_share": 0.1}
        got = gpu_parser.correlate(log, **kw)
        assert got == cpu.correlate(log, **kw) == golden.correlate(log, _library(), cpu.config.scoring, **kw)
        assert got == gpu_parser.correlate_stream(data, chunk_bytes=65536, **kw) == gpu_parser.correlate_resident(res, **kw)
        assert len(got["top"]) == 5
    assert gpu_parser.frequency_statistics() == before
