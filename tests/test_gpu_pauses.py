"""GPU: the pause scan (csrc/kernels/pauses.hip k_ps_tiles / k_ps_prefix / k_ps_emit) against its host
twin and the Python loop of pauses_cases -- rows in order, statistics, histogram and carry, exactly --
and the whole report GPU engine == CPU engine == golden.pauses for a document, streams, a resident
log and an accumulator in parts."""
import pytest
import torch

from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from pauses_cases import expected, parameter_sets, report_log, run_case, scan_cases, wanted

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(scan_cases()))
def test_pause_scan_kernel_matches_twin(gpu_device, name):
    got = run_case(name, gpu_device)
    assert got == run_case(name, "cpu")
    assert got == expected(name)


def test_pause_scan_adds_to_given_tensors(gpu_device):
    """Two runs into the same statistics and histogram, next to tensors that nobody scans into."""
    idle = K.pause_stats(gpu_device), torch.zeros(64, dtype=torch.int64, device=gpu_device)
    stats, hist = K.pause_stats(gpu_device), torch.zeros(64, dtype=torch.int64, device=gpu_device)
    ts = torch.tensor([10, 20, K.TS_NONE, 15, 2000], dtype=torch.int64, device=gpu_device)
    sig = torch.zeros(5, dtype=torch.int64, device=gpu_device)
    carry = None
    for base in (0, 5):
        rows, s, h, carry = K.pause_scan(ts, sig, 1000, base, carry, stats, hist)
        assert s is stats and h is hist and rows[0].is_cuda
    assert carry == (2000, 9, 0)
    assert stats.tolist() == [8, 3, 3970, 10, 2000] and hist.tolist()[:12] == [0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 2]
    assert idle[0].tolist() == K.pause_stats("cpu").tolist() and not idle[1].any()


def test_no_lines_launch_nothing(gpu_device):
    none = torch.empty(0, dtype=torch.int64, device=gpu_device)
    stats = K.pause_stats(gpu_device)
    rows, s, hist, carry = K.pause_scan(none, none, 1000, 7, (5, 3, -1), stats)
    assert all(c.numel() == 0 and c.is_cuda for c in rows) and s is stats and carry == (5, 3, -1)
    assert stats.tolist() == K.pause_stats("cpu").tolist() and hist.is_cuda and not hist.any()
    with pytest.raises(ValueError):
        K.pause_scan(none, none, 0)
    with pytest.raises(ValueError):
        K.pause_scan(torch.zeros(1, dtype=torch.int64, device=gpu_device), torch.zeros(1, dtype=torch.int64), 1000)


def test_report_gpu_equals_cpu_and_golden(gpu_device):
    text, planted = report_log()
    cpu = LogParser([], config=Config.load(overrides={"engine.device": "cpu"}))
    gpu = LogParser([], config=Config.load(overrides={"engine.device": str(gpu_device)}))
    data = text.encode()
    before = gpu.frequency_statistics()
    res = gpu.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3
    head = "".join(text.splitlines(keepends=True)[:150])                               # one-line chunks
    cut = len("".join(text.splitlines(keepends=True)[:planted[0][1] + 1]).encode())    # between the lines of a pause
    sets, wants = parameter_sets(), wanted()
    for kw, want in ((sets[k], wants[k]) for k in (0, 5, 8, 9)):
        assert cpu.pauses(text, **kw) == want, kw
        assert gpu.pauses(text, **kw) == want, kw                                             # a document
        for c in (4096, 1 << 22):
            assert gpu.pauses_stream(data, chunk_bytes=c, **kw) == want, (kw, c)              # ~40-line chunks; one chunk
        assert gpu.pauses_resident(res, **kw) == want, kw                                     # a resident log
        assert gpu.pauses_stream(head.encode(), chunk_bytes=64, **kw) == cpu.pauses(head, **kw), kw
        acc_kw = {k: v for k, v in kw.items() if k in ("min_ms", "by")}
        acc = gpu.pause_accumulator(longest=kw.get("top", 20), **acc_kw)                      # one log in two parts
        acc.add_document(data[:cut])
        acc.add_stream(data[cut:], 50000)
        assert acc.report(**{k: v for k, v in kw.items() if k not in acc_kw}) == want, kw
    assert gpu.frequency_statistics() == before
