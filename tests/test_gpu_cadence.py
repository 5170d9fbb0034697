"""GPU: the beat scan (csrc/kernels/cadence.hip k_cd_tile / k_cdl_tiles / k_cdl_prefix / k_cdl_emit)
against its host twins and the Python loop of cadence_cases -- beats, buckets and state rows, exactly
and the same on every run -- and the whole report GPU engine == CPU engine == golden.cadence for a
document, streams, a resident log and an accumulator in parts."""
import pytest
import torch

from cadence_cases import expected, joined, parameter_sets, report_log, run_case, run_runs, scan_cases, wanted
from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(scan_cases()))
def test_beat_scan_kernel_matches_twin(gpu_device, name):
    got = run_case(name, gpu_device)
    assert got == run_case(name, "cpu")
    assert got == expected(name)


@pytest.mark.parametrize("name", ["skewed mix", "rows past every link block", "a template absent from a middle run"])
def test_two_runs_give_identical_rows(gpu_device, name):
    assert run_case(name, gpu_device) == run_case(name, gpu_device)


def test_split_runs_small_capacity_and_no_lines(gpu_device):
    for name in ("many small runs", "a middle run without a stamp"):
        split, one = run_case(name, gpu_device), run_runs(joined(name), gpu_device)
        assert split[2] == one[2] and sum(split[0], []) == one[0][0] and sum(split[1], []) == one[1][0]
    for cap in (0, 5):
        assert run_case("skewed mix", gpu_device, cap=cap) == expected("skewed mix")
    none = torch.empty(0, dtype=torch.int64, device=gpu_device)
    _, _, state = K.beat_scan(torch.tensor([5, 9], device=gpu_device), torch.tensor([1, 1], device=gpu_device))
    beat, bkt, same = K.beat_scan(none, none, 2, state)
    assert beat.is_cuda and beat.numel() == 0 and same is state and state[K.CD_MAX].tolist() == [4]
    with pytest.raises(ValueError):
        K.beat_scan(torch.zeros(1, dtype=torch.int64, device=gpu_device), torch.zeros(1, dtype=torch.int64))


def test_report_gpu_equals_cpu_and_golden(gpu_device):
    text, known = report_log()
    cpu = LogParser([], config=Config.load(overrides={"engine.device": "cpu"}))
    gpu = LogParser([], config=Config.load(overrides={"engine.device": str(gpu_device)}))
    data = text.encode()
    before = gpu.frequency_statistics()
    res = gpu.load_resident(data, chunk_bytes=32768)
    assert len(res.chunks) > 3
    lines = text.splitlines(keepends=True)
    head = "".join(lines[:150])                                                                  # one-line chunks
    cut = len("".join(lines[:(known["hole"]["fromLine"] + known["hole"]["toLine"]) // 2]).encode())    # inside the hole
    sets, wants = parameter_sets(), wanted()
    for kw, want in ((sets[k], wants[k]) for k in (0, 1, 4, 8)):
        assert cpu.cadence(text, **kw) == want, kw
        assert gpu.cadence(text, **kw) == want, kw                                             # a document
        for c in (4096, 1 << 22):
            assert gpu.cadence_stream(data, chunk_bytes=c, **kw) == want, (kw, c)              # ~40-line chunks; one chunk
        assert gpu.cadence_resident(res, **kw) == want, kw                                     # a resident log
        assert gpu.cadence_stream(head.encode(), chunk_bytes=64, **kw) == cpu.cadence(head, **kw), kw
        acc = gpu.cadence_accumulator()                                                        # one log in two parts
        acc.add_document(data[:cut])
        acc.add_stream(data[cut:], 50000)
        assert acc.report(**kw) == want, kw
    assert gpu.frequency_statistics() == before
