"""GPU: the signature group table kernels (csrc/kernels/gap_table.hip k_gap_fold, k_gap_winners,
k_gap_rows, k_gap_reinsert) against their host twins, and the stream / resident / corpus gap
reports on the GPU engine against the one-document report, the CPU engine and golden.gaps_corpus."""
import random

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.engine import Engine
from log_parser_amd.models.compiled import CompiledLibrary
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config, ScoringParams
from log_parser_amd.utils.synth import make_library, make_log

pytestmark = pytest.mark.gpu


def _rows(table):
    """Rows sorted by signature."""
    sig, count, first, docs = (x.cpu() for x in table.rows())
    o = torch.sort(sig)[1]
    return sig[o].tolist(), count[o].tolist(), first[o].tolist(), docs[o].tolist()


def _both(dev, launches, cap=1 << 12, tile=0):
    """Fold the launches [(sig, ord, doc)] into a GPU table and into the host twin: after every
    launch the winners agree as sets, at the end the rows agree."""
    gpu, cpu = K.GapTable(dev, cap=cap, tile=tile), K.GapTable("cpu", cap=cap)
    for sig, ordinal, doc in launches:
        sig, ordinal = torch.tensor(sig, dtype=torch.int64), torch.tensor(ordinal, dtype=torch.int64)
        got = gpu.fold(sig.to(dev), ordinal.to(dev), doc)
        want = cpu.fold(sig, ordinal, doc)
        assert got.dtype == torch.int64 and got.device.type == "cuda"
        assert sorted(got.cpu().tolist()) == sorted(want.tolist())
    assert _rows(gpu) == _rows(cpu)
    assert gpu.used == cpu.used and gpu.cap == cpu.cap
    return gpu, cpu


def _pool(k: int, seed: int):
    rng = random.Random(seed)
    return [rng.randrange(-(1 << 63), 1 << 63) for _ in range(k)]


# wave and block sizes; 257 is one block of k_gap_fold plus one pair at the tile a small launch
# gets (256), GT_TILE + 1 the same at the largest tile
SIZES = (1, 63, 64, 65, 257, K.GT_TILE + 1)


@pytest.mark.parametrize("distinct", [1, 7, 3000])
def test_fold_matches_twin(gpu_device, distinct):
    """Skewed signatures from a pool of 1 (all pairs on one slot), 7 and 3000 values; three launches
    per size, the last of a later document."""
    pool = _pool(distinct, seed=distinct)
    for n in SIZES:
        rng = random.Random(1000 * distinct + n)
        launches = []
        for doc in (0, 0, 2):
            sig = [pool[min(distinct - 1, int(distinct * rng.random() ** 4))] for _ in range(n)]
            launches.append((sig, [(doc << 40) | x for x in rng.sample(range(1 << 20), n)], doc))
        gpu, _ = _both(gpu_device, launches, tile=K.GT_TILE if n > K.GT_TILE else 0)
        if n == SIZES[-1]:
            assert sum(_rows(gpu)[1]) == 3 * n


def test_more_distinct_signatures_than_the_lds_table(gpu_device):
    """Every signature distinct, two tiles of the largest size (forced: a launch this small would get
    256-pair tiles): each block meets GT_TILE = 2048 distinct signatures, twice what its LDS table of
    GT_LDS_SLOTS = 1024 holds, so at least half of every tile takes the direct path to the global
    table -- and no pair is dropped. Then the same pairs at the tile the launch picks itself."""
    assert K.GT_TILE >= 2 * K.GT_LDS_SLOTS
    n = 2 * K.GT_TILE
    sig = _pool(n, seed=6)
    assert len(set(sig)) == n
    rng = random.Random(6)
    first = [rng.randrange(1 << 40) for _ in range(n)]
    for tile in (K.GT_TILE, 0):
        gpu, _ = _both(gpu_device, [(sig, first, 0), (sig[::-1], [x + 1 for x in first[::-1]], 1)], cap=1 << 14,
                       tile=tile)
        _, count, got_first, docs = _rows(gpu)
        assert gpu.used == n and count == [2] * n and docs == [2] * n and sorted(got_first) == sorted(first)
    with pytest.raises(ValueError):
        K.GapTable(gpu_device, tile=100)


def test_growth_from_cap_4(gpu_device):
    sig = _pool(5000, seed=4)
    rng = random.Random(4)
    launches = [(sig[lo:hi], [rng.randrange(1 << 40) for _ in range(hi - lo)], 0)
                for lo, hi in ((0, 1), (1, 3), (3, 700), (700, 5000))]
    launches.append((sig[:10], [-5] * 10, 1))                  # the groups go on counting after the growth
    gpu, _ = _both(gpu_device, launches, cap=4)
    assert gpu.used == 5000 and gpu.cap & (gpu.cap - 1) == 0 and gpu.cap >= 2 * gpu.used


def test_empty_marker_signature(gpu_device):
    m = K.GT_EMPTY
    gpu, _ = _both(gpu_device, [([m, -1, m, 0, -1, m], [9, 8, 4, 7, 6, 5], 0),
                                ([m, 3, 4, 5, 6, 7, 8, 9], [1 << 40] * 8, 1),       # grows with the marker inside
                                ([m] * 300 + [-1], list(range(2 << 40, (2 << 40) + 301)), 2)], cap=4)
    sig, count, first, docs = _rows(gpu)
    assert sig[0] == m and (count[0], first[0], docs[0]) == (304, 4, 3)


def test_second_launch_lowers_a_first(gpu_device):
    gpu, _ = _both(gpu_device, [([5, 5, 9], [40, 30, 7], 0), ([5, 9, 11, 5], [10, 8, 99, 20], 0), ([5], [10], 0)])
    assert _rows(gpu) == ([5, 9, 11], [5, 2, 1], [10, 7, 99], [1, 1, 1])


# ---- the reports on the GPU engine

@pytest.fixture(scope="module")
def report_case():
    """make_library(64, seed=1), a 20k-line log with CRLF line ends, ~300 spliced lines of 6 fixed
    templates (numbers vary), and the CPU engine's one-document report -- shared by the tests below."""
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
    data = "\n".join(lines).encode("utf-8")
    lib = CompiledLibrary(sets, ScoringParams())
    cpu = Engine(lib, Config.load(overrides={"engine.device": "cpu"}), device=torch.device("cpu"))
    return sets, data, {c: cpu.gaps_bytes(data, top=None, cover=c) for c in ("context", "events")}


@pytest.fixture(scope="module")
def gpu_parser(gpu_device, report_case):
    return LogParser(report_case[0], config=Config.load(overrides={"engine.device": str(gpu_device)}))


@pytest.fixture(scope="module")
def gpu_document(gpu_parser, report_case):
    """Engine.gaps_bytes on the GPU: the one-document twin of the stream."""
    return {c: gpu_parser.engine.gaps_bytes(report_case[1], top=None, cover=c) for c in ("context", "events")}


# 3000-byte chunks: ~700 chunks of ~30 lines, so most windows near a border cross it
@pytest.mark.parametrize("chunk_bytes", [3000, 1 << 16])
def test_stream_gpu_equals_document_and_cpu(gpu_parser, report_case, gpu_document, chunk_bytes):
    _, data, cpu = report_case
    before = gpu_parser.frequency_statistics()
    for cover in ("context", "events"):
        got = gpu_parser.gaps_stream(data, chunk_bytes=chunk_bytes, top=None, cover=cover)
        assert got == gpu_document[cover]
        assert got == cpu[cover]
    assert gpu_parser.gaps_stream(data, chunk_bytes=chunk_bytes, top=3)["top"] == cpu["context"]["top"][:3]
    assert gpu_parser.frequency_statistics() == before
    assert cpu["context"]["templates"] >= 6 and cpu["context"]["uncoveredErrorLines"] >= 250


def test_resident_gpu_equals_document(gpu_parser, report_case):
    _, data, cpu = report_case
    res = gpu_parser.load_resident(data, chunk_bytes=1 << 16)
    assert len(res.chunks) > 3 and res.chunks[0][0].is_cuda
    for cover in ("context", "events"):
        assert gpu_parser.gaps_resident(res, top=None, cover=cover) == cpu[cover]


def test_corpus_gpu_equals_golden(gpu_parser, report_case):
    sets, data, _ = report_case
    lines = data.decode("utf-8").split("\n")
    docs = ["\n".join(lines[k * 150:(k + 1) * 150]) for k in range(8)]     # 8 small documents
    docs[5] = ""
    want = golden.gaps_corpus(docs, sets, ScoringParams(), None, "context")
    assert want["documents"] == 8 and want["templates"] >= 3
    assert max(g["documents"] for g in want["top"]) >= 2
    assert gpu_parser.gaps_corpus(docs, top=None) == want
    assert gpu_parser.gaps_corpus(docs, top=2, cover="events") == golden.gaps_corpus(docs, sets, ScoringParams(), 2, "events")
