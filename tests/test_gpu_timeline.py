"""GPU: the timestamp kernel (csrc/kernels/timeline.hip k_ts_parse), the forward-fill scans
(k_tl_tiles / k_tl_prefix / k_tl_fill) and the bucket histogram (k_tl_hist) against their host
twins, and the whole timeline report GPU engine == CPU engine == golden.timeline, in one piece and
as a stream."""
import random

import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.api import LogParser
from log_parser_amd.ops import kernels as K
from log_parser_amd.utils.config import Config
from log_parser_amd.utils.synth import make_library, make_log

pytestmark = pytest.mark.gpu

S = b"2025-09-19T12:00:00"
NONE = K.TS_NONE


def _index(data: bytes, dev):
    """(cpu text, ls, ll) and their device copies; the line index comes from the host twin."""
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    ls, ll = K.split_lines(text, len(data))
    return (text, ls, ll), (text.to(dev), ls.to(dev), ll.to(dev))


def _golden_ts(lines):
    return [NONE if t is None else t for t in map(golden.line_timestamp, lines)]


def test_ts_parse_matches_twin(gpu_device):
    lines = []
    size = 0

    def put(line):
        nonlocal size
        lines.append(line)
        size += len(line) + 1

    # a stamp at every start offset 0..32 of a line that starts at every offset mod 16: every way a
    # stamp can straddle the 16-byte loads; odd offsets behind bytes >= 0x80
    for a in range(16):
        for o in range(33):
            put(b"q" * ((a - size - 1) % 16))
            assert size % 16 == a
            pre = b"\xc3\xa9" * (o // 2) + b"\xff" if o % 2 else b"." * o
            put(pre + S + b".%03d%s rest of the line" % (a * 33 + o, (b"Z", b"+05:30", b"-0100", b"")[o % 4]))
    stamped_from = len(lines)
    long = b"." * 31 + S + b".123456789+05:30 tail " + b"x" * 5000    # the stamp ends with byte 67
    for n in (0, 1, 18, 19, 20, 66, 67, 68, 5000):
        put(long[:n])
        put((S + b"Z" + b"y" * 5000)[:n])
    put(b"\xff\xfe\x80 " + S + b",5")
    put(b"2025-13-19T12:00:00 " + S)                                   # invalid leftmost match
    put(b"2025-09 2025-2025-09-19 " + S)                               # failed attempts before the match
    put(b"1234567890" * 7)
    put(bytes(range(128, 256)))
    # the text ends with its last line, whose stamp ends it, exactly at a multiple of the line-index
    # tile: the last aligned load of the last line ends where the text's padding begins
    last = b"final " + S + b".123456789+05:30"
    put(b"f" * (-(size + len(last)) % K.NL_TILE + K.NL_TILE - 1))
    lines.append(last)
    data = b"\n".join(lines)
    assert len(data) % K.NL_TILE == 0
    (text, ls, ll), (dtext, dls, dll) = _index(data, gpu_device)
    assert ls.numel() == len(lines) and int(ls[-1]) + int(ll[-1]) == len(data)
    assert sorted(set((ls[1:stamped_from:2] % 16).tolist())) == list(range(16))
    want = K.line_timestamps(text, ls, ll)
    assert want.tolist() == _golden_ts(lines)                  # (the twin is tied to the oracle on the CPU)
    assert (want[1:stamped_from:2] != NONE).sum().item() == 16 * 32 and want[-1].item() != NONE
    got = K.line_timestamps(dtext, dls, dll)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("L", [1, 255, 256, 257, 4097])
def test_ts_parse_grid_edges(gpu_device, L):
    lines = [b"\tat x.Y(Z.java:%d)" % i if i % 5 == 4 else
             b"." * (i % 40) + b"2025-09-19T12:%02d:%02d.%03dZ line %d" % (i // 60 % 60, i % 60, i % 1000, i)
             for i in range(L)]
    (text, ls, ll), (dtext, dls, dll) = _index(b"\n".join(lines), gpu_device)
    assert ls.numel() == L
    want = K.line_timestamps(text, ls, ll)
    assert want[:64].tolist() == _golden_ts(lines[:64]) and want[-1].item() == _golden_ts(lines[-1:])[0]
    assert torch.equal(K.line_timestamps(dtext, dls, dll).cpu(), want)


# ---- k_tl_tiles / k_tl_prefix / k_tl_fill

@pytest.mark.parametrize("L", [1, 7, 8, 9, 2047, 2048, 2049, 4097, 2048 * 257 + 3])
def test_fill_matches_twin(gpu_device, L):
    """Around the tile edges (8 lines a lane, 2048 a block) and with more tiles than the 256 lanes
    of the prefix block; the twin is tied to a plain loop in tests/test_timeline.py."""
    g = torch.Generator().manual_seed(L)
    t0 = 1758283200000
    stamps = t0 + torch.randint(-500, 500, (L,), generator=g) * 1000
    ar = torch.arange(L)
    kinds = [torch.full((L,), NONE),                                               # nothing stamped
             torch.where(torch.rand(L, generator=g) < .7, stamps, NONE),
             torch.where(ar % 97 == 0, t0 - ar, NONE),                             # sparse, every stamp runs backwards
             torch.where(ar == min(3, L - 1), t0 + 5, NONE)]                       # one stamp fills every later tile
    for ts in kinds:
        for carry_last, carry_top in ((NONE, NONE), (t0 - 77, t0 + 100000)):
            want_eff, want_n = K.timeline_fill(ts, carry_last, carry_top)
            eff, n = K.timeline_fill(ts.to(gpu_device), carry_last, carry_top)
            assert eff.dtype == torch.int64 and torch.equal(eff.cpu(), want_eff), carry_last
            assert n.cpu().tolist() == want_n.tolist()
    assert (want_eff != NONE).all() and (K.timeline_fill(kinds[3])[0][:min(3, L - 1)] == NONE).all()


# ---- k_tl_hist

W = 60000


def _hist_case(name):
    """(eff, feat, ev_line, ev_pat, sev_index, t0, W, nb, S) of a named case (CPU tensors)."""
    rng = random.Random(name)
    L, E, S, t0, nb = 4097, 1500, 5, 1758283200000, 1
    if name == "one_bucket":                                # every item on one address: the contention path
        eff = [t0 + rng.randrange(W) for _ in range(L)]
    elif name == "own_bucket":                              # more distinct buckets in a tile than the block table holds
        nb = L
        eff = [t0 + i * W + rng.randrange(W) for i in range(L)]
        assert K.TL_TILE > K.TL_LDS_SLOTS
    elif name == "two_buckets_S1":
        nb, S = 2, 1
        eff = [t0 + rng.randrange(2 * W) for _ in range(L)]
    elif name == "undated_mixed":                           # a time-ordered log with undated lines and events
        nb = 300
        eff = sorted(t0 + rng.randrange(nb * W) for _ in range(L))
        eff = [NONE if rng.random() < .3 else t for t in eff]
    elif name == "no_events_S1":
        nb, S, E = 7, 1, 0
        eff = [t0 + rng.randrange(nb * W) for _ in range(L)]
    elif name == "negative_starts":
        t0, nb = -10 * W, 20
        eff = [t0 + rng.randrange(nb * W) for _ in range(L)]
    elif name == "shuffled_many":                           # no order at all, 2000 buckets
        nb = 2000
        eff = [NONE if rng.random() < .1 else t0 + rng.randrange(nb * W) for _ in range(L)]
    else:
        raise KeyError(name)
    P = 40
    feat = torch.tensor([rng.choice((0, 1, 2, 4, 5, 8, 9, 12, 13)) for _ in range(L)], dtype=torch.uint8)
    ev_line = torch.tensor(sorted(rng.randrange(L) for _ in range(E)), dtype=torch.int32)
    ev_pat = torch.tensor([rng.randrange(P) for _ in range(E)], dtype=torch.int32)
    sev_index = torch.tensor([rng.randrange(S) for _ in range(P)], dtype=torch.int32)
    return torch.tensor(eff, dtype=torch.int64), feat, ev_line, ev_pat, sev_index, t0, W, nb, S


@pytest.mark.parametrize("name", ["one_bucket", "own_bucket", "two_buckets_S1", "undated_mixed", "no_events_S1",
                                  "negative_starts", "shuffled_many"])
def test_hist_matches_twin(gpu_device, name):
    eff, feat, ev_line, ev_pat, sev_index, t0, w, nb, S = _hist_case(name)
    want = K.timeline_hist(eff, feat, ev_line, ev_pat, sev_index, t0, w, nb, S)
    assert want.shape == (nb, 3 + S)
    # the twin against plain counting
    dated = eff != NONE
    b = (eff[dated] - t0) // w
    assert torch.equal(want[:, 0], torch.bincount(b, minlength=nb))
    cand = ((feat & 9) != 0) & ((feat & 4) == 0)
    assert torch.equal(want[:, 1], torch.bincount((eff[dated & cand] - t0) // w, minlength=nb))
    ev_dated = dated[ev_line.long()]
    n_ev = int(ev_dated.sum())
    assert want.sum(0).tolist()[:3] == [int(dated.sum()), int((dated & cand).sum()), n_ev]
    assert int(want[:, 3:].sum()) == n_ev and torch.equal(want[:, 3:].sum(1), want[:, 2])
    if name in ("undated_mixed", "shuffled_many"):
        assert 0 < n_ev < ev_line.numel() and 0 < int(dated.sum()) < eff.numel()
    d = gpu_device
    got = K.timeline_hist(eff.to(d), feat.to(d), ev_line.to(d), ev_pat.to(d), sev_index.to(d), t0, w, nb, S)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)


def test_hist_ignores_what_lies_outside(gpu_device):
    """Times before t0 or behind the last bucket and events on lines outside [0, L) are counted
    nowhere (and written nowhere)."""
    t0 = 1758283200000
    eff = torch.tensor([t0 - 1, t0, t0 + 2 * W - 1, t0 + 2 * W, NONE, t0 + W], dtype=torch.int64)
    feat = torch.tensor([1, 1, 0, 1, 1, 8], dtype=torch.uint8)
    ev_line = torch.tensor([-1, 0, 1, 5, 6, 4], dtype=torch.int32)
    ev_pat = torch.tensor([0, 0, 1, 0, 0, 0], dtype=torch.int32)
    sev = torch.tensor([0, 1], dtype=torch.int32)
    want = K.timeline_hist(eff, feat, ev_line, ev_pat, sev, t0, W, 2, 2)
    assert want.tolist() == [[1, 1, 1, 0, 1], [2, 1, 1, 1, 0]]
    d = gpu_device
    got = K.timeline_hist(eff.to(d), feat.to(d), ev_line.to(d), ev_pat.to(d), sev.to(d), t0, W, 2, 2)
    assert torch.equal(got.cpu(), want)


# ---- the whole report

@pytest.fixture(scope="module")
def case():
    sets, trig = make_library(64, seed=1)
    log = "no stamp yet\n\tat x.Y(Z.java:1)\n" + make_log(20000, trig, seed=3, stack_rate=0.05, crlf_rate=0.1)
    cpu = LogParser(sets, config=Config.load(overrides={"engine.device": "cpu"}))
    return sets, log, cpu


@pytest.fixture(scope="module")
def gpu_parser(gpu_device, case):
    return LogParser(case[0], config=Config.load(overrides={"engine.device": str(gpu_device)}))


@pytest.mark.parametrize("bucket", [1, 60])
def test_report_gpu_cpu_golden(case, gpu_parser, bucket):
    sets, log, cpu = case
    want = golden.timeline(log, sets, cpu.config.scoring, bucket)
    assert want["outOfOrderLines"] > 0 and want["undatedLines"] == 2 and want["events"] > 0
    assert cpu.timeline(log, bucket_seconds=bucket) == want
    assert gpu_parser.timeline(log, bucket_seconds=bucket) == want
    data = log.encode()
    for c in (1 << 16, 300000):
        assert gpu_parser.timeline_stream(data, chunk_bytes=c, bucket_seconds=bucket) == want, c


def test_span_error_leaves_the_stream_clean(gpu_parser, tmp_path):
    """The ValueError leaves in the middle of a mapped file with chunks still queued: the mapping
    closes, no producer thread stays behind, and the next stream runs."""
    import threading
    doc = ("2025-09-19T12:00:00Z INFO a\n" + "INFO filler\n" * 40 + "1999-01-01T00:00:00Z ERROR a stray old date\n"
           + "INFO filler\n" * 400 + "2025-09-19T12:00:01Z INFO b\n")
    f = tmp_path / "stray.log"
    f.write_text(doc)
    threads = threading.active_count()
    for src in (str(f), doc.encode()):
        with pytest.raises(ValueError, match="larger bucket"):
            gpu_parser.timeline_stream(src, chunk_bytes=300)
    assert threading.active_count() == threads
    assert gpu_parser.timeline_stream(str(f), chunk_bytes=300, bucket_seconds=86400) == gpu_parser.timeline(doc, 86400)
