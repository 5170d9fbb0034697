"""Lines for the values tests (test_values.py, test_gpu_values.py): hand-written lines with the values
``golden.line_values`` must give, and random lines of words, numbers, units and ids."""
import random

import torch

from log_parser_amd.ops import kernels as K

S = b"2025-09-19T12:01:02"          # a valid stamp core: 19 bytes

# (line, [(field, value)])
HAND = [
    # digits: 9 against 10; units: 3 letters against 4
    (b"took 123456789 us", [(0, 123456789)]), (b"took 1234567890 us", []),
    (b"999999999 0 007 0000000012", [(0, 999999999), (1, 0), (2, 7)]),
    (b"heap 498MB of 512MiB used 12abc 12abcd", [(0, 498), (1, 512), (2, 12)]),
    (b"served in 31874ms, 3rd retry 5 of 5", [(0, 31874), (1, 3), (2, 5), (3, 5)]),
    # shapes without a value are fields all the same: j skips
    (b"at 0x1f then 5", [(1, 5)]), (b"a1b2 c3 4d 2h30m 6", [(2, 4), (4, 6)]), (b"0xff 0xabcd 0x12", [(0, 0)]),
    (b"12.5 -7 +8 1e3 1_000", [(0, 12), (1, 5), (2, 7), (3, 8), (5, 1), (6, 0)]),
    # the stamp: at byte 31 it hides its tokens, at byte 32 it is no stamp
    (b" " * 31 + S + b" took 5ms", [(0, 5)]),
    (b" " * 32 + S + b" took 5ms", [(0, 2025), (1, 9), (3, 1), (4, 2), (5, 5)]),
    (S + b" took 9ms", [(0, 9)]), (S.replace(b"T", b" ") + b",123456+05:30 took 9ms", [(0, 9)]),
    (S + b".5 took 9ms", [(0, 9)]), (S + b"Z took 9ms", [(0, 9)]), (S + b"+0530 4", [(0, 4)]),
    (S + b".123456789Z 4", [(0, 4)]), (S + b".1234567891 4", [(0, 4)]), (S + b". 5", [(0, 5)]),
    (S + b"-07 3", [(0, 7), (1, 3)]), (S + b"+05:3 3", [(0, 5), (1, 3), (2, 3)]),
    (b"[" + S + b"] 17 items", [(0, 17)]), (b"x" + S + b" 17", [(1, 9), (3, 1), (4, 2), (5, 17)]),
    # an invalid stamp hides nothing: month 13, zone hour 24
    (b"2025-13-19T12:01:02 x 7", [(0, 2025), (1, 13), (3, 1), (4, 2), (5, 7)]),
    (S + b"+2400 x 7", [(0, 2025), (1, 9), (3, 1), (4, 2), (5, 2400), (6, 7)]),
    (b"1969-09-19T12:01:02 7", [(0, 1969), (1, 9), (3, 1), (4, 2), (5, 7)]),
    # a token glued to the stamp starts before its end
    (b"2025-09-19T12:01:00Z7 up 3", [(0, 3)]), (b"2025-09-19T12:01:007 up 3", [(0, 3)]),
    (b"2025-09-19T12:01:00.5ms up 3", [(0, 3)]),
    # the cut at byte 1024: to a shorter value, to a 9-digit value from a 10-digit run, to nothing
    (b"x" * 1019 + b" 123456", [(0, 1234)]), (b"x" * 1014 + b" 1234567890", [(0, 123456789)]),
    (b"x" * 1013 + b" 1234567890", []), (b"x" * 1023 + b" 77", []), (b"x" * 1022 + b" 77", [(0, 7)]),
    (b"x" * 1018 + b" 12abcd", [(0, 12)]), (b"y" * 1000 + b" 5 " + b"z" * 4000 + b" 6", [(0, 5)]),
    # 8, 9 and 20 fields
    (b" ".join(b"%d" % (i + 10) for i in range(8)), [(i, i + 10) for i in range(8)]),
    (b" ".join(b"%d" % (i + 10) for i in range(9)), [(i, i + 10) for i in range(8)]),
    (b" ".join(b"%dms" % (i + 10) for i in range(20)), [(i, i + 10) for i in range(8)]),
    (b"a1 b2 c3 d4 e5 f6 g7 8 9", [(7, 8)]), (b"a1 b2 c3 d4 e5 f6 g7 h8 9", []),
    (S + b" " + b" ".join(b"%d" % i for i in range(9)), [(i, i) for i in range(8)]),
    # nothing, and bytes >= 0x80
    (b"", []), (b"no digit at all", []), (b"7", [(0, 7)]), (b"caf\xc3\xa912 \xff7ms\x80", [(0, 12), (1, 7)]),
    (bytes(range(128, 256)) + b"3" + bytes(range(128, 256)), [(0, 3)]),
    (b"queue depth 10432\tlag 15s", [(0, 10432), (1, 15)]), (b"the last line ends with a value 42ms", [(0, 42)]),
]


def random_lines(n: int, seed: int):
    """``n`` lines of words, numbers with and without units, hex numbers, ids in either letter case,
    under a stamp or not; blank and long ones among them; the last is not empty."""
    rng = random.Random(seed)
    pool = [("%016x" % rng.getrandbits(64)).encode() for _ in range(30)] + [b"node%05d" % i for i in range(10)]
    units = (b"", b"", b"ms", b"s", b"MB", b"KiB", b"rd", b"usec", b"x")
    out = []
    for i in range(n):
        words = [rng.choice([b"INFO", b"served", b"in", b"%dms" % rng.randrange(999), b"0x%x" % rng.getrandbits(rng.choice((8, 16, 40))),
                             b"id=%d" % rng.randrange(1 << rng.choice((10, 40))),
                             b"%d%s" % (rng.randrange(10 ** rng.choice((1, 3, 8, 9, 10))), rng.choice(units)),
                             b"%d.%03d" % (rng.randrange(100), rng.randrange(1000)), b"0" * rng.randrange(1, 12)])
                 for _ in range(rng.randrange(0, 9))]
        for _ in range(rng.choice((0, 0, 1, 1, 2, 3, 12))):
            x = rng.choice(pool)
            words.insert(rng.randrange(len(words) + 1), rng.choice((b"rid=", b"", b"[")) + rng.choice((x, x.upper())))
        line = rng.choice((b" ", b"\t", b" - ")).join(words)
        stamp = rng.choice((b"", b"", b"2025-09-19T12:%02d:%02d.%03dZ " % (i // 60 % 60, i % 60, i % 1000),
                            b"[2025-09-19 12:%02d:%02d,%03d+02:00] " % (i // 60 % 60, i % 60, i % 1000),
                            b"2025-19-09 12:00:%02d " % (i % 60), b"%s2025-09-19T12:00:%02d%d " % (b" " * rng.randrange(25, 36), i % 60, i % 7)))
        out.append(stamp + line * rng.choice((1, 1, 1, 30)))
    return out + [b"done 1"]


def index(lines, shift: int):
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
