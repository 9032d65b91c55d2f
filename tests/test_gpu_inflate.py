"""gm_inflate_bodies (gm_inflate.inc: a wave per gzip stream) against Python's zlib, byte for byte:
one batch holds every case, the malformed members last."""

import struct
import zlib

import numpy as np
import pytest

from gpumatch import engine, records

pytestmark = pytest.mark.gpu

RATIO = 8   # GM_INFLATE_RATIO


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    out, prev = b"", 0
    for cut in flush_at:
        out += co.compress(data[prev:cut]) + co.flush(zlib.Z_FULL_FLUSH)
        prev = cut
    return out + co.compress(data[prev:]) + co.flush()


def member(raw, isize, crc=0):
    return b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + raw + struct.pack("<II", crc, isize)


def gz_extra(data, pad):
    """data behind a header with a pad-byte FEXTRA field: a body long enough that RATIO * its length
    does not cut a payload that compresses better than RATIO to one."""
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\x03" + struct.pack("<H", pad) + bytes(pad) + co.compress(data) + co.flush() +
            struct.pack("<II", zlib.crc32(data), len(data)))


def bits(seq):
    return sum(b << i for i, b in enumerate(seq)).to_bytes((len(seq) + 7) // 8, "little")


def cases():
    rng = np.random.default_rng(7)
    text = " ".join(records._WORDS[int(k)] for k in rng.integers(0, len(records._WORDS), 1500)).encode()[:8192]
    rnd = rng.integers(0, 256, 33_000, dtype=np.uint8).tobytes()
    near = rng.integers(0, 256, 32_400, dtype=np.uint8).tobytes()
    # byte k twice as rare as byte k - 1: Huffman-only code lengths run up to 15 bits
    geo = np.concatenate([np.full(1 << (15 - k), 65 + k, np.uint8) for k in range(16)])
    rng.shuffle(geo)
    raw = zlib.compressobj(9, zlib.DEFLATED, -15)
    raw = raw.compress(text[:700]) + raw.flush()
    head = b"\x1f\x8b\x08\x1e\0\0\0\0\x00\x03" + struct.pack("<H", 5) + b"extra" + b"name.txt\0" + b"a comment\0"
    head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    zeros = gz(bytes(100 << 10), 9)
    good = [
        ("empty", gz(b"")), ("one_byte", gz(b"Q")),
        ("stored_70000", gz(rnd + rnd + rnd[:4000], 0)),
        ("fixed_200", gz(text[:200], 6, zlib.Z_FIXED)),
        ("dynamic_8k", gz(text, 9)),
        ("dist1_len258", gz_extra(b"a" * 1000, 120)), ("dist3", gz_extra(b"abc" * 500, 180)),
        ("random_33000_repeat", gz(rnd + rnd[:300], 9)),
        ("distance_32400", gz(near + near[:300], 9)),
        ("long_codes", gz(geo.tobytes(), 6, zlib.Z_HUFFMAN_ONLY)),
        ("full_flush_3", gz(text[:6000], 6, flush_at=(2000, 4000))),
        ("header_fields", head + raw + struct.pack("<II", zlib.crc32(text[:700]), 700)),
    ]
    out = [(name, b, zlib.decompress(b, wbits=31)) for name, b in good]
    assert all(len(x) <= RATIO * len(b) for _, b, x in out)   # none of these is cut
    out.append(("cut_at_limit", zeros, bytes(RATIO * len(zeros))))
    out += [("not_gzip", b"plain body, long enough to be one", None), ("short", gz(b"")[:17], None)]
    g = gz(text, 9)
    out += [
        ("truncated", g[:len(g) // 2] + g[-8:], None),
        ("isize_plus_1", g[:-4] + struct.pack("<I", len(text) + 1), None),
        ("isize_minus_1", g[:-4] + struct.pack("<I", len(text) - 1), None),
        ("block_type_3", member(bits([1, 1, 1]) + bytes(7), 0), None),
        # fixed block: length code 257 (len 3), distance code 0 (dist 1) with no output yet, EOB
        ("distance_before_start", member(bits([1, 1, 0] + [0] * 6 + [1] + [0] * 5 + [0] * 7) + bytes(4), 3), None),
    ]
    return out


CASES = cases()


@pytest.fixture(scope="module")
def inflated():
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    # (URI lengths differ, so the bodies start at every alignment)
    reqs, arena = records.from_dicts([{"host": "a.example.com", "uri": "/" + "u" * i, "body": b, "port": 80}
                                      for i, (_, b, _) in enumerate(CASES)])
    return engine.Engine(0).inflate_bodies(reqs, arena)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_inflate_matches_zlib(inflated, i):
    assert inflated[i] == CASES[i][2]
