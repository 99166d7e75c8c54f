"""The input matrix of the gzip member writer's tests (test_gzip_encode_host.py on the host,
test_gpu_gzip_encode.py on the device): (label, bytes, blocksize) rows, blocksize 0 being the
default, and a walk over the segments of a member the writer made.  The generators are those of
zstd_enc_inputs.py; the DEFLATE-specific inputs are added here."""
import struct

import numpy as np

from zstd_enc_inputs import far, labels, mix, random_bytes, sizes, text  # noqa: F401

DEFAULT_BLOCK = 16 << 10     # zh_gz::kDefaultBlock
MAX_BLOCK = 32 << 10         # zh_gz::kMaxBlock: DEFLATE's window; holds far() in one block
BLOCKSIZES = (1 << 10, 0, MAX_BLOCK)
HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
MARKER = b"\x00\x00\xff\xff"
# the first length of every length code of RFC 1951 §3.2.5 (257..285)
LENGTH_BASES = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83,
                99, 115, 131, 163, 195, 227, 258)


def zero_runs():
    """Runs of one byte value (0 first, another value for each run, so no run matches an
    earlier one) of 258 k + {0, 1, 2, 3, 4} bytes, k = 1..3, random bytes of 144..255 between
    them: the run's match is one byte shorter than the run, so its length crosses 258 k from
    both sides and the split rule meets every remainder."""
    rng = np.random.default_rng(21)
    out = []
    for k in (1, 2, 3):
        for r in (0, 1, 2, 3, 4):
            out.append(rng.integers(144, 256, 7, dtype=np.uint8).tobytes())
            out.append(bytes([len(out) // 2]) * (258 * k + r))
    return b"".join(out)


def high_bytes(n=5000):
    """Bytes of 144..255 only: the 9-bit literal codes.  Every block is stored."""
    return np.random.default_rng(22).integers(144, 256, n, dtype=np.uint8).tobytes()


def high_text():
    """text() with every byte moved up by 128: 9-bit literals between matches, fixed form."""
    return bytes(b | 0x80 for b in text()[:20000])


def length_codes():
    """Copies of the prefixes of one random piece between random 4-byte separators: prefix
    lengths at, one under and one over the first length of every length code, from 259, 258
    and 257 downwards, three times over.  The lengths fall, so every earlier copy holds the whole
    of a later one: the matcher finds each prefix whichever copy its table still points at.  A
    copy whose slot of the 1024-slot table another position has taken is matched a byte or two
    late, with other separators the next time round: three rounds reach every length."""
    rng = np.random.default_rng(23)
    piece = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    out = []
    for _ in range(3):
        out.append(piece)
        for base in reversed(LENGTH_BASES):
            for n in (base + 1, base, base - 1):
                if n < 4:
                    continue
                out.append(rng.integers(0, 256, 4, dtype=np.uint8).tobytes())
                out.append(piece[:n])
    return b"".join(out)


def matrix():
    rows = []
    for bs in BLOCKSIZES:
        for j, n in enumerate(sizes(bs)):
            rows.append((f"zeros-{n}-b{bs}", bytes(n), bs))
            rows.append((f"random-{n}-b{bs}", random_bytes(n, 100 + j), bs))
        rows.append((f"labels-b{bs}", labels(), bs))
        rows.append((f"text-b{bs}", text(), bs))
        rows.append((f"mix-b{bs}", mix(), bs))
        rows.append((f"far-b{bs}", far(), bs))
        rows.append((f"zero_runs-b{bs}", zero_runs(), bs))
        rows.append((f"high_bytes-b{bs}", high_bytes(), bs))
        rows.append((f"high_text-b{bs}", high_text(), bs))
        rows.append((f"length_codes-b{bs}", length_codes(), bs))
    return rows


def bound(n, bs):
    b = min(max(bs, 1 << 10), MAX_BLOCK) if bs else DEFAULT_BLOCK
    return 20 + n + 5 * -(-n // b)


# ---- a reader of the writer's two segment forms ----------------------------------------------
class _Bits:
    def __init__(self, data, pos):
        self.d, self.p = data, 8 * pos

    def take(self, n):          # LSB first
        v = 0
        for k in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v

    def code(self, n):          # Huffman codes are packed MSB first
        v = 0
        for _ in range(n):
            v = (v << 1) | self.take(1)
        return v


_LEXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
          1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)


def _fixed_symbol(b):
    v = b.code(7)
    if v <= 0b0010111:
        return 256 + v
    v = (v << 1) | b.take(1)
    if 0b00110000 <= v <= 0b10111111:
        return v - 0b00110000
    if 0b11000000 <= v <= 0b11000111:
        return 280 + v - 0b11000000
    v = (v << 1) | b.take(1)
    assert 0b110010000 <= v <= 0b111111111
    return 144 + v - 0b110010000


def segments(member):
    """[(form, raw bytes, segment bytes, [(length, distance, literals before it)] or None)] of a
    member the writer made: form "stored" or "fixed"; the matches of a fixed segment in order,
    each with the number of literals since the match before.  Asserts the layout:
    the header, byte-aligned segments, the sync marker, the 03 00 ending, the trailer's place."""
    assert member[:10] == HEADER
    p, out = 10, []
    while member[p:p + 2] != b"\x03\x00" or p + 10 != len(member):
        start = p
        if member[p] == 0:                                  # stored, not final
            n, nn = struct.unpack("<HH", member[p + 1:p + 5])
            assert n ^ nn == 0xFFFF and n > 0
            p += 5 + n
            out.append(("stored", n, p - start, None))
            continue
        b = _Bits(member, p)
        assert b.take(1) == 0 and b.take(2) == 1            # BFINAL 0, BTYPE 01
        nraw, nlit, matches = 0, 0, []
        while True:
            sym = _fixed_symbol(b)
            if sym == 256:
                break
            if sym < 256:
                nraw += 1
                nlit += 1
                continue
            assert sym <= 285
            ln = LENGTH_BASES[sym - 257] + b.take(_LEXTRA[sym - 257])
            dc = b.code(5)
            assert dc < 30
            dist = _DBASE[dc] + b.take(max(0, dc // 2 - 1))
            matches.append((ln, dist, nlit))
            nraw += ln
            nlit = 0
        assert b.take(3) == 0                               # the marker: BFINAL 0, BTYPE 00
        while b.p & 7:
            assert b.take(1) == 0
        p = b.p >> 3
        assert member[p:p + 4] == MARKER
        p += 4
        out.append(("fixed", nraw, p - start, matches))
    return out
