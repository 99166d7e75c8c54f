"""Gzip members for the decoder tests (test_gzip_decode_host.py, test_gpu_gzip_decode.py): the
valid set, the frames the batch plan sends to the host, and one corrupt member per verdict.
Nothing here needs a device.  The module proves with zh_debug_gzip_blocks that the valid set
reaches the cases it is meant to reach (coverage())."""
import functools
import random
import struct
import zlib

from zarrhip import _abi as A
from zarrhip import _lib

HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"


# ---- a small DEFLATE writer -------------------------------------------------------------------
class Bits:
    """An LSB-first bit stream (RFC 1951 §3.1.1)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):          # a Huffman code (value, length): first bit first
        v, n = c
        for k in range(n - 1, -1, -1):
            self.bits((v >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code (RFC 1951 §3.2.2)."""
    code, out = 0, {}
    for n in range(1, 16):
        for s, ln in enumerate(lengths):
            if ln == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
# a complete code-length code over all 19 symbols: 13 of 4 bits, 6 of 5 bits
CL_LENGTHS = [4] * 13 + [5] * 6
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
            115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
             1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


def block_header(w, final, btype):
    w.bits(1 if final else 0, 1)
    w.bits(btype, 2)


def stored(w, final, data):
    block_header(w, final, 0)
    w.align()
    w.raw(struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data)


def symbols(w, lit, dist, items):
    """items: ints (literal / end of block), ("m", length, distance) or ("raw", lit symbol)."""
    for it in items:
        if isinstance(it, int):
            w.code(lit[it])
        elif it[0] == "raw":
            w.code(lit[it[1]])
        else:
            _, ln, d = it
            k = max(i for i in range(29) if LEN_BASE[i] <= ln)
            if ln == 258:
                k = 28
            w.code(lit[257 + k])
            w.bits(ln - LEN_BASE[k], LEN_EXTRA[k])
            j = max(i for i in range(30) if DIST_BASE[i] <= d)
            w.code(dist[j])
            w.bits(d - DIST_BASE[j], DIST_EXTRA[j])


def fixed(w, final, items):
    block_header(w, final, 1)
    symbols(w, FIXED_LIT, FIXED_DIST, items)


def dynamic(w, final, litlens, distlens, items, cl_syms=None, hlit=None, hdist=None):
    """A dynamic block.  cl_syms: the code-length symbols as (symbol, extra value) pairs; by
    default one symbol 0..15 per length."""
    block_header(w, final, 2)
    w.bits((len(litlens) if hlit is None else hlit) - 257, 5)
    w.bits((len(distlens) if hdist is None else hdist) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(CL_LENGTHS[s], 3)
    cl = canonical(CL_LENGTHS)
    if cl_syms is None:
        cl_syms = [(n, 0) for n in list(litlens) + list(distlens)]
    for s, extra in cl_syms:
        w.code(cl[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    symbols(w, canonical(litlens), canonical(distlens), items)


def member(deflate, data, header=HEADER, crc=None, isize=None):
    return header + deflate + struct.pack(
        "<II", zlib.crc32(data) if crc is None else crc,
        (len(data) & 0xFFFFFFFF) if isize is None else isize)


def lit_lengths(d):
    """286 literal/length code lengths from {symbol: length}."""
    return [d.get(s, 0) for s in range(max(d) + 1)] + [0] * max(0, 257 - (max(d) + 1))


def zgz(data, level=5, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    return c.compress(data) + c.flush()


def header_with(flags, extra=b"ab\x02\x00xy", name=b"chunk.bin", comment=b"a comment", bad_crc=False):
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\x11\x22\x33\x44\x02\x03")
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) ^ (1 if bad_crc else 0))
    return bytes(h)


def text(n=100 << 10):
    rng = random.Random(5)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 9)))
             for _ in range(400)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b" " if rng.random() < 0.9 else b".\n")
    return bytes(out[:n])


def fibonacci_input():
    """23 byte values with counts 1, 1, 2, 3, 5, ...: literal codes of 15 bits under
    Z_HUFFMAN_ONLY."""
    a, b, out = 1, 1, bytearray()
    for v in range(23):
        out += bytes([65 + v]) * a
        a, b = b, a + b
    lst = list(out)
    random.Random(3).shuffle(lst)
    return bytes(lst)


def one_distance_code():
    """A dynamic block with exactly one distance code, of length 1: a, b, match(3, distance 1)."""
    w = Bits()
    dynamic(w, True, lit_lengths({97: 2, 98: 2, 256: 2, 257: 2}), [1],
            [97, 98, ("m", 3, 1), 256])
    return b"abbbb", member(w.done(), b"abbbb")


def no_distance_codes():
    """A dynamic block of literals only: every distance length is zero."""
    w = Bits()
    dynamic(w, True, lit_lengths({120: 1, 121: 2, 256: 2}), [0], [120, 121, 120, 120, 256])
    return b"xyxx", member(w.done(), b"xyxx")


def mixed_blocks():
    """dynamic -> fixed -> stored -> dynamic; no Huffman block ends on a byte boundary."""
    w = Bits()
    lits = lit_lengths({97: 2, 98: 2, 256: 2, 257: 2})
    dynamic(w, False, lits, [1], [97, 98, ("m", 3, 1), 256])
    assert w.n != 0
    fixed(w, False, [99, 100, ("m", 4, 2), ("m", 5, 7), 256])
    assert w.n != 0
    stored(w, False, b"stored bytes")
    dynamic(w, True, lits, [1], [98, 97, ("m", 3, 1), 256])
    assert w.n != 0
    data = b"abbbb" + b"cdcdcd"
    data += data[-7:-2]
    data += b"stored bytes" + b"baaaa"
    return data, member(w.done(), data)


def far_match():
    """A stored block of 32 768 bytes, then a match at distance 32 768, the window's edge."""
    base = random.Random(9).randbytes(32768)
    w = Bits()
    stored(w, False, base)
    fixed(w, True, [("m", 10, 32768), 33, 256])
    data = base + base[:10] + b"!"
    return data, member(w.done(), data)


def big_stored():
    data = random.Random(8).randbytes(65535)
    w = Bits()
    stored(w, False, data)
    stored(w, True, b"")
    return data, member(w.done(), data)


@functools.lru_cache(maxsize=None)
def valid():
    """(label, data, member) triples every decoder must accept."""
    out = []
    txt = text()
    rng = random.Random(4)
    small = bytes(rng.choice(b"zarr chunk ") for _ in range(3000))
    for level in (0, 1, 5, 9):
        out.append((f"zlib level {level} text", txt, zgz(txt, level)))
        out.append((f"zlib level {level} small", small, zgz(small, level)))
    for name, st in (("fixed", zlib.Z_FIXED), ("huffman only", zlib.Z_HUFFMAN_ONLY),
                     ("rle", zlib.Z_RLE)):
        out.append((f"zlib {name} small", small, zgz(small, 6, st)))
        out.append((f"zlib {name} text", txt[:30000], zgz(txt[:30000], 6, st)))
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    m = (c.compress(txt[:5000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(txt[5000:9000]) +
         c.flush(zlib.Z_FULL_FLUSH) + c.compress(txt[9000:12000]) + c.flush())
    out.append(("sync and full flush", txt[:12000], m))
    for bs in (1 << 10, 16 << 10, 32 << 10):
        out.append((f"own writer {bs}", txt, _lib.gzip_compress(txt, bs)))
        out.append((f"own writer {bs} small", small, _lib.gzip_compress(small, bs)))
    body = zgz(small)[10:]
    for name, flags in (("FNAME", 8), ("FEXTRA", 4), ("FCOMMENT", 16), ("FHCRC", 2),
                        ("every header field", 1 | 2 | 4 | 8 | 16)):
        out.append((f"header {name}", small, header_with(flags) + body))
    for n in (0, 1, 63, 64, 65, 129):   # the edges of the 64-literal run
        d = bytes(k % 128 for k in range(n))
        out.append((f"{n} literals", d, zgz(d, 6, zlib.Z_FIXED)))
    zeros = bytes(70000)
    out.append(("70000 zeros", zeros, zgz(zeros, 9)))
    out.append(("stored 65535 then empty",) + big_stored())
    out.append(("mixed blocks",) + mixed_blocks())
    fib = fibonacci_input()
    out.append(("fibonacci counts", fib, zgz(fib, 6, zlib.Z_HUFFMAN_ONLY)))
    out.append(("one distance code",) + one_distance_code())
    out.append(("no distance codes",) + no_distance_codes())
    out.append(("distance 32768",) + far_match())
    for label, data, m in out:
        assert zlib.decompress(m, 31) == data, label
    return out


def coverage():
    """What zh_debug_gzip_blocks sees in the valid set: the cases the tests rely on."""
    rows = [(label, r) for label, _, m in valid() for r in _lib.gzip_blocks(m)]
    return {
        "fifteen_bit_code": any(r[5] == 15 for _, r in rows),
        "one_distance_code": any(r[0] == 2 and r[7] == 1 and r[6] == 1 for _, r in rows),
        "no_distance_code": any(r[0] == 2 and r[7] == 0 for _, r in rows),
        "distance_32768": any(r[8] == 32768 for _, r in rows),
        "block_types": {r[0] for _, r in rows},
        "several_dynamic_blocks": any(
            sum(1 for r in _lib.gzip_blocks(m) if r[0] == 2) > 1 for _, _, m in valid()),
    }


@functools.lru_cache(maxsize=None)
def host_routed():
    """(label, data, member, host_only): frames the batch hands to zh_gzip_decompress."""
    small = valid()[1]
    other = valid()[3]
    return [
        ("trailing bytes", small[1], small[2] + b"\xff" * 8, 0),
        ("two members", small[1], small[2] + other[2], 0),
        ("host_only", other[1], other[2], 1),
        # the last four bytes read as a size of 1: the batch call finds the real size too large
        # for the planned slot, and the wrapper plans the frame for the host
        ("hidden size", small[1], small[2] + b"\x01\x00\x00\x00", 0),
    ]


def frames_of(routed):
    """host_routed() rows as _lib.gzip_frame_array takes them; the list keeps the bytes alive."""
    import ctypes as C
    keep, frames = [], []
    for _, _, m, host_only in routed:
        b = (C.c_char * len(m)).from_buffer_copy(m)
        keep.append(b)
        frames.append((C.addressof(b), len(m), host_only))
    return frames, keep


def host_decode(m):
    """(status, bytes or None, text) of zh_gzip_decompress."""
    try:
        return A.ZH_OK, _lib.gzip_decompress(m), ""
    except _lib.ZhError as e:
        return e.status, None, str(e)


@functools.lru_cache(maxsize=None)
def corrupt():
    """(kind, member) pairs, one per verdict a header or a stream can raise; TEXTS has the text
    zh_gzip_decompress gives each."""
    good = valid()[1][2]
    txt_m = valid()[0][2]
    out = []
    out.append(("magic", b"\x1f\x8c" + good[2:]))
    out.append(("CM", good[:2] + b"\x07" + good[3:]))
    out.append(("reserved FLG bit", good[:3] + b"\x20" + good[4:]))
    out.append(("header truncated", good[:7]))
    out.append(("FHCRC mismatch", header_with(2 | 8, bad_crc=True) + good[10:]))

    def hand(build, data=b"", **kw):
        w = Bits()
        build(w)
        return member(w.done(), data, **kw)

    def btype3(w):
        block_header(w, True, 3)
    out.append(("BTYPE 3", hand(btype3)))

    def bad_len(w):
        block_header(w, True, 0)
        w.align()
        w.raw(struct.pack("<HH", 5, 5) + b"hello")
    out.append(("LEN/NLEN mismatch", hand(bad_len, b"hello")))
    out.append(("over-subscribed lengths", hand(lambda w: dynamic(
        w, True, lit_lengths({97: 1, 98: 1, 256: 1}), [1], [97, 256]), b"a")))
    out.append(("incomplete lengths", hand(lambda w: dynamic(
        w, True, lit_lengths({97: 2, 256: 2}), [1], [97, 256]), b"a")))
    lits = lit_lengths({97: 2, 98: 2, 256: 2, 257: 2})
    out.append(("repeat without a predecessor", hand(lambda w: dynamic(
        w, True, lits, [1], [97, 256], cl_syms=[(16, 0)] + [(n, 0) for n in lits[3:] + [1]]),
        b"a")))
    out.append(("repeat overrun", hand(lambda w: dynamic(
        w, True, lits, [1], [97, 256],
        cl_syms=[(n, 0) for n in lits[:250]] + [(18, 127)]), b"a")))
    out.append(("no end-of-block code", hand(lambda w: dynamic(
        w, True, lit_lengths({97: 1, 98: 1}), [1], [97, 98]), b"ab")))
    out.append(("symbol 286", hand(lambda w: fixed(w, True, [97, ("raw", 286), 256]), b"a")))

    def dist30(w):
        block_header(w, True, 1)
        symbols(w, FIXED_LIT, FIXED_DIST, [97, 98, 99])
        w.code(FIXED_LIT[257])
        w.code(FIXED_DIST[30])
        w.code(FIXED_LIT[256])
    out.append(("distance symbol 30", hand(dist30, b"abc")))
    out.append(("distance too far back", hand(
        lambda w: fixed(w, True, [97, ("m", 3, 2), 256]), b"aaaa")))
    out.append(("truncated in a code", txt_m[:len(txt_m) // 2]))
    out.append(("truncated before the trailer", good[:-5]))
    out.append(("CRC mismatch", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:]))
    out.append(("ISIZE mismatch", good[:-4] + struct.pack("<I", len(valid()[1][1]) + 1)))
    out.append(("output past ISIZE", good[:-4] + struct.pack("<I", len(valid()[1][1]) - 5)))
    for kind, m in out:
        try:
            zlib.decompress(m, 31)
        except zlib.error:
            continue
        raise AssertionError(f"zlib accepts the corrupt member {kind!r}")
    return out


TEXTS = {
    "magic": "gzip: incorrect header check",
    "CM": "gzip: unknown compression method",
    "reserved FLG bit": "gzip: unknown header flags set",
    "header truncated": "gzip: header truncated",
    "FHCRC mismatch": "gzip: header crc mismatch",
    "BTYPE 3": "gzip: invalid block type",
    "LEN/NLEN mismatch": "gzip: invalid stored block lengths",
    "over-subscribed lengths": "gzip: invalid literal/lengths set",
    "incomplete lengths": "gzip: invalid literal/lengths set",
    "repeat without a predecessor": "gzip: invalid bit length repeat",
    "repeat overrun": "gzip: invalid bit length repeat",
    "no end-of-block code": "gzip: invalid code -- missing end-of-block",
    "symbol 286": "gzip: invalid literal/length code",
    "distance symbol 30": "gzip: invalid distance code",
    "distance too far back": "gzip: invalid distance too far back",
    "truncated in a code": "gzip: incomplete or truncated stream",
    "truncated before the trailer": "gzip: trailer truncated",
    "CRC mismatch": "gzip: incorrect data check",
    "ISIZE mismatch": "gzip: incorrect length check",
    "output past ISIZE": "gzip: incorrect length check",
}


def mutations(count, seed=2024, limit=4096):
    """`count` seeded mutations of one to three bytes of the valid members of at most `limit`
    bytes (a tenth of them also cut short)."""
    rng = random.Random(seed)
    pool = [m for _, _, m in valid() if len(m) <= limit]
    out = []
    for _ in range(count):
        m = bytearray(rng.choice(pool))
        for _ in range(rng.randint(1, 3)):
            i = rng.randrange(len(m))
            m[i] = rng.randrange(256) if rng.random() < 0.5 else m[i] ^ (1 << rng.randrange(8))
        if rng.random() < 0.1:
            m = m[:rng.randrange(1, len(m) + 1)]
        out.append(bytes(m))
    return out
