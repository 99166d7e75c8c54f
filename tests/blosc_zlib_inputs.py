"""Frames for the device decode of blosc frames with zlib streams (test_blosc_zlib_host.py on the
CPU, test_gpu_blosc_zlib.py on the device): blosc1 frames assembled by blosc_frames.frame_streams
over zlib streams written by Python's zlib (levels, strategies, flushes, window sizes) and a few
built bit by bit from RFC 1950 / 1951, the valid matrix, the frames the flag still leaves to the
host, a mixed batch and a fixed list of corrupt frames.  Every expected value is
zh_blosc_decompress on the same frame (blosc_frames.host_decode) and the input the frame was made
from.  Test infrastructure only; nothing here needs a device."""
import functools
import struct
import zlib

import numpy as np

import blosc_frames as bf
import blosc_zstd_inputs as zi
from blosc_zstd_inputs import datasets, shuffled_streams
from zarrhip import _lib

FLAG = 4               # ZH_BLOSC_ZLIB_DEVICE
ZSTD_FLAG = zi.FLAG    # ZH_BLOSC_ZSTD_DEVICE
KZLIB = 4              # zh_bs::kZlib, the method column of the stream table
LDS_BLOCK = zi.LDS_BLOCK
ADLER_SIZES = [1, 63, 64, 65, 5552, 5553, 65521, 65522]


def deflate(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    """bytes -> one zlib stream (compress2's header when wbits is 15)."""
    def run(b):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
        return c.compress(bytes(b)) + c.flush()
    return run


def sync_flushed(b):
    """A Z_SYNC_FLUSH in the middle: an empty stored block between two compressed ones."""
    b = bytes(b)
    c = zlib.compressobj(6)
    return c.compress(b[:len(b) // 2]) + c.flush(zlib.Z_SYNC_FLUSH) + \
        c.compress(b[len(b) // 2:]) + c.flush()


# ---- DEFLATE by hand (RFC 1951 3.2.6: the fixed codes) -----------------------------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
             115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
              1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


class Bits:
    """The bit stream of RFC 1951: fields from the low bit up, Huffman codes from their first
    (most significant) bit."""

    def __init__(self):
        self.bits = []

    def field(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]

    def code(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n - 1, -1, -1)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        self.align()
        return bytes(sum(b << k for k, b in enumerate(self.bits[i:i + 8]))
                     for i in range(0, len(self.bits), 8))


def _litlen(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_block(w, ops, final):
    """One fixed-Huffman block: ops are literal byte values or (length, distance) pairs."""
    w.field(1 if final else 0, 1)
    w.field(1, 2)
    for op in ops:
        if isinstance(op, int):
            _litlen(w, op)
            continue
        length, dist = op
        k = max(i for i, b in enumerate(_LEN_BASE) if b <= length)    # 258 has its own code
        _litlen(w, 257 + k)
        w.field(length - _LEN_BASE[k], _LEN_EXTRA[k])
        d = max(i for i, b in enumerate(_DIST_BASE) if b <= dist)
        w.code(d, 5)
        w.field(dist - _DIST_BASE[d], _DIST_EXTRA[d])
    _litlen(w, 256)


def stored_block(w, data, final):
    w.field(1 if final else 0, 1)
    w.field(0, 2)
    w.align()
    w.field(len(data), 16)
    w.field(len(data) ^ 0xFFFF, 16)
    for b in data:
        w.field(b, 8)


def expand(ops, history=b""):
    """What the ops of fixed_block decode to behind `history`."""
    out = bytearray(history)
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            for _ in range(op[0]):
                out.append(out[-op[1]])
    return bytes(out[len(history):])


def zlib_wrap(w, content):
    return b"\x78\x01" + w.bytes() + struct.pack(">I", zlib.adler32(content))


def far_match_stream():
    """(content, stream): 32 KiB in a stored block, then fixed-block matches at the distance
    32 768, the format's largest (zlib's own compressor stops 262 bytes short of it)."""
    head = datasets()["skew"][:32768]
    ops = [(258, 32768), (3, 32768), 65, (200, 32768), (258, 1)]
    w = Bits()
    stored_block(w, head, False)
    fixed_block(w, ops, True)
    content = head + expand(ops, head)
    return content, zlib_wrap(w, content)


# ---- frames ---------------------------------------------------------------------------------------
def frame(data, typesize, blocksize, zfn, shuffle="none", split=False, version=2, edit=None,
          keep=False):
    """A blosc1 frame with compressor code 3 whose streams are `zfn`'s zlib streams (or stored raw
    where that is not smaller, as c-blosc does; `keep` keeps a larger payload).
    `edit(block, stream, payload, raw)` may replace a payload."""
    blocks = []
    for b, parts in enumerate(shuffled_streams(data, typesize, blocksize, shuffle, split, version)):
        row = []
        for s, part in enumerate(parts):
            c = zfn(part)
            if len(c) >= len(part) and not keep:
                c = part
            if edit is not None:
                c = edit(b, s, c, part)
            assert len(c) != len(part) or c == part     # a payload of the raw size is raw
            row.append(c)
        blocks.append(row)
    return bf.frame_streams(blocks, len(data), typesize, blocksize, "zlib",
                            shuffle=shuffle == "byte", split=split, bitshuffle=shuffle == "bit",
                            version=version)


def one_stream(payload, rawsize, typesize=1):
    return bf.frame_streams([[payload]], rawsize, typesize, max(rawsize, 1), "zlib")


def zlib_streams(f):
    """The payloads of the kZlib streams of a frame (by the flagged stream table)."""
    return [bytes(f[r[1]:r[1] + r[2]]) for r in _lib.blosc_streams(f, FLAG)
            if r[0] == 1 and r[5] == KZLIB]


@functools.lru_cache(maxsize=None)
def runs():
    """Byte runs of 1 to 300: Z_RLE turns them into overlapping matches at distance 1."""
    rng = np.random.default_rng(20250114)
    return b"".join(bytes([int(v)]) * int(n) for v, n in
                    zip(rng.integers(0, 256, 120), rng.integers(1, 301, 120)))[:8192]


@functools.lru_cache(maxsize=None)
def matrix():
    """[(label, data, frame)]: every frame is one the flag sends to the device (where == 0)."""
    ds = datasets()
    big = LDS_BLOCK + 512
    out = []

    def add(label, data, *a, zfn=deflate(6), **kw):
        out.append((label, bytes(data), frame(data, *a, zfn=zfn, **kw)))
    for level in (1, 6, 9):
        add(f"level {level}", ds["words"][:4096], 1, 4096, zfn=deflate(level))
    for name in ("Z_FIXED", "Z_HUFFMAN_ONLY", "Z_RLE"):
        add(name, runs(), 1, len(runs()), zfn=deflate(6, getattr(zlib, name)))
    add("level 0: stored blocks", ds["skew"][:5000], 1, 5000, zfn=deflate(0), keep=True)
    add("sync flush in the middle", ds["words"][:6000], 1, 6000, zfn=sync_flushed)
    add("160 KiB in one stream", ds["skew"][:100 << 10] + ds["words"][:60 << 10], 1, 160 << 10)
    content, stream = far_match_stream()
    out.append(("matches at distance 32768", content, one_stream(stream, len(content))))
    add("byte shuffle, unsplit", ds["walk"][:32 << 10], 4, 32 << 10, shuffle="byte")
    add("split, raw and constant streams", ds["quad"], 4, 8192, shuffle="byte", split=True)
    add("split, 8 streams", ds["oct"], 8, 8192, shuffle="byte", split=True)
    add("split, 8 streams, 2 blocks and a tail", ds["oct"] * 2 + ds["oct"][:1004], 8, 8192,
        shuffle="byte", split=True)
    add("bit shuffle v2, 1003 elements", ds["walk"][:4 * 1003], 4, 4 * 1003, shuffle="bit")
    add("bit shuffle v2, 1024 elements", ds["walk"][:4096], 4, 4096, shuffle="bit")
    add("bit shuffle v3, 1003 elements", ds["walk"][:4 * 1003], 4, 4 * 1003, shuffle="bit",
        version=3)
    add("byte shuffle, large, short tail", ds["walk"][:big + 1001], 2, big, shuffle="byte")
    add("no shuffle, large, short tail", ds["words"][:big + 1001], 2, big)
    add("empty", b"", 4, 256)
    # bytes behind the Adler-32: uncompress ignores them, and so does the device
    d = ds["words"][:3000]
    out.append(("rubbish behind the trailer", d,
                one_stream(zlib.compress(d, 6) + b"\x00\xffzh\x07", len(d))))
    # the Adler-32 at the sizes where its sums wrap or a lane's share changes
    rng = np.random.default_rng(65521)
    for n in ADLER_SIZES:
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        add(f"adler, {n} random bytes, level 0", d, 1, n, zfn=deflate(0), keep=True)
        add(f"adler, {n} bytes of 0xff, level 1", b"\xff" * n, 1, n, zfn=deflate(1), keep=True)
    add("adler, 1 MiB of 0xff", b"\xff" * (1 << 20), 1, 1 << 20, zfn=deflate(1))
    return out


def host_routed():
    """[(label, data, frame)]: valid blosc-zlib frames the flag still leaves to the host."""
    ds = datasets()
    d = ds["words"][:6000]
    out = [(f"wbits {w}", d, frame(d, 1, len(d), deflate(6, wbits=w))) for w in range(9, 15)]

    def small_window(b, s, c, part):
        return deflate(6, wbits=12)(part) if s == 2 else c
    out.append(("one stream of a split block with wbits 12", ds["quad"],
                frame(ds["quad"], 4, 8192, deflate(6), shuffle="byte", split=True,
                      edit=small_window)))
    return out


def mixed_batch():
    """([frame], {flags: [where]}): LZ4, memcpyed, zlib and zstd frames."""
    frames = zi.mixed_batch()[0][:4]
    return frames, {0: [0, 2, 1, 1], ZSTD_FLAG: [0, 2, 1, 0], FLAG: [0, 2, 0, 1],
                    FLAG | ZSTD_FLAG: [0, 2, 0, 0]}


# ---- corrupt frames -----------------------------------------------------------------------------
def corrupt():
    """[(label, frame, where with the flag)]: each is rejected by zh_blosc_decompress (asserted by
    the CPU test before the GPU test relies on it).  where None: the plan itself refuses."""
    ds = datasets()
    d = ds["words"][:20000]
    good = frame(d, 1, len(d), deflate(6))
    (s,) = zlib_streams(good)
    base = 16 + 4 + 4                      # header, one block start, the stream's csize
    assert good[base:] == s and (s[2] >> 1) & 3 == 2    # the stream opens with a dynamic block
    out = []
    fl = bytearray(good)
    fl[-2] ^= 0x01
    out.append(("flipped Adler byte", bytes(fl), 0))
    fl = bytearray(good)
    fl[base + len(s) // 2] ^= 0x10
    out.append(("flipped bit in a dynamic block", bytes(fl), 0))
    # the last byte of the stream is gone: with its csize kept the chain runs past the frame;
    # with csize fixed up as well the trailer is three bytes
    cut = bytearray(good[:-1])
    cut[12:16] = struct.pack("<I", len(cut))
    out.append(("truncated by one byte", bytes(cut), 1))
    cut[20:24] = struct.pack("<i", len(s) - 1)
    out.append(("truncated by one byte, csize too", bytes(cut), 0))
    for label, n in (("decodes to neb - 1", 99), ("decodes to neb + 1", 101)):
        c = zlib.compress(d[:n], 6)
        assert len(c) != 100               # a payload of the raw size would be a raw stream
        out.append((label, one_stream(c, 100), 0))
    # a fixed block whose first match (3 bytes at distance 2) follows a single literal
    ops = [ord("a"), (3, 2)]
    w = Bits()
    fixed_block(w, ops, True)
    out.append(("distance before the stream",
                one_stream(b"\x78\x01" + w.bytes() + struct.pack(">I", 1), 4), 0))
    bad = bytearray(good)
    bad[base + 1] ^= 0x01                  # FLG: the check bits no longer divide by 31
    out.append(("wrong header check bits", bytes(bad), 1))
    bad = bytearray(good)
    bad[base:base + 2] = b"\x78\xbb"       # FDICT set, check bits right
    assert (0x78bb % 31, 0xbb & 0x20) == (0, 0x20)
    out.append(("preset dictionary", bytes(bad), 1))
    return out


def mutation_inputs():
    """The matrix frames whose streams the checker mutates: all but the large ones."""
    return [f for _, d, f in matrix() if 0 < len(d) <= 64 << 10]
