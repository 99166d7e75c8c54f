"""The expected frames of the blosc writer with zlib streams (test_blosc_zlib_encode_host.py on the
CPU, test_gpu_blosc_zlib_encode.py on the device), built here without the writer under test: the
layout rule of the LZ4 writer restated, blosc_zlib_inputs.frame around the library's gzip member
writer per stream (zh_gzip_compress with 16 KiB blocks, its 10 header and 8 trailer bytes replaced
by 78 01 and Python's Adler-32), and the MEMCPYED fallback.  Test infrastructure only; nothing
here needs a device."""
import functools
import struct
import zlib

import numpy as np

import blosc_enc_inputs as bi
import blosc_zlib_inputs as bz
from zarrhip import _lib

FLAG = 4                  # ZH_BLOSC_ENC_ZLIB
FLAG_DYN = 12             # ZH_BLOSC_ENC_ZLIB | ZH_BLOSC_ENC_DYNAMIC
FLAGS = (FLAG, FLAG_DYN)
BAD_FLAGS = (5, 8, 9, 13, 16, 0x80000000)
PIECE = 16 << 10          # zh_gz::kDefaultBlock: one DEFLATE segment per piece of a stream
DEFAULT_BLOCK = 16 << 10
SHUFFLE_NAME = {0: "none", 1: "byte", 2: "bit"}
# payload names of blosc_enc_inputs.payloads that must come out compressed / MEMCPYED
# (the image as it is has few repeats of four bytes and its literals cost eight bits or more
# under the fixed codes: only the dynamic form shrinks it under every typesize and shuffle)
COMPRESSED = ("zeros", "block+leftover", "127el", "128el", "128el+3")
COMPRESSED_DYNAMIC = COMPRESSED + ("img",)
MEMCPYED = ("random", "len0", "len1", "len12", "len13")
CAPACITIES = (16 << 10, (16 << 10) + 4, 32 << 10, (32 << 10) + 4, 64 << 10)


def layout(n, ts, sh, bs):
    """(effective block size, split) of a frame of n bytes: the default is 16 KiB, the block is
    clamped to 64 KiB and to the frame, then cut to whole elements; streams are split under the
    byte shuffle when typesize <= 16 and the block holds 128 elements or more."""
    b = min(bs if bs > 0 else DEFAULT_BLOCK, bi.BLOCK, n)
    if b > ts:
        b = b // ts * ts
    return b, sh == 1 and ts <= 16 and b // ts >= 128


def zlib_stream(dynamic):
    """zfn of blosc_zlib_inputs.frame: the payload the format fixes for a stream."""
    def run(b):
        b = bytes(b)
        return (b"\x78\x01" + _lib.gzip_compress(b, PIECE, dynamic)[10:-8] +
                zlib.adler32(b).to_bytes(4, "big"))
    return run


def segments(stream, dynamic):
    """The segments of a stream's payload, one per 16 KiB piece (each piece is compressed on its
    own, so a piece's segment is what the member writer gives for the piece alone)."""
    stream = bytes(stream)
    segs = [_lib.gzip_compress(stream[o:o + PIECE], PIECE, dynamic)[10:-10]
            for o in range(0, len(stream), PIECE)]
    assert b"".join(segs) + b"\x03\x00" == _lib.gzip_compress(stream, PIECE, dynamic)[10:-8]
    return segs


def segment_forms(stream, dynamic):
    """{"stored", "fixed", "dynamic"} over the segments of a stream (BTYPE of the segment's first
    byte: every segment starts on a byte boundary with BFINAL 0)."""
    return {{0: "stored", 2: "fixed", 4: "dynamic"}[s[0] & 7] for s in segments(stream, dynamic)}


def expected(data, ts, sh, bs, flags=FLAG):
    """The frame the format section fixes for (data, typesize, shuffle, block size, flags)."""
    data = bytes(data)
    n = len(data)
    b, split = layout(n, ts, sh, bs)
    fl = (3 << 5) | (0x01 if sh == 1 else 0) | (0x04 if sh == 2 else 0) | (0 if split else 0x10)
    f = None
    if n:
        f = bz.frame(data, ts, b, zfn=zlib_stream(flags == FLAG_DYN), shuffle=SHUFFLE_NAME[sh],
                     split=split)
        assert f[2] == fl
    if f is None or len(f) > n + 16:
        return struct.pack("<BBBBIII", 2, 1, (fl & ~0x10) | 0x02, ts, n, b, n + 16) + data
    return f


def raw_streams(data, ts, sh, bs):
    """The shuffled streams of the frame of (data, ts, sh, bs), in stored order."""
    b, split = layout(len(data), ts, sh, bs)
    return [s for blk in bz.shuffled_streams(bytes(data), ts, b, SHUFFLE_NAME[sh], split)
            for s in blk]


@functools.lru_cache(maxsize=None)
def matrix(flags=FLAG):
    """[(label, data, typesize, shuffle, blocksize, expected frame)] over blosc_enc_inputs."""
    return [(label, data, ts, sh, bs, expected(data, ts, sh, bs, flags))
            for label, data, ts, sh, bs in bi.matrix()]


def name_of(label):
    return label.split("-ts")[0]


@functools.lru_cache(maxsize=None)
def multi_segment():
    """[(label, data, typesize, shuffle, blocksize)]: unsplit blocks (stream = block) of more than
    one 16 KiB piece, the Adler-32's largest sums, stored and fixed segments in one stream, and
    the stream lengths at which the Adler-32 changes its path."""
    rng = np.random.default_rng(41)
    noise = rng.integers(0, 256, 16 << 10, dtype=np.uint8).tobytes()
    text = bytes((np.arange(200001) // 3 % 7 + np.arange(200001) % 5).astype(np.uint8))
    out = []
    for bs in (16 << 10, (16 << 10) + 4, 32 << 10, 64 << 10):
        out.append((f"text-bs{bs}-sh0", text[:3 * bs + 77], 1, 0, bs))
        out.append((f"text-bs{bs}-sh2", text[:2 * bs + 16], 4, 2, bs))
        out.append((f"img-bs{bs}-sh2", bi.img(), 2, 2, bs))
    out.append(("ff-64k", b"\xff" * (64 << 10), 1, 0, 64 << 10))
    out.append(("stored+fixed", noise + bytes(48 << 10), 1, 0, 64 << 10))
    out.append(("fixed+stored", bytes(48 << 10) + noise, 1, 0, 64 << 10))
    for n in (k for k in bz.ADLER_SIZES if k < 64 << 10):
        out.append((f"adler-{n}", text[:n], 1, 0, 64 << 10))
        out.append((f"adler-ff-{n}", b"\xff" * n, 1, 0, 64 << 10))
    return out
