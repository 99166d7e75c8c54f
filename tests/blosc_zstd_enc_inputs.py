"""The expected frames of the blosc writer with zstd streams (test_blosc_zstd_encode_host.py on
the CPU, test_gpu_blosc_zstd_encode.py on the device), built here without the writer under test:
the layout rule of the LZ4 writer restated, blosc_zstd_inputs.frame around the library's plain zstd
writer (zh_zstd_compress, no checksum, 64 KiB blocks) per stream, and the MEMCPYED fallback.  Test
infrastructure only; nothing here needs a device."""
import functools
import struct

import blosc_enc_inputs as bi
import blosc_zstd_inputs as bz
from zarrhip import _lib

FLAG = 1                  # ZH_BLOSC_ENC_ZSTD
DEFAULT_BLOCK = 16 << 10
SHUFFLE_NAME = {0: "none", 1: "byte", 2: "bit"}
# payload names of blosc_enc_inputs.payloads that must come out compressed / MEMCPYED
COMPRESSED = ("img", "zeros", "block+leftover", "127el", "128el", "128el+3")
MEMCPYED = ("random", "len0", "len1", "len12", "len13")


def layout(n, ts, sh, bs):
    """(effective block size, split) of a frame of n bytes: the default is 16 KiB, the block is
    clamped to 64 KiB and to the frame, then cut to whole elements; streams are split under the
    byte shuffle when typesize <= 16 and the block holds 128 elements or more."""
    b = min(bs if bs > 0 else DEFAULT_BLOCK, bi.BLOCK, n)
    if b > ts:
        b = b // ts * ts
    return b, sh == 1 and ts <= 16 and b // ts >= 128


def zstd_stream(b):
    return _lib.zstd_compress(bytes(b), False, 64 << 10)


def expected(data, ts, sh, bs):
    """The frame the format section fixes for (data, typesize, shuffle, block size)."""
    data = bytes(data)
    n = len(data)
    b, split = layout(n, ts, sh, bs)
    flags = (4 << 5) | (0x01 if sh == 1 else 0) | (0x04 if sh == 2 else 0) | (0 if split else 0x10)
    f = None
    if n:
        f = bz.frame(data, ts, b, zfn=zstd_stream, shuffle=SHUFFLE_NAME[sh], split=split)
        assert f[2] == flags
    if f is None or len(f) > n + 16:
        return struct.pack("<BBBBIII", 2, 1, (flags & ~0x10) | 0x02, ts, n, b, n + 16) + data
    return f


@functools.lru_cache(maxsize=None)
def matrix():
    """[(label, data, typesize, shuffle, blocksize, expected frame)] over blosc_enc_inputs."""
    return [(label, data, ts, sh, bs, expected(data, ts, sh, bs))
            for label, data, ts, sh, bs in bi.matrix()]


def name_of(label):
    return label.split("-ts")[0]
