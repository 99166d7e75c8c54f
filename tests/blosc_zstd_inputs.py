"""Frames for the device decode of blosc frames with zstd streams (test_blosc_zstd_host.py on the
CPU, test_gpu_blosc_zstd.py on the device): blosc1 frames assembled by blosc_frames.frame_streams
over zstd stream payloads from two independent sources (libzstd through pyarrow at levels 1 and 5,
where pyarrow exists, and the library's own zh_zstd_compress without a checksum), the valid
matrix, a mixed batch and a fixed list of corrupt frames.  Every expected value is
zh_blosc_decompress on the same frame (blosc_frames.host_decode) and the input the frame was made
from.  Test infrastructure only; nothing here needs a device."""
import functools
import struct
import zlib

import numpy as np

import blosc_frames as bf
import spec_blosc as sb
from zarrhip import _lib

FLAG = 1               # ZH_BLOSC_ZSTD_DEVICE
KZSTD = 3              # zh_bs::kZstd, the method column of the stream table
LDS_BLOCK = 64 << 10   # kLdsBlock of zh_blosc_kernels.hip
MAGIC = b"\x28\xb5\x2f\xfd"

try:
    import pyarrow as _pa
except ImportError:      # the library's own compressor remains
    _pa = None


def have_libzstd():
    return _pa is not None


def libzstd(level):
    return lambda b: _pa.Codec("zstd", compression_level=level).compress(bytes(b), asbytes=True)


def own(b):
    return _lib.zstd_compress(bytes(b), False, 0)


def sources():
    """[(name, bytes -> one zstd frame)]: the payload sources of the matrix."""
    out = [("own", own)]
    if have_libzstd():
        out += [("libzstd1", libzstd(1)), ("libzstd5", libzstd(5))]
    return out


# ---- frames ---------------------------------------------------------------------------------------
def shuffled_streams(data, typesize, blocksize, shuffle="none", split=False, version=2):
    """[[stream bytes, ...] per block]: the blocks of `data`, shuffled (none / byte / bit) and cut
    into their streams as c-blosc does (a leftover block is never split)."""
    data = bytes(data)
    out = []
    for k in range(-(-len(data) // blocksize) if data else 0):
        blk = data[k * blocksize:(k + 1) * blocksize]
        bs = len(blk)
        if shuffle == "byte" and typesize > 1:
            ne = bs // typesize
            a = np.frombuffer(blk[:ne * typesize], np.uint8).reshape(ne, typesize).T.ravel()
            blk = a.tobytes() + blk[ne * typesize:]
        elif shuffle == "bit":
            blk = sb.bit_shuffle(blk, typesize, version)
        nsplit = typesize if split and bs == blocksize else 1
        neb = bs // nsplit
        out.append([blk[s * neb:(s + 1) * neb] for s in range(nsplit)])
    return out


def frame(data, typesize, blocksize, zfn, shuffle="none", split=False, version=2, edit=None):
    """A blosc1 frame with compressor code 4 whose streams are `zfn`'s zstd frames (or stored raw
    where that is not smaller, as c-blosc does).  `edit(block, stream, payload, raw)` may replace
    a payload."""
    blocks = []
    for b, parts in enumerate(shuffled_streams(data, typesize, blocksize, shuffle, split, version)):
        row = []
        for s, part in enumerate(parts):
            c = zfn(part)
            if len(c) >= len(part):
                c = part
            if edit is not None:
                c = edit(b, s, c, part)
            row.append(c)
        blocks.append(row)
    return bf.frame_streams(blocks, len(data), typesize, blocksize, "zstd",
                            shuffle=shuffle == "byte", split=split, bitshuffle=shuffle == "bit",
                            version=version)


def zstd_streams(f):
    """The payloads of the kZstd streams of a frame (by the flagged stream table)."""
    return [bytes(f[r[1]:r[1] + r[2]]) for r in _lib.blosc_streams(f, FLAG)
            if r[0] == 1 and r[5] == KZSTD]


# ---- data -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def datasets():
    rng = np.random.default_rng(20241021)
    skew = rng.choice(np.arange(256, dtype=np.uint8), 160 << 10,
                      p=np.r_[np.full(16, 0.05), np.full(240, 0.2 / 240)]).tobytes()
    ramp = ((np.arange(48 << 10) // 3 + rng.integers(0, 2, 48 << 10)) % 65536).astype("<u2")
    walk = np.cumsum(rng.integers(-3, 4, 80 << 10)).astype("<i2").tobytes()
    vocab = [b"zarr", b"chunk", b"shard", b"codec", b"the", b"of", b"array", b"index", b"bytes"]
    words = b" ".join(vocab[i] for i in rng.integers(0, 9, 40000))
    # elements of 4 bytes: byte 0 random (its stream is stored raw), byte 1 constant, 2 and 3 a ramp
    n = 2048
    quad = np.stack([rng.integers(0, 256, n), np.full(n, 7), np.arange(n) & 255,
                     np.arange(n) >> 8], axis=1).astype(np.uint8).tobytes()
    oct_ = (np.arange(1024, dtype="<u8") * 0x0101010101 + rng.integers(0, 4, 1024)
            .astype("<u8")).tobytes()
    return {"skew": skew, "ramp": ramp.tobytes(), "walk": walk, "words": words, "quad": quad,
            "oct": oct_}


@functools.lru_cache(maxsize=None)
def matrix():
    """[(label, data, frame)]: every frame is one the flag sends to the device (where == 0)."""
    ds = datasets()
    big = LDS_BLOCK + 512
    out = []
    for name, z in sources():
        def add(label, data, *a, **kw):
            out.append((f"{label} [{name}]", bytes(data), frame(data, *a, zfn=z, **kw)))
        add("single small block", ds["words"][:4096], 1, 4096)
        add("byte shuffle, small", ds["walk"][:32 << 10], 4, 32 << 10, shuffle="byte")
        add("byte shuffle, large", ds["walk"][:96 << 10], 2, big, shuffle="byte")
        add("byte shuffle, large, short tail", ds["walk"][:big + 1001], 2, big, shuffle="byte")
        add("no shuffle, large, short tail", ds["words"][:big + 1001], 2, big)
        add("split, raw and constant streams", ds["quad"], 4, 8192, shuffle="byte", split=True)
        # the constant stream as one RLE block (the compressors above write a match instead)
        add("split, raw stream and RLE block", ds["quad"], 4, 8192, shuffle="byte", split=True,
            edit=lambda b, s, c, part: zframe_of([(1, part[:1], len(part))], len(part))
            if s == 1 else c)
        add("split, 8 streams", ds["oct"], 8, 8192, shuffle="byte", split=True)
        add("split, 8 streams, 2 blocks and a tail", ds["oct"] * 2 + ds["oct"][:1004], 8, 8192,
            shuffle="byte", split=True)
        add("bit shuffle v2, 1003 elements", ds["walk"][:4 * 1003], 4, 4 * 1003, shuffle="bit")
        add("bit shuffle v3, 1003 elements", ds["walk"][:4 * 1003], 4, 4 * 1003, shuffle="bit",
            version=3)
        add("bit shuffle v2, 1024 elements", ds["walk"][:4096], 4, 4096, shuffle="bit")
        add("skewed bytes", ds["skew"][:16 << 10], 1, 16 << 10)
        add("uint16 ramp", ds["ramp"][:32 << 10], 2, 32 << 10, shuffle="byte")
        if name != "libzstd1":
            add("160 KiB in one stream", ds["skew"][:100 << 10] + ds["words"][:60 << 10], 1,
                160 << 10)
        add("empty", b"", 4, 256)
    return out


# ---- zstd frames built from RFC 8878 ----------------------------------------------------------------
def zframe_of(blocks, size, checksum=None):
    """A single-segment zstd frame with a 4-byte content size over (type, payload, block size)."""
    out = MAGIC + bytes([0xA0 | (4 if checksum is not None else 0)]) + struct.pack("<I", size)
    for k, (btype, payload, bsz) in enumerate(blocks):
        bh = (bsz << 3) | (btype << 1) | (1 if k + 1 == len(blocks) else 0)
        out += struct.pack("<I", bh)[:3] + payload
    return out + (struct.pack("<I", checksum) if checksum is not None else b"")


def one_stream(payload, rawsize, typesize=1):
    return bf.frame_streams([[payload]], rawsize, typesize, max(rawsize, 1), "zstd")


def host_routed():
    """[(label, data, frame)]: valid blosc-zstd frames the flag still leaves to the host."""
    ds = datasets()
    d = ds["words"][:6000]
    csum = _lib.zstd_compress(d, True, 0)
    a, b = own(d[:3000]), own(d[3000:])
    skip = b"\x50\x2a\x4d\x18" + struct.pack("<I", 5) + b"hello"
    raw = zframe_of([(0, d[:100], 100)], 100)
    nofcs = MAGIC + b"\x00\x58" + raw[9:]      # no content size; a window descriptor instead
    return [("checksum", d, one_stream(csum, len(d))),
            ("concatenated", d, one_stream(a + b, len(d))),
            ("skippable then frame", d, one_stream(skip + own(d), len(d))),
            ("no content size", d[:100], one_stream(nofcs, 100))]


def mixed_batch():
    """([frame], [where with the flag], [where without]): LZ4, memcpyed, zlib, a zstd device
    frame, a zstd frame with one checksummed stream (host)."""
    ds = datasets()
    data = np.arange(2000, dtype="<i4").tobytes()
    memc = struct.pack("<BBBBIII", 2, 1, 0x02, 1, 64, 64, 80) + bytes(range(64))
    zl = bf.frame_streams([[zlib.compress(data, 6)]], len(data), 4, len(data), "zlib")

    def with_checksum(b, s, c, part):
        return _lib.zstd_compress(part, True, 0) if s == 2 else c
    frames = [sb.frame(data, 4, 4096, "lz4"), memc, zl,
              frame(ds["walk"][:8192], 4, 8192, own, shuffle="byte", split=True),
              frame(ds["walk"][:8192], 4, 8192, own, shuffle="byte", split=True,
                    edit=with_checksum)]
    return frames, [0, 2, 1, 0, 1], [0, 2, 1, 1, 1]


# ---- corrupt frames -----------------------------------------------------------------------------
def flip_position(stream):
    """A byte of the last block's sequence section: the bitstream is read backwards from the
    block's end, so the byte before the last one holds the first states and extra bits."""
    return len(stream) - 2


def corrupt():
    """[(label, frame, where with the flag)]: each is rejected by zh_blosc_decompress (asserted by
    the CPU test before the GPU test relies on it)."""
    ds = datasets()
    d = ds["words"][:20000]
    good = frame(d, 1, len(d), own)
    (s,) = zstd_streams(good)
    base = 16 + 4 + 4                      # header, one block start, the stream's csize
    assert good[base:] == s
    out = []
    # the last byte of the stream is gone, its csize is not: the chain runs past the frame
    cut = bytearray(good[:-1])
    out.append(("truncated, cbytes kept", bytes(cut), None))     # the plan itself refuses
    cut[12:16] = struct.pack("<I", len(cut))
    out.append(("truncated by one byte", bytes(cut), 1))
    # one bit of the sequence bitstream
    fl = bytearray(good)
    fl[base + flip_position(s)] ^= 0x08
    out.append(("flipped sequence bit", bytes(fl), 0))
    # a content size one short of the stream's raw size: the host's, and it fails there
    short = zframe_of([(0, d[:99], 99)], 99)
    out.append(("content size neb - 1", one_stream(short, 100), 1))
    # no literals (a raw literals header of size 0) and one sequence: a 3-byte match whose
    # offset (repeat offset 2, which is 4) reaches before the first byte of the stream
    blk = b"\x00" + bytes([1]) + bytes([0x54, 0, 0, 0]) + b"\x01"
    before = zframe_of([(2, blk, len(blk))], 3)
    out.append(("offset before the stream", one_stream(before, 3), 0))
    # the same after 16 bytes of history: offset 4 is fine, the frame is valid -- and a second
    # sequence count that the literals cannot serve
    hist = b"abcdefghijklmnop"
    blk2 = bytes([(2 << 3) | 1, ord("Z")]) + bytes([5]) + bytes([0x54, 2, 0, 1]) + b"\x01"
    past = zframe_of([(0, hist, 16), (2, blk2, len(blk2))], 46)
    out.append(("sequences past the literals", one_stream(past, 46), 0))
    return out
