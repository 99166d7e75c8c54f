"""Shared inputs of the zstd device-decode tests (test_zstd_batch_host.py, test_gpu_zstd_decode.py):
seeded data compressed by libzstd (through pyarrow) at several levels, the library's own frames,
the OME v0.5 fixtures, frames built here from RFC 8878 for what libzstd does not readily emit
(RLE literals, tables in RLE mode, the 3-byte sequence count), frames the device route hands to
the host, a fixed list of corrupt frames, and an independent walk over a frame's block headers.
Nothing here needs a device."""
import functools
import os
import struct

import numpy as np

from helpers import GOLDEN
from independent_codecs import pa, zstd_decode
from zarrhip import _abi as A
from zarrhip import _lib

MAGIC = b"\x28\xb5\x2f\xfd"
LEVELS = (-5, 1, 3, 9, 19)
OME_ZSTD = ["v0.5/0/c/0/0/0/0/0", "v0.5/0/c/0/1/0/0/0", "v0.5/1/c/0/0/0/0/0", "v0.5/1/c/0/1/0/0/0",
            "v0.5/labels/nuclei/0/c/0/0/0", "v0.5_hcs/A/1/0/0/c/0/0/0/0/0",
            "v0.5_hcs/A/1/0/0/c/0/1/0/0/0"]


def libzstd(data, level):
    return pa.Codec("zstd", compression_level=level).compress(bytes(data), asbytes=True)


@functools.lru_cache(maxsize=None)
def datasets():
    """name -> bytes, all seeded."""
    rng = np.random.default_rng(20240607)
    vocab = [b"zarr", b"chunk", b"shard", b"codec", b"the", b"of", b"array", b"index", b"bytes",
             b"wave", b"lane", b"frame", b"block"]
    words = b" ".join(vocab[i] for i in rng.integers(0, 13, 60000))
    t = rng.integers(1, 5000, (15, 16), dtype=np.uint16)
    labels = np.repeat(np.repeat(t, 32, axis=0), 31, axis=1).astype("<u2").tobytes()
    noise4 = rng.integers(0, 16, 300000, dtype=np.uint8).tobytes()
    text = (b"A zstd frame is a header, blocks and an optional checksum; a compressed block is a "
            b"literals section and a sequences section. ") * 6
    walk = np.cumsum(rng.integers(-3, 4, 200000)).astype("<i2").tobytes()
    runs = b"".join(bytes([int(v)]) * int(n) for v, n in
                    zip(rng.integers(0, 256, 2000), rng.integers(30, 60, 2000)))
    return {"words": words, "labels": labels, "noise4": noise4, "zeros": bytes(400000),
            "text": text[:700], "walk": walk, "runs": runs}


# ---- frames built from the specification --------------------------------------------------------
def frame_of(blocks, size, checksum=None):
    """A single-segment frame with a 4-byte content size over (type, payload, block size)."""
    out = MAGIC + bytes([0xA0 | (4 if checksum is not None else 0)]) + struct.pack("<I", size)
    for k, (btype, payload, bsz) in enumerate(blocks):
        bh = (bsz << 3) | (btype << 1) | (1 if k + 1 == len(blocks) else 0)
        out += struct.pack("<I", bh)[:3] + payload
    return out + (struct.pack("<I", checksum) if checksum is not None else b"")


def rle_tables_block(lit_header, nseq_bytes, ll=2, of=0, ml=1, stream=b"\x01", modes=0x54):
    """A compressed block: literals header (and payload) as given, the sequence count, the three
    tables in RLE mode (one code each, states of 0 bits) and the bitstream.  With codes that
    carry no extra bits the stream is the end marker alone."""
    return lit_header + nseq_bytes + bytes([modes, ll, of, ml]) + stream


HISTORY = b"abcdefghijklmnop"


def hand_rle(checksum=False):
    """RLE literals (12 x 'Z') and 5 sequences of 2 literals + a 4-byte match at repeat offset 1."""
    blk = rle_tables_block(bytes([(12 << 3) | 1, ord("Z")]), bytes([5]))
    data = HISTORY + b"ZZZZZZ" * 5 + b"ZZ"
    return data, frame_of([(0, HISTORY, len(HISTORY)), (2, blk, len(blk))], len(data),
                          xxh32(data) if checksum else None)


def hand_count3(nseq=0x7F00 + 3):
    """The 3-byte sequence count: nseq sequences of no literals and a 3-byte match; with ll == 0
    offset code 0 names repeat offset 2, so the offsets alternate 4, 1, 4, 1, ..."""
    blk = rle_tables_block(b"\x00", b"\xff" + struct.pack("<H", nseq - 0x7F00), ll=0, of=0, ml=0)
    data = bytearray(HISTORY)
    rep = [1, 4, 8]
    for _ in range(nseq):
        off = rep[1]
        rep[1], rep[0] = rep[0], off
        for _ in range(3):
            data.append(data[-off])
    return bytes(data), frame_of([(0, HISTORY, len(HISTORY)), (2, blk, len(blk))], len(data))


def hand_blocks():
    """An RLE block, a raw block and a compressed block with no sequences (raw literals)."""
    blk = bytes([5 << 3]) + b"hello" + b"\x00"
    data = b"\x07" * 1000 + b"raw!" + b"hello"
    return data, frame_of([(1, b"\x07", 1000), (0, b"raw!", 4), (2, blk, len(blk))], len(data))


def xxh32(data):
    return _lib.lib().zh_xxh64(bytes(data), len(data), 0) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def valid():
    """[(label, data, frame)]: every frame is one the device decodes (where == 0)."""
    out = []
    for name, data in datasets().items():
        for lv in LEVELS:
            out.append((f"libzstd {name} L{lv}", data, libzstd(data, lv)))
    ds = datasets()
    for name in ("labels", "walk", "text"):
        for bs in (1 << 10, 16 << 10, 64 << 10):
            for cs in (True, False):
                d = ds[name][:150000]
                out.append((f"own {name} {bs} {cs}", d, _lib.zstd_compress(d, cs, bs)))
    for key in OME_ZSTD:
        f = open(os.path.join(GOLDEN, "ome_zstd", *key.split("/")), "rb").read()
        out.append((f"ome {key}", host_decode(f)[1], f))
    out.append(("empty", b"", _lib.zstd_compress(b"", True, 0)))
    out.append(("empty hand", b"", frame_of([(0, b"", 0)], 0)))
    for label, (data, frame) in (("hand rle", hand_rle()), ("hand count3", hand_count3()),
                                 ("hand blocks", hand_blocks())):
        out.append((label, data, frame))
    out.append(("hand rle checksum",) + hand_rle(True))
    return out


def host_routed():
    """[(label, data, frame)]: valid, but planned where == 1."""
    ds = datasets()
    a, b = libzstd(ds["text"], 3), libzstd(ds["walk"][:5000], 1)
    skip = b"\x50\x2a\x4d\x18" + struct.pack("<I", 5) + b"hello"
    d, f = hand_blocks()
    nofcs = MAGIC + b"\x00\x58" + f[9:]        # no content size; a window descriptor instead
    return [("concatenated", ds["text"] + ds["walk"][:5000], a + b),
            ("skippable then frame", ds["text"], skip + a),
            ("frame then skippable", ds["text"], a + skip),
            ("no content size", d, nofcs)]


def impossible_size():
    """Raw blocks of 10 bytes under a content size of 11: the size query says 11, the decode
    fails with the host's text."""
    return frame_of([(0, b"0123456789", 10)], 11)


def corrupt():
    """[(label, frame)]: the fixed list of corrupt frames; every one is rejected by
    zh_zstd_decompress (asserted by the CPU test before the GPU test relies on it)."""
    lits = bytes([(12 << 3) | 1, ord("Z")])
    good = rle_tables_block(lits, bytes([5]))

    def one(blk, size=48, hist=True):
        blocks = ([(0, HISTORY, 16)] if hist else []) + [(2, blk, len(blk))]
        return frame_of(blocks, size)
    # a Huffman tree of two direct weights (1, 1: the implied third weight is 2), then four
    # bytes where the six of a jump table should be
    tree = bytes([129, 0x11])
    jump = struct.pack("<I", 2 | (1 << 2) | (8 << 4) | (6 << 14))[:3] + tree + b"\x01\x00\x01\x00"
    # direct weights 1 and 3: 1 + 4 = 5 leaves 3, no power of two
    badw = struct.pack("<I", 2 | (0 << 2) | (8 << 4) | (3 << 14))[:3] + bytes([129, 0x13, 0x01])
    # an LL description (accuracy 5) of one zero probability and "three more zeros" until the
    # symbols run out with all 32 cells unassigned.  (A probability larger than what remains
    # cannot be written: the field's width follows what remains.)
    fse = lits + bytes([5, 0x94, 0x10, 0xFE]) + b"\xff" * 8 + bytes([0, 1, 0x01])
    ds = datasets()
    ck = bytearray(_lib.zstd_compress(ds["walk"][:20000], True, 16 << 10))
    ck[-1] ^= 0x40
    mid = bytearray(libzstd(ds["words"], 3))
    mid[len(mid) // 2] ^= 0x10
    big = frame_of([(0, bytes((128 << 10) + 1), (128 << 10) + 1)], (128 << 10) + 1)
    return [
        ("bad huffman weight sum", one(badw + b"\x00")),
        ("fse probabilities do not sum", one(fse)),
        ("sequence code out of range", one(rle_tables_block(lits, bytes([5]), ml=53))),
        ("offset before the frame", one(rle_tables_block(b"\x00", bytes([1]), ll=0, ml=0), 3,
                                        hist=False)),
        ("literals overrun", one(rle_tables_block(bytes([(9 << 3) | 1, ord("Z")]), bytes([5])), 45)),
        ("bitstream not consumed", one(rle_tables_block(lits, bytes([5]), stream=b"\x03"))),
        ("treeless without a table", one(struct.pack("<I", 3 | (8 << 4) | (2 << 14))[:3] +
                                         b"\x01\x01\x00")),
        ("repeat without a table", one(lits + bytes([5, 0xFC, 0x01]))),
        ("truncated jump table", one(jump + b"\x00")),
        ("block larger than 128 KiB", big),
        ("checksum mismatch", bytes(ck)),
        ("reserved block type", frame_of([(3, b"abc", 3)], 3)),
        ("flipped bit mid-frame", bytes(mid)),
        ("content size mismatch", one(good, 47)),
        ("reserved mode bits", one(rle_tables_block(lits, bytes([5]), modes=0x55))),
        ("no end marker", one(rle_tables_block(lits, bytes([5]), stream=b"\x00"))),
    ]


def mutations(n=1200, seed=77):
    """n seeded single-byte, truncation and bit-flip mutations of the smaller valid frames."""
    rng = np.random.default_rng(seed)
    pool = [f for _, _, f in valid() if 0 < len(f) <= 40000]
    out = []
    for k in range(n):
        f = bytearray(pool[int(rng.integers(0, len(pool)))])
        kind = k % 3
        pos = int(rng.integers(0, len(f)))
        if kind == 0:
            f[pos] = int(rng.integers(0, 256))
        elif kind == 1:
            f = f[:pos]
        else:
            f[pos] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(f))
    return out


# ---- the host decoder and an independent walk ---------------------------------------------------
def size_query(frame):
    """zh_zstd_decompress with no destination: (status, nbytes, message)."""
    import ctypes as C
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    b = bytes(frame)
    st = _lib.lib().zh_zstd_decompress(b, len(b), None, 0, C.byref(n), err, 256)
    return st, n.value, err.value.decode()


def host_decode(frame):
    """zh_zstd_decompress: (status, bytes, message)."""
    import ctypes as C
    st, nb, msg = size_query(frame)
    if st != A.ZH_OK:
        return st, b"", msg
    out = C.create_string_buffer(max(1, nb))
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    b = bytes(frame)
    st = _lib.lib().zh_zstd_decompress(b, len(b), out, nb, C.byref(n), err, 256)
    return st, out.raw[:n.value] if st == A.ZH_OK else b"", err.value.decode()


def independent_blocks(frame):
    """One row per block of a single frame, read from RFC 8878 here: (type, stored size, decoded
    size or -1, literals type, streams, regen, nseq, LL mode, OF mode, ML mode); -1 where a
    field does not apply."""
    assert frame[:4] == MAGIC
    fhd = frame[4]
    single = (fhd >> 5) & 1
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    p += {0: 1 if single else 0, 1: 2, 2: 4, 3: 8}[fhd >> 6]
    rows = []
    while True:
        bh = int.from_bytes(frame[p:p + 3], "little")
        p += 3
        last, btype, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
        if btype != 2:
            rows.append((btype, 1 if btype == 1 else bsz, bsz) + (-1,) * 7)
            p += 1 if btype == 1 else bsz
        else:
            b = frame[p:p + bsz]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt < 2:
                hs = (1, 2, 1, 3)[sf]
                regen = b[0] >> 3 if hs == 1 else int.from_bytes(b[:hs], "little") >> 4
                streams, sec = 0, hs + (regen if lt == 0 else 1)
            else:
                hs, nb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
                h = int.from_bytes(b[:hs], "little")
                regen, csz = (h >> 4) & ((1 << nb) - 1), (h >> (4 + nb)) & ((1 << nb) - 1)
                streams, sec = (1 if sf == 0 else 4), hs + csz
            q = b[sec:]
            if q[0] < 128:
                nseq, q = q[0], q[1:]
            elif q[0] < 255:
                nseq, q = ((q[0] - 128) << 8) + q[1], q[2:]
            else:
                nseq, q = q[1] + (q[2] << 8) + 0x7F00, q[3:]
            modes = (q[0] >> 6, (q[0] >> 4) & 3, (q[0] >> 2) & 3) if nseq else (-1, -1, -1)
            rows.append((2, bsz, -1, lt, streams, regen, nseq) + modes)
            p += bsz
        if last:
            return rows


def check_with_libzstd(data, frame):
    assert zstd_decode(frame, len(data)) == data
