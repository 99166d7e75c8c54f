"""Frames for the batched blosc decode tests (test_blosc_batch_host.py on the CPU,
test_gpu_blosc.py on the device): token emitters for hand-made LZ4 / BloscLZ streams, a frame
assembler over given stream payloads, the valid-frame matrix, the twelve fixed corrupt frames
and the host decoder as the expected value.  Test infrastructure only."""
import ctypes as C
import struct

import numpy as np

import spec_blosc as sb
from zarrhip import _lib

ZH_OK, ZH_EINVAL, ZH_EDATA, ZH_EUNSUPPORTED = 0, 1, 2, 3
COMP = {"blosclz": 0, "lz4": 1, "zlib": 3, "zstd": 4}


# ---- the host decoder: every expected value -------------------------------------------------
def host_decode(frame):
    """zh_blosc_decompress: (status, decoded bytes or None, message)."""
    L = _lib.lib()
    frame = bytes(frame)
    src = (C.c_char * max(1, len(frame))).from_buffer_copy(frame or b"\0")
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    st = L.zh_blosc_decompress(src, len(frame), None, 0, C.byref(n), err, 256)
    if st != ZH_OK:
        return st, None, err.value.decode()
    dst = (C.c_char * max(1, n.value))()
    st = L.zh_blosc_decompress(src, len(frame), dst, n.value, C.byref(n), err, 256)
    if st != ZH_OK:
        return st, None, err.value.decode()
    return st, bytes(dst)[:n.value], ""


def size_query(frame):
    """zh_blosc_decompress with dst NULL: (status, nbytes, message)."""
    L = _lib.lib()
    frame = bytes(frame)
    src = (C.c_char * max(1, len(frame))).from_buffer_copy(frame or b"\0")
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    st = L.zh_blosc_decompress(src, len(frame), None, 0, C.byref(n), err, 256)
    return st, n.value, err.value.decode()


# ---- token emitters ------------------------------------------------------------------------
def lz4_seq(ops, last=b""):
    """LZ4 block from sequences (literals, match offset, match length >= 4) and the closing
    literal-only sequence `last` (None: no closing sequence)."""
    out = bytearray()
    for lit, off, ml in ops:
        out.append((min(len(lit), 15) << 4) | min(ml - 4, 15))
        if len(lit) >= 15:
            out += sb._ext(len(lit) - 15)
        out += lit
        out += struct.pack("<H", off)
        if ml - 4 >= 15:
            out += sb._ext(ml - 4 - 15)
    if last is not None:
        out.append(min(len(last), 15) << 4)
        if len(last) >= 15:
            out += sb._ext(len(last) - 15)
        out += last
    return bytes(out)


def lz4_expand(ops, last=b""):
    """What lz4_seq's stream decodes to (the format's definition, for sizing frames)."""
    out = bytearray()
    for lit, off, ml in ops:
        out += lit
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out + (last or b""))


def blz_seq(ops):
    """BloscLZ stream from ("lit", bytes <= 32) and ("match", distance >= 1, length >= 3)."""
    out = bytearray()
    for op in ops:
        if op[0] == "lit":
            out.append(len(op[1]) - 1)
            out += op[1]
            continue
        _, distance, length = op
        dist, ln = distance - 1, length - 3
        far = dist >= 8191
        hi = 31 if far else dist >> 8
        if ln < 6:
            out.append(((ln + 1) << 5) | hi)
        else:
            out.append((7 << 5) | hi)
            out += sb._ext(ln - 6)
        if far:
            d = dist - 8191
            out += bytes([255, d >> 8, d & 255])
        else:
            out.append(dist & 255)
    return bytes(out)


def frame_streams(blocks, nbytes, typesize, blocksize, comp, shuffle=False, split=False,
                  bitshuffle=False, version=2):
    """A blosc1 frame around given stream payloads: blocks = [[payload, ...], ...] (a payload
    as long as its stream is a stored-raw stream)."""
    flags = (COMP[comp] << 5) | (0x01 if shuffle else 0) | (0x04 if bitshuffle else 0) | \
        (0 if split else 0x10)
    base = 16 + 4 * len(blocks)
    body, starts = bytearray(), []
    for streams in blocks:
        starts.append(base + len(body))
        for p in streams:
            body += struct.pack("<i", len(p)) + p
    hdr = struct.pack("<BBBBIII", version, 1, flags, typesize, nbytes, blocksize,
                      base + len(body))
    return hdr + struct.pack("<%di" % len(blocks), *starts) + bytes(body)


# ---- valid frames ----------------------------------------------------------------------------
def payloads():
    """The five payloads of test_blosc._payloads."""
    rng = np.random.default_rng(7)
    yield "arange_i4", np.arange(5000, dtype="<i4").tobytes()
    yield "runs", bytes([7]) * 3000 + bytes(range(256)) * 3 + bytes(1000)
    yield "random", rng.integers(0, 256, 4099, dtype=np.uint8).tobytes()
    yield "text", (b"the quick brown fox jumps over the lazy dog " * 200)[:7777]
    far = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    yield "far", far + bytes(50) + far[:4000]   # BloscLZ matches beyond 8191 bytes


SHAPES = [(1, 65536, None), (2, 16384, True), (4, 2048, None), (4, 4096, True),
          (8, 1024, False), (3, 3000, None), (16, 4096, True)]
# (shuffle, bitshuffle, frame version)
SHUFFLES = [(False, False, 2), (True, False, 2), (False, True, 2), (False, True, 3)]

_matrix = None


def matrix():
    """[(label, frame)] over compressor x (typesize, blocksize, split) x shuffle x payload:
    split and unsplit blocks, leftover blocks, stored-raw streams (the random payload)."""
    global _matrix
    if _matrix is None:
        out = []
        for comp in ("lz4", "blosclz"):
            for ts, bs, split in SHAPES:
                for shuf, bit, ver in SHUFFLES:
                    for name, data in payloads():
                        f = sb.frame(data, ts, bs, comp, shuf, split, bitshuffle=bit, version=ver)
                        out.append((f"{comp}-{ts}-{bs}-{split}-{shuf}-{bit}-v{ver}-{name}", f))
        _matrix = out
    return _matrix


def mutations(comp, split):
    """300 seeded mutations of one valid frame, of the kinds in
    test_blosc.test_mutated_frames_never_crash."""
    rng = np.random.default_rng(100 + len(comp) + split)
    data = (np.arange(6000, dtype="<i4") % 97).tobytes()
    good = sb.frame(data, 4, 4096, comp, True, split)
    out = []
    for i in range(300):
        b = bytearray(good)
        kind = i % 4
        if kind == 0:      # flip a few payload bytes
            for _ in range(int(rng.integers(1, 6))):
                b[int(rng.integers(16, len(b)))] ^= int(rng.integers(1, 256))
        elif kind == 1:    # truncate
            b = b[:int(rng.integers(0, len(b)))]
        elif kind == 2:    # overwrite a header field (sizes, block size, compressed size)
            o = int(rng.choice([4, 8, 12]))
            b[o:o + 4] = struct.pack("<I", int(rng.integers(0, 1 << 32)))
        else:              # corrupt a block start offset
            if len(b) >= 20:
                b[16:20] = struct.pack("<I", int(rng.integers(0, 1 << 32)))
        out.append(bytes(b))
    return out


# ---- the twelve corrupt frames ---------------------------------------------------------------
def _one(payload, rawsize, comp="lz4"):
    return frame_streams([[payload]], rawsize, 1, max(rawsize, 1), comp)


def corrupt_frames():
    """[(kind, frame)]: two frames of each kind, every one a single unshuffled block whose
    stream breaks one acceptance rule of the host decoder."""
    r = np.random.default_rng(11).integers(0, 256, 64, dtype=np.uint8).tobytes()
    lit = lambda b: ("lit", b)
    out = [
        # a match offset beyond the bytes produced so far
        ("offset-beyond", _one(lz4_seq([(r[:40], 41, 20)], r[:10]), 70)),
        ("offset-beyond", _one(blz_seq([lit(r[:20]), ("match", 21, 30), lit(r[:10])]), 60,
                               "blosclz")),
        # offset 0
        ("offset-0", _one(lz4_seq([(r[:40], 0, 20)], r[:10]), 70)),
        ("offset-0", _one(lz4_seq([(r[:40], 8, 20), (r[:3], 0, 7)], r[:10]), 80)),
        # a 255-continued length that runs into the end of the stream
        ("length-run", _one(bytes([0xF0, 255, 255]), 600)),
        ("length-run", _one(bytes([0x4F]) + r[:4] + struct.pack("<H", 4) + bytes([255, 255]),
                            900)),
    ]
    # csize past the frame: the int32 in front of the stream says more than the frame holds
    good = bytearray(_one(lz4_seq([(r[:40], 8, 20)], r[:10]), 70))
    for extra in (1, 0x7FFFFF00):
        b = bytearray(good)
        (cs,) = struct.unpack_from("<i", b, 20)
        struct.pack_into("<i", b, 20, cs + extra)
        out.append(("csize-past-frame", bytes(b)))
    out += [
        # too few bytes: a well-formed stream that ends before the raw size
        ("too-few", _one(lz4_seq([(r[:40], 8, 10)], r[:10]), 70)),
        ("too-few", _one(blz_seq([lit(r[:20]), ("match", 4, 30)]), 60, "blosclz")),
        # too many: a match / literal run that passes the raw size
        ("too-many", _one(lz4_seq([(r[:40], 8, 31)], None), 70)),
        ("too-many", _one(blz_seq([lit(r[:20]), ("match", 4, 30), lit(r[:32])]), 60, "blosclz")),
    ]
    assert len(out) == 12
    return out
