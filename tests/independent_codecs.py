"""Independent decoders of the two frame formats Array.write stores: zstd frames through libzstd
and blosc1 LZ4 frames through liblz4 (both bundled with pyarrow).  The blosc header, block starts
and stream layout are parsed here; the shuffles are undone with numpy.  Test infrastructure
only: nothing in this module calls into zarrhip or libzarrhip."""
import struct

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

ZSTD_MAGIC = b"\x28\xb5\x2f\xfd"


def zstd_decode(frame, nbytes):
    """`frame` decoded by libzstd into exactly `nbytes` bytes (a frame's checksum is verified by
    libzstd when it carries one)."""
    frame = bytes(frame)
    assert frame[:4] == ZSTD_MAGIC
    if nbytes == 0:    # pyarrow takes no empty destination: the header must say 0 itself
        assert _zstd_says_empty(frame)
        return b""
    out = pa.Codec("zstd").decompress(frame, decompressed_size=nbytes, asbytes=True)
    assert len(out) == nbytes
    return out


def _zstd_says_empty(frame):
    """Frame_Content_Size of RFC 8878 §3.1.1.1 is present and 0."""
    fhd = frame[4]
    fcs_flag, single = fhd >> 6, (fhd >> 5) & 1
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    size = {0: 1 if single else 0, 1: 2, 2: 4, 3: 8}[fcs_flag]
    if size == 0:
        return False
    v = int.from_bytes(frame[p:p + size], "little")
    return (v + 256 if size == 2 else v) == 0


def zstd_has_checksum(frame):
    """Content_Checksum_flag of the frame header descriptor."""
    return bool(frame[4] & 4)


def bit_unshuffle(blk, typesize, version=2):
    """Inverse of spec_blosc.bit_shuffle: for byte position j and bit k, a row of ne/8 bytes
    whose bit m of byte q is bit k of byte j of element 8q+m.  Format 2 shuffles a block only
    when its element count is a multiple of 8; later formats shuffle the multiple-of-8 prefix
    and keep the leftover bytes."""
    blk = bytes(blk)
    ne = len(blk) // typesize
    if version <= 2 and ne % 8:
        return blk
    ne -= ne % 8
    if ne == 0:
        return blk
    rows = np.frombuffer(blk[:ne * typesize], np.uint8).reshape(typesize * 8, ne // 8)
    bits = np.unpackbits(rows, axis=1, bitorder="little")          # [(j, k), e]
    elems = bits.reshape(typesize, 8, ne).transpose(2, 0, 1)          # [e, j, k]
    out = np.packbits(np.ascontiguousarray(elems), axis=2, bitorder="little").ravel()
    return out.tobytes() + blk[ne * typesize:]


def byte_unshuffle(blk, typesize):
    """typesize planes of len // typesize bytes back to elements; the ragged tail stays."""
    blk = bytes(blk)
    n = len(blk) // typesize
    if typesize <= 1 or n == 0:
        return blk
    planes = np.frombuffer(blk[:n * typesize], np.uint8).reshape(typesize, n)
    return planes.T.tobytes() + blk[n * typesize:]


def blosc_lz4_decode(frame):
    """A blosc1 frame with LZ4 streams (or a MEMCPYED one) → its bytes.  Layout rules are
    c-blosc's: block k starts at bstarts[k]; a block is split into typesize streams when the
    header does not say "not split" (0x10) and the block is not the leftover block — a leftover
    block is never split, however many elements it holds; each stream is an int32 size and a
    payload, raw when the size equals the stream's; byte shuffle (0x01, typesize > 1) or bit
    shuffle (0x04) is undone per block."""
    frame = bytes(frame)
    assert len(frame) >= 16
    ver, _, flags, typesize = frame[0], frame[1], frame[2], frame[3]
    nbytes, blocksize, cbytes = struct.unpack("<III", frame[4:16])
    assert cbytes == len(frame) and ver >= 2
    if flags & 0x02:                                   # MEMCPYED: the payload as it is
        assert cbytes == nbytes + 16
        return frame[16:]
    assert flags >> 5 == 1, "LZ4 streams"
    if nbytes == 0:
        return b""
    assert blocksize > 0 and typesize > 0
    nblocks = -(-nbytes // blocksize)
    bstarts = struct.unpack(f"<{nblocks}I", frame[16:16 + 4 * nblocks])
    lz = pa.Codec("lz4_raw")
    out = bytearray()
    for b in range(nblocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        leftover = bsize < blocksize
        nsplits = typesize if not flags & 0x10 and not leftover else 1
        assert bsize % nsplits == 0
        want = bsize // nsplits
        pos, blk = bstarts[b], bytearray()
        for _ in range(nsplits):
            (cs,) = struct.unpack("<i", frame[pos:pos + 4])
            pos += 4
            assert 0 < cs <= want and pos + cs <= len(frame)
            data = frame[pos:pos + cs]
            pos += cs
            blk += data if cs == want else lz.decompress(data, decompressed_size=want,
                                                         asbytes=True)
        assert len(blk) == bsize
        if flags & 0x01:
            blk = byte_unshuffle(blk, typesize)
        elif flags & 0x04:
            blk = bit_unshuffle(blk, typesize, ver)
        out += blk
    assert len(out) == nbytes
    return bytes(out)
