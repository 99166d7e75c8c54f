"""The input matrix of the zstd frame writer's tests (test_zstd_encode_host.py on the host,
test_gpu_zstd_encode.py on the device): (label, bytes, checksum, blocksize) rows, blocksize 0
being the default, and a walk over the blocks of a frame the writer made."""
import struct

import numpy as np

DEFAULT_BLOCK = 16 << 10     # zh_ze::kDefaultBlock
ONE_BLOCK = 32 << 10         # holds mix() and far() in one block
BLOCKSIZES = (1 << 10, 0)    # the smallest block the params take, and the default
RAW_BLOCK = 128 << 10


def labels():
    """2048 seeded values in 0..49 as <u2, each repeated 64 times: a piecewise-constant image."""
    rng = np.random.default_rng(7)
    return np.repeat(rng.integers(0, 50, 2048).astype("<u2"), 64).tobytes()


def text():
    words = b"zarr chunk shard codec bytes index array store fill value zstd frame block".split()
    rng = np.random.default_rng(8)
    return b" ".join(words[i] for i in rng.integers(0, len(words), 12000))


def mix():
    """20000 random bytes, then 12000 zeros: in one block of ONE_BLOCK a literal length and a
    match length in the high codes."""
    rng = np.random.default_rng(9)
    return rng.integers(0, 256, 20000, dtype=np.uint8).tobytes() + bytes(12000)


def far():
    """A 600-byte random piece at the start and the end of one block of ONE_BLOCK, zeros between
    them (a long match leaves the hash table alone): an offset of 30 600."""
    rng = np.random.default_rng(10)
    a = rng.integers(0, 256, 600, dtype=np.uint8).tobytes()
    return a + bytes(30000) + a


def random_bytes(n, seed=11):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def sizes(bs):
    b = bs or DEFAULT_BLOCK
    return (0, 1, 12, 13, b - 1, b, b + 1, 3 * b + 5)


def matrix():
    rows = []
    for k, bs in enumerate(BLOCKSIZES):
        for j, n in enumerate(sizes(bs)):
            cs = bool((j + k) % 2)
            rows.append((f"zeros-{n}-b{bs}", bytes(n), cs, bs))
            rows.append((f"random-{n}-b{bs}", random_bytes(n, 100 + j), not cs, bs))
        for cs in (True, False):
            rows.append((f"labels-b{bs}-c{int(cs)}", labels(), cs, bs))
            rows.append((f"text-b{bs}-c{int(cs)}", text(), cs, bs))
            rows.append((f"mix-b{bs}-c{int(cs)}", mix(), cs, bs))
        rows.append((f"far-b{bs}", far(), True, bs))
    for cs in (True, False):
        rows.append((f"mix-b{ONE_BLOCK}-c{int(cs)}", mix(), cs, ONE_BLOCK))
        rows.append((f"far-b{ONE_BLOCK}-c{int(cs)}", far(), cs, ONE_BLOCK))
    return rows


def blocks(frame):
    """[(type, size, nseq or None)] of a frame with the writer's header (13 bytes)."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd" and frame[4] & ~4 == 0xE0
    p, out = 13, []
    while True:
        h = frame[p] | frame[p + 1] << 8 | frame[p + 2] << 16
        p += 3
        typ, size = (h >> 1) & 3, h >> 3
        nseq = None
        if typ == 2:
            assert frame[p] & 15 == 0x0C                     # raw literals, 3-byte header
            nl = (frame[p] >> 4) + (frame[p + 1] << 4) + (frame[p + 2] << 12)
            q = p + 3 + nl
            nseq = frame[q] if frame[q] < 128 else ((frame[q] - 128) << 8) + frame[q + 1]
            assert frame[q] < 255 and frame[q + (1 if frame[q] < 128 else 2)] == 0   # predefined
        out.append((typ, size, nseq))
        p += size
        if h & 1:
            break
    assert p + (4 if frame[4] & 4 else 0) == len(frame)
    return out


def content_size(frame):
    return struct.unpack("<Q", frame[5:13])[0]
