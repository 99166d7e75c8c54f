"""The input matrix of the blosc LZ4 frame writer's tests (test_blosc_encode_host.py on the CPU,
test_gpu_blosc_encode.py on the device): buffers of one 64 KiB block or less, or a small block
plus a leftover, under every typesize and shuffle.  Test infrastructure only."""
import numpy as np

TYPESIZES = (1, 2, 4, 8, 16, 17)
SHUFFLES = (0, 1, 2)          # zh_blosc_enc_params.shuffle: none, byte, bit
BLOCK = 64 << 10
SMALL_BLOCK = 4096            # the configured block size of the "block plus leftover" case


def img():
    """A smooth 128 x 256 uint16 image (64 KiB)."""
    rng = np.random.default_rng(7)
    a = np.outer(np.arange(128) * 40, np.arange(256)) % 65536 + rng.integers(0, 16)
    return a.astype("<u2").tobytes()


def ramp():
    return np.arange(16384, dtype="<u4").tobytes()


def smooth(n):
    """n compressible bytes that are not one run."""
    return bytes((np.arange(n) // 5 % 3).astype(np.uint8))


def payloads(ts):
    """(name, bytes, configured blocksize) for one typesize."""
    rng = np.random.default_rng(11)
    yield "img", img(), BLOCK
    yield "ramp", ramp(), BLOCK
    yield "zeros", bytes(BLOCK), BLOCK
    yield "random", rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes(), BLOCK
    for n in (0, 1, 12, 13, 63, 64, 65):
        yield f"len{n}", smooth(n), 0
    # the split threshold (blocksize / typesize >= 128) and a ragged tail behind it
    for n, name in ((ts * 127, "127el"), (ts * 128, "128el"), (ts * 128 + 3, "128el+3")):
        yield name, smooth(n), 0
    # one full block and a leftover block (never split; 100 bytes: under 128 elements for every
    # typesize, so the liblz4 walk of test_blosc.py reads the same layout)
    yield "block+leftover", smooth(SMALL_BLOCK // ts * ts + 100), SMALL_BLOCK


def matrix():
    """[(label, data, typesize, shuffle, blocksize)]"""
    out = []
    for ts in TYPESIZES:
        for name, data, bs in payloads(ts):
            for sh in SHUFFLES:
                out.append((f"{name}-ts{ts}-sh{sh}", data, ts, sh, bs))
    return out


def shuffled_streams(data, ts):
    """The typesize byte planes of `data` (its length a multiple of ts): the streams of one
    split, byte-shuffled block."""
    a = np.frombuffer(data, np.uint8).reshape(-1, ts).T
    return [a[j].tobytes() for j in range(ts)]
