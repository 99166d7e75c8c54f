"""Gzip members compressed on the device (zh_gzip_encode_batch, zarr-java_amd/csrc/
zh_gzip_enc_kernels.hip) and the write path that uses it when asked to (ZH_GZIP_ENCODE_DEVICE=1).
Every expected member is zh_gzip_compress on the same bytes, byte for byte; the stored members
are decoded with zlib and compared with the oracle's encoding of the chunk; the arrays are read
back through both read routes; with the switch unset every stored byte is zlib's."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import gzip_enc_inputs as gi
import oracle as O
import zarrhip as z
from zarrhip import _abi as A
from zarrhip import _lib

pytestmark = pytest.mark.gpu

SPAN = 64 << 10       # bytes per workgroup of the CRC kernel
PIECE = 256           # bytes per thread of it


class Uploaded:
    """Buffers side by side in one device allocation; buffer k starts at an address that is
    align[k] modulo 16 (default: k % 5 bytes behind the one before, as the zstd tests do)."""

    def __init__(self, dev, buffers, align=None):
        self.dev, self.sources, pos = dev, [], 0
        for k, b in enumerate(buffers):
            if align is not None:
                pos += (align[k] - pos) % 16
            self.sources.append((pos, len(b)))
            pos += len(b) + (k % 5 if align is None else 0)
        host = bytearray(max(1, pos))
        for (o, n), b in zip(self.sources, buffers):
            host[o:o + n] = b
        self.ptr = dev.malloc(len(host))
        assert self.ptr % 16 == 0
        dev.h2d(self.ptr, bytes(host))
        self.sources = [(self.ptr + o, n) for o, n in self.sources]

    def free(self):
        self.dev.free(self.ptr)


def encode(dev, buffers, bs):
    """zh_gzip_encode_batch twice over the uploaded buffers: the members, checked for placement
    and for being the same both times."""
    up = Uploaded(dev, buffers)
    try:
        out, rows = dev.gzip_encode_batch_raw(up.sources, bs)
        out2, rows2 = dev.gzip_encode_batch_raw(up.sources, bs)
    finally:
        up.free()
    members = [bytes(out[o:o + n]) for o, n in rows]
    assert members == [bytes(out2[o:o + n]) for o, n in rows2]
    end = 0
    for (o, n), b in zip(rows, buffers):      # in order, 16-byte aligned, never overlapping
        assert o >= end and o % 16 == 0 and 20 <= n <= gi.bound(len(b), bs)
        end = o + n
    assert end <= len(out)
    return members


# ---- batch level -----------------------------------------------------------------------------
def test_matrix_equals_the_host_writer(dev):
    """The input matrix of test_gzip_encode_host.py, one batch per block size: the parameters
    belong to the batch."""
    groups = {}
    for label, data, bs in gi.matrix():
        groups.setdefault(bs, []).append((label, data))
    assert len(groups) == len(gi.BLOCKSIZES)
    for bs, items in groups.items():
        labels, buffers = zip(*items)
        members = encode(dev, buffers, bs)
        for label, data, f in zip(labels, buffers, members):
            assert f == _lib.gzip_compress(data, bs), label
    assert _lib.lib().zh_debug_gzip_encode_kernel_ms() > 0
    parts = _lib.gzip_encode_kernel_parts_ms()
    assert all(v > 0 for v in parts.values()), parts


def test_both_block_capacities(dev):
    """The match kernel is built for blocks of at most 16 and 32 KiB; a batch takes the smaller
    form that holds its block size: block sizes at and next to the threshold."""
    buffers = [gi.labels(), gi.text(), gi.mix(), gi.far(), gi.random_bytes(70001), b""]
    for bs in (16 << 10, (16 << 10) + 4, 32 << 10):
        members = encode(dev, buffers, bs)
        for k, (data, f) in enumerate(zip(buffers, members)):
            assert f == _lib.gzip_compress(data, bs), (bs, k)


def test_three_hundred_small_members(dev):
    """More members than one table row of 256 bytes and more blocks than one workgroup's."""
    rng = np.random.default_rng(3)
    buffers = []
    for k in range(300):
        n = int(rng.integers(0, 3000))
        a = (np.arange(n) // (1 + k % 7) % (2 + k % 50)).astype(np.uint8)
        if k % 11 == 0:
            a = rng.integers(0, 256, n, dtype=np.uint8)   # stored segments
        buffers.append(a.tobytes())
    members = encode(dev, buffers, 1024)
    forms = set()
    for k, (data, f) in enumerate(zip(buffers, members)):
        assert f == _lib.gzip_compress(data, 1024), k
        assert zlib.decompress(f, 31) == data, k
        forms |= {s[0] for s in gi.segments(f)}
    assert forms == {"stored", "fixed"}


def test_device_crc32(dev):
    """The CRC kernel and the host fold at every source alignment: lengths around a thread's
    piece and around a workgroup's span, and more spans than one."""
    lengths = (0, 1, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, SPAN - 1, SPAN, SPAN + 1,
               3 * SPAN + 5)
    buffers, align = [], []
    for a in range(16):
        for n in lengths:
            buffers.append(gi.random_bytes(n, 40 + a + n % 7))
            align.append(a)
    up = Uploaded(dev, buffers, align)
    try:
        assert [s[0] % 16 for s in up.sources] == align
        got = dev.gzip_crc32(up.sources)
    finally:
        up.free()
    assert got == [zlib.crc32(b) for b in buffers]
    assert got == [_lib.crc32(b) for b in buffers]


def test_empty_batches(dev):
    out, rows = dev.gzip_encode_batch_raw([])
    assert rows == []
    assert dev.gzip_crc32([]) == []
    assert encode(dev, [b"", b"", b""], 0) == [_lib.gzip_compress(b"")] * 3
    with pytest.raises(_lib.ZhError) as e:
        dev.gzip_encode_batch_raw([(0, 0)], -1)
    assert e.value.status == A.ZH_EINVAL


# ---- array level -----------------------------------------------------------------------------
def _data():
    """16^3 int32: runs of five equal values, never 0 (the fill value); chunks (0, 0, 0) and
    (3, 1, 1) and the inner chunk at [4:6, 4:6, 8:12] at fill; chunk (7, 3, 1) noise."""
    d = (np.arange(4096) // 5 % 50 + 1).astype(np.int32).reshape(16, 16, 16)
    d[0:2, 0:4, 0:8] = 0
    d[6:8, 4:8, 8:16] = 0
    d[4:6, 4:6, 8:12] = 0
    d[14:16, 12:16, 8:16] = np.random.default_rng(5).integers(1, 2 ** 31 - 1, (2, 4, 8))
    return d


ABSENT = {(0, 0, 0), (3, 1, 1)}
NOISE = (7, 3, 1)

CODECS = {
    "bytes-gzip": lambda c: c.withBytes("LITTLE").withGzip(5),
    "transpose-big-gzip": lambda c: c.withTranspose([1, 0, 2]).withBytes("BIG").withGzip(3),
    "sharded-start": lambda c: c.withSharding(
        [2, 2, 4], lambda c1: c1.withBytes("LITTLE").withGzip(), "start"),
    "sharded-end": lambda c: c.withSharding(
        [2, 2, 4], lambda c1: c1.withBytes("LITTLE").withGzip(7), "end"),
}
LEVEL = {"bytes-gzip": 5, "transpose-big-gzip": 3, "sharded-start": 5, "sharded-end": 7}


def _meta(codecs):
    return (z.ArrayMetadataBuilder().withShape(16, 16, 16).withDataType(z.DataType.INT32)
            .withChunkShape(2, 4, 8).withFillValue(0).withCodecs(codecs).build())


def _objects(a):
    """{chunk coords: stored bytes or None} over the whole array."""
    shape = list(a.metadata.shape)
    out = {}
    for c in a._chunk_coords([0] * len(shape), shape):
        h = a._handle(c)
        out[c] = bytes(h.read()) if h.exists() else None
    return out


def _entries(a, shard):
    """[(offset, nbytes) or None] of a stored or oracle shard, its index checked."""
    ch = a.chain.chain
    n = a._n_inner()
    isz = 16 * n + (4 if ch["index_crc32c"] else 0)
    idx = shard[:isz] if ch["index_location"] == A.ZH_INDEX_START else shard[-isz:]
    fmt = ">QQ" if ch["index_endian"] == A.ZH_ENDIAN_BIG else "<QQ"
    ents = [struct.unpack(fmt, idx[16 * e:16 * e + 16]) for e in range(n)]
    if ch["index_crc32c"]:
        assert struct.unpack("<I", idx[16 * n:])[0] == O.crc32c(idx[:16 * n])
    return [None if off == 2 ** 64 - 1 else (off, nb) for off, nb in ents], isz


def _pairs(a, stored, want):
    """(chunk coords, stored member, the oracle's bytes of that chunk or inner chunk) over the
    array; absent chunks and elided inner chunks agree with the oracle."""
    for c, obj in stored.items():
        if obj is None:
            assert want[c] is None, c
            continue
        assert want[c] is not None, c
        if not a.chain.chain["sharded"]:
            yield c, obj, want[c]
            continue
        (se, isz), (we, _) = _entries(a, obj), _entries(a, want[c])
        assert [e is None for e in se] == [e is None for e in we], c
        assert sum(s[1] for s in se if s) + isz == len(obj), c
        for s, w in zip(se, we):
            if s is not None:
                yield c, obj[s[0]:s[0] + s[1]], want[c][w[0]:w[0] + w[1]]


def _read_both_ways(a, data, monkeypatch):
    for files in ("1", "0"):
        monkeypatch.setenv("ZH_FILES", files)
        r = z.Array.open(a.storeHandle)
        np.testing.assert_array_equal(r.read(), data)
        np.testing.assert_array_equal(r.read([3, 1, 5], [9, 13, 10]), data[3:12, 1:14, 5:15])
    monkeypatch.delenv("ZH_FILES")


@pytest.mark.parametrize("case", list(CODECS))
def test_array_write_device_route(dev, case, tmp_path, monkeypatch):
    data = _data()
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "1")
    a = z.Array.create(z.FilesystemStore(tmp_path).resolve("dev"), _meta(CODECS[case]))
    a.write(None, data)
    info = a.last_write_info
    assert info["gzip_device_frames"] > 0 and info["gzip_host_frames"] == 0
    assert info["blosc_device_frames"] == 0 and info["zstd_device_frames"] == 0
    stored = _objects(a)
    assert {c for c, b in stored.items() if b is None} == ABSENT        # all fill: no key
    assert info["stored_bytes"] == sum(len(b) for b in stored.values() if b is not None)
    want = dict(zip(stored, O.array_write(a.zmeta, data.tobytes(), [0, 0, 0], [16, 16, 16])))
    seen, forms = 0, set()
    for c, f, raw in _pairs(a, stored, want):
        assert zlib.decompress(f, 31) == raw, c
        assert f == _lib.gzip_compress(raw), c          # one writer, two places
        kinds = {s[0] for s in gi.segments(f)}
        assert kinds == ({"stored"} if c == NOISE else {"fixed"}), c
        forms |= kinds
        seen += 1
    assert seen == info["gzip_device_frames"] and forms == {"stored", "fixed"}
    if a.chain.chain["sharded"]:
        assert seen == (64 - 2) * 4 - 1                 # one inner chunk elided
    _read_both_ways(a, data, monkeypatch)
    # a partial write: chunk (2, 0, 0) is read, patched and encoded on the device again; chunk
    # (1, 0, 0) becomes all fill and loses its key
    a.write([2, 0, 0], np.zeros((3, 4, 8), np.int32))
    assert a.last_write_info["gzip_host_frames"] == 0
    assert a.last_write_info["gzip_device_frames"] > 0
    data[2:5, 0:4, 0:8] = 0
    assert {c for c, b in _objects(a).items() if b is None} == ABSENT | {(1, 0, 0)}
    _read_both_ways(a, data, monkeypatch)


@pytest.mark.parametrize("case", list(CODECS))
def test_switch_unset_stores_zlib(dev, case, tmp_path, monkeypatch):
    data = _data()
    monkeypatch.delenv("ZH_GZIP_ENCODE_DEVICE", raising=False)
    a = z.Array.create(z.FilesystemStore(tmp_path).resolve("host"), _meta(CODECS[case]))
    a.write(None, data)
    info = a.last_write_info
    assert info["gzip_device_frames"] == 0 and info["gzip_host_frames"] > 0
    stored = _objects(a)
    assert {c for c, b in stored.items() if b is None} == ABSENT
    want = dict(zip(stored, O.array_write(a.zmeta, data.tobytes(), [0, 0, 0], [16, 16, 16])))
    seen = 0
    for c, f, raw in _pairs(a, stored, want):
        assert f == gzip.compress(raw, LEVEL[case], mtime=0), c
        seen += 1
    assert seen == info["gzip_host_frames"]
    _read_both_ways(a, data, monkeypatch)


def test_other_routes_keep_the_host(dev, tmp_path, monkeypatch):
    """gzip followed by crc32c, and a write with two devices listed, stay zlib's with the
    switch at 1."""
    data = _data()
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "1")
    a = z.Array.create(z.MemoryStore().resolve("gc"),
                       _meta(lambda c: c.withBytes("LITTLE").withGzip(4).withCrc32c()))
    a.write(None, data)
    assert a.last_write_info["gzip_device_frames"] == 0
    want = dict(zip(_objects(a), O.array_write(a.zmeta, data.tobytes(), [0, 0, 0],
                                               [16, 16, 16])))
    for c, b in _objects(a).items():
        if b is not None:
            assert b[:-4] == gzip.compress(want[c], 4, mtime=0), c
            assert struct.unpack("<I", b[-4:])[0] == O.crc32c(b[:-4]), c
    np.testing.assert_array_equal(z.Array.open(a.storeHandle).read(), data)
    monkeypatch.setenv("ZH_DEVICES", "0,0")
    b = z.Array.create(z.MemoryStore().resolve("two"), _meta(CODECS["bytes-gzip"]))
    b.write(None, data)
    info = b.last_write_info
    assert info["gzip_device_frames"] == 0 and info["gzip_host_frames"] == 64 - 2
    want = dict(zip(_objects(b), O.array_write(b.zmeta, data.tobytes(), [0, 0, 0],
                                               [16, 16, 16])))
    for c, obj in _objects(b).items():
        assert obj == (None if want[c] is None else gzip.compress(want[c], 5, mtime=0)), c
    monkeypatch.delenv("ZH_DEVICES")
    np.testing.assert_array_equal(z.Array.open(b.storeHandle).read(), data)


# ---- a seeded fuzz: random small arrays with a gzip stage --------------------------------------
DTYPES = [z.DataType.INT8, z.DataType.UINT8, z.DataType.INT16, z.DataType.UINT16,
          z.DataType.INT32, z.DataType.UINT32, z.DataType.INT64, z.DataType.UINT64,
          z.DataType.FLOAT32, z.DataType.FLOAT64, z.DataType.BOOL]


def random_gzip_array(seed):
    """A random data type, shape, chunk grid and chain ending in gzip (transposed or not,
    either endianness, sharded or not with the index at either end); values from a small set, so
    that chunks compress, with blocks of noise and blocks at fill."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 4))
    dt = DTYPES[int(rng.integers(len(DTYPES)))]
    chunk = [int(rng.choice([4, 6, 8, 12])) for _ in range(n)]
    shape = [int(rng.integers(1, 3 * c + 2)) for c in chunk]
    sharded = rng.random() < 0.5
    inner = [int(rng.choice([d for d in range(1, c + 1) if c % d == 0])) for c in chunk]
    order = [int(x) for x in rng.permutation(n)] if rng.random() < 0.4 else None
    endian = "BIG" if rng.random() < 0.5 else "LITTLE"
    level = int(rng.integers(0, 10))

    def leaf(c):
        if order is not None:
            c = c.withTranspose(order)
        return c.withBytes(endian).withGzip(level)
    if sharded:
        loc = "start" if rng.random() < 0.5 else "end"
        codecs = lambda c: c.withSharding(inner, leaf, loc)  # noqa: E731
    else:
        codecs = leaf
    meta = (z.ArrayMetadataBuilder().withShape(*shape).withDataType(dt).withChunkShape(*chunk)
            .withFillValue(0).withCodecs(codecs).build())
    npdt = dt.numpy
    if dt == z.DataType.BOOL:
        a = rng.random(shape) < 0.5
    else:
        a = rng.integers(1, 4, size=shape).astype(npdt)
    blk = inner if sharded else chunk
    for k in range(int(rng.integers(0, 4))):  # blocks at fill (elided) and blocks of noise
        lo = [int(rng.integers(0, s)) // b * b for s, b in zip(shape, blk)]
        sl = tuple(slice(o, o + b) for o, b in zip(lo, blk))
        if k % 2 == 0 or dt == z.DataType.BOOL:
            a[sl] = 0
        else:
            a[sl] = rng.integers(1, 120, size=a[sl].shape).astype(npdt)
    return meta, a, rng


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_gzip_arrays_round_trip(dev, tmp_path, monkeypatch, seed):
    meta, a, rng = random_gzip_array(seed)
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "1")
    arr = z.Array.create(z.FilesystemStore(tmp_path).resolve("a"), meta)
    arr.write(None, a)
    info = arr.last_write_info
    assert info["gzip_host_frames"] == 0, seed
    stored = _objects(arr)
    want = dict(zip(stored, O.array_write(arr.zmeta, a.tobytes(), [0] * a.ndim, list(a.shape))))
    seen = 0
    for c, f, raw in _pairs(arr, stored, want):
        assert zlib.decompress(f, 31) == raw, (seed, c)
        seen += 1
    assert seen == info["gzip_device_frames"] and (seen > 0 or not a.any()), seed
    regions = [([0] * a.ndim, list(a.shape))]
    for _ in range(3):
        off = [int(rng.integers(0, s)) for s in a.shape]
        regions.append((off, [int(rng.integers(1, s - o + 1)) for s, o in zip(a.shape, off)]))
    for files in ("1", "0"):
        monkeypatch.setenv("ZH_FILES", files)
        b = z.Array.open(z.FilesystemStore(tmp_path).resolve("a"))
        for off, shp in regions:
            sl = tuple(slice(o, o + s) for o, s in zip(off, shp))
            np.testing.assert_array_equal(b.read(off, shp), a[sl],
                                          err_msg=f"seed {seed} files {files} {off} {shp}")
