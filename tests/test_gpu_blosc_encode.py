"""Blosc LZ4 frames compressed on the device (zh_blosc_encode_batch, zarr-java_amd/csrc/
zh_blosc_enc_kernels.hip) and the write path that uses it (ZH_BLOSC_ENCODE_DEVICE).  Every
expected frame is zh_blosc_compress on the same bytes, byte for byte; the arrays are read back
through both read routes and compared with what the host route stores."""
import numpy as np
import pytest

import blosc_enc_inputs as bi
import blosc_frames as bf
import zarrhip as z
from zarrhip import _lib, v2

pytestmark = pytest.mark.gpu


class Uploaded:
    """Buffers side by side in one device allocation, at offsets of every alignment."""

    def __init__(self, dev, buffers):
        self.dev, self.sources, pos = dev, [], 0
        for k, b in enumerate(buffers):
            self.sources.append((pos, len(b)))
            pos += len(b) + k % 5
        host = bytearray(max(1, pos))
        for (o, n), b in zip(self.sources, buffers):
            host[o:o + n] = b
        self.ptr = dev.malloc(len(host))
        dev.h2d(self.ptr, bytes(host))
        self.sources = [(self.ptr + o, n) for o, n in self.sources]

    def free(self):
        self.dev.free(self.ptr)


def encode(dev, buffers, ts, sh, bs):
    """zh_blosc_encode_batch twice over the uploaded buffers: the frames, checked for placement
    and for being the same both times."""
    up = Uploaded(dev, buffers)
    try:
        out, rows = dev.blosc_encode_batch_raw(up.sources, ts, sh, bs)
        out2, rows2 = dev.blosc_encode_batch_raw(up.sources, ts, sh, bs)
    finally:
        up.free()
    frames = [bytes(out[o:o + n]) for o, n in rows]
    assert frames == [bytes(out2[o:o + n]) for o, n in rows2]
    end = 0
    for o, n in rows:                       # in order, 16-byte aligned, never overlapping
        assert o >= end and o % 16 == 0 and n >= 16
        end = o + n
    assert end <= len(out)
    return frames


def decode(dev, frames):
    ptr, rows = dev.blosc_decode_batch(frames)
    try:
        raw = dev.d2h(ptr, max([o + n for o, n, _ in rows] + [1]))
    finally:
        dev.free(ptr)
    return [raw[o:o + n] for o, n, _ in rows]


# ---- batch level -----------------------------------------------------------------------------
def test_matrix_equals_the_host_writer(dev):
    """The input matrix of test_blosc_encode_host.py, one batch per (typesize, shuffle, block
    size): the parameters belong to the batch."""
    groups = {}
    for label, data, ts, sh, bs in bi.matrix():
        groups.setdefault((ts, sh, bs), []).append((label, data))
    assert len(groups) == len(bi.TYPESIZES) * len(bi.SHUFFLES) * 3
    for (ts, sh, bs), items in groups.items():
        labels, buffers = zip(*items)
        frames = encode(dev, buffers, ts, sh, bs)
        for label, data, f in zip(labels, buffers, frames):
            assert f == _lib.blosc_compress(data, ts, sh, bs), label
        assert decode(dev, frames) == list(buffers), (ts, sh, bs)
    assert _lib.lib().zh_debug_blosc_encode_kernel_ms() > 0


def test_three_hundred_small_frames(dev):
    """More frames than one table row of 256 bytes and more blocks than one wave's worth."""
    rng = np.random.default_rng(3)
    buffers = []
    for k in range(300):
        n = int(rng.integers(0, 1400))
        a = (np.arange(n) // (1 + k % 7) % (2 + k % 50)).astype(np.uint8)
        if k % 11 == 0:
            a = rng.integers(0, 256, n, dtype=np.uint8)   # stored raw or MEMCPYED
        buffers.append(a.tobytes())
    for ts, sh, bs in ((4, 1, 0), (2, 2, 512), (1, 0, 256)):
        frames = encode(dev, buffers, ts, sh, bs)
        for k, (data, f) in enumerate(zip(buffers, frames)):
            assert f == _lib.blosc_compress(data, ts, sh, bs), k
        assert decode(dev, frames) == buffers
    kinds = {f[2] & 0x02 for f in frames}
    assert kinds == {0, 2}


def test_every_block_capacity(dev):
    """The kernel is built for blocks of at most 16, 32 and 64 KiB; a slab takes the smallest
    form that holds its blocks: block sizes at and next to each threshold."""
    buffers = [bi.img(), bi.ramp(), bi.smooth(100001), bytes(70000)]
    for bs in (16 << 10, (16 << 10) + 4, 32 << 10, (32 << 10) + 4, 64 << 10):
        for ts, sh in ((2, 1), (4, 2), (1, 0)):
            frames = encode(dev, buffers, ts, sh, bs)
            for k, (data, f) in enumerate(zip(buffers, frames)):
                assert f == _lib.blosc_compress(data, ts, sh, bs), (bs, ts, sh, k)


def test_empty_batches(dev):
    out, rows = dev.blosc_encode_batch_raw([], 4, 1)
    assert rows == []
    assert encode(dev, [b"", b"", b""], 4, 1, 0) == [_lib.blosc_compress(b"", 4, 1)] * 3
    with pytest.raises(_lib.ZhError) as e:
        dev.blosc_encode_batch_raw([(0, 0)], 0, 1)
    assert e.value.status == bf.ZH_EINVAL


# ---- array level -----------------------------------------------------------------------------
DATA3 = (np.add.outer(np.add.outer(np.arange(16) * 700, np.arange(16) * 40), np.arange(32))
         % 65536).astype(np.uint16)
DATA2 = (np.add.outer(np.arange(15) * 3, np.arange(10)) + 2).astype(np.uint32)


def _v3(codecs):
    return (z.ArrayMetadataBuilder().withShape(16, 16, 32).withDataType(z.DataType.UINT16)
            .withChunkShape(8, 16, 32).withFillValue(0).withCodecs(codecs).build())


def _sharded(loc):
    return lambda c: c.withSharding(
        [4, 8, 16], lambda c1: c1.withTranspose([2, 0, 1]).withBytes("BIG")
        .withBlosc("lz4", "shuffle"), loc)


CASES = {
    "unsharded": (z.Array, lambda: _v3(lambda c: c.withBytes("LITTLE").withBlosc("lz4", "shuffle")),
                  DATA3),
    "sharded-end": (z.Array, lambda: _v3(_sharded("end")), DATA3),
    "sharded-start": (z.Array, lambda: _v3(_sharded("start")), DATA3),
    "v2": (v2.Array, lambda: (v2.ArrayMetadataBuilder().withShape(15, 10)
                              .withDataType(v2.DataType.UINT32).withChunks(4, 5).withFillValue(2)
                              .withBloscCompressor("lz4", "shuffle", 6).build()), DATA2),
}


def _store(kind, tmp_path, name):
    return (z.MemoryStore() if kind == "memory" else z.FilesystemStore(tmp_path)).resolve(name)


def _objects(a):
    """{chunk coords: stored bytes or None} over the whole array."""
    shape = list(a.metadata.shape)
    out = {}
    for c in a._chunk_coords([0] * len(shape), shape):
        h = a._handle(c)
        out[c] = bytes(h.read()) if h.exists() else None
    return out


@pytest.mark.parametrize("kind", ["memory", "files"])
@pytest.mark.parametrize("case", list(CASES))
def test_array_write_device_route(dev, case, kind, tmp_path, monkeypatch):
    cls, meta, data = CASES[case]
    monkeypatch.setenv("ZH_BLOSC_ENCODE_DEVICE", "1")
    a = cls.create(_store(kind, tmp_path, "dev"), meta())
    a.write(None, data)
    info = a.last_write_info
    assert info["blosc_device_frames"] > 0 and info["blosc_host_frames"] == 0
    assert info["raw_bytes"] >= data.nbytes and info["stored_bytes"] < info["raw_bytes"]
    stored = _objects(a)
    assert info["stored_bytes"] == sum(len(b) for b in stored.values())
    # both read routes return the data
    for route in ("0", "1"):
        monkeypatch.setenv("ZH_BLOSC_DEVICE", route)
        r = cls.open(a.storeHandle)
        np.testing.assert_array_equal(r.read(), data)
        off = [s // 3 for s in data.shape]
        shp = [s - o - 1 for s, o in zip(data.shape, off)]
        sl = tuple(slice(o, o + n) for o, n in zip(off, shp))
        np.testing.assert_array_equal(r.read(off, shp), data[sl])
    # the host route stores the same objects, byte for byte: one compressor, two places
    monkeypatch.setenv("ZH_BLOSC_ENCODE_DEVICE", "0")
    b = cls.create(_store(kind, tmp_path, "host"), meta())
    b.write(None, data)
    assert b.last_write_info["blosc_device_frames"] == 0
    assert b.last_write_info["blosc_host_frames"] > 0
    assert b.last_write_info["stored_bytes"] == info["stored_bytes"]
    assert _objects(b) == stored


@pytest.mark.parametrize("case", list(CASES))
def test_partial_write_deletes_all_fill_chunks(dev, case, tmp_path, monkeypatch):
    cls, meta, data = CASES[case]
    monkeypatch.setenv("ZH_BLOSC_ENCODE_DEVICE", "1")
    a = cls.create(_store("files", tmp_path, "p"), meta())
    a.write(None, data)
    assert all(v is not None for v in _objects(a).values())
    fill = a.metadata.fill_value
    cs = a.metadata.chunk_shape
    # the fill value over the second chunk along axis 0 and one row more: that chunk's key goes,
    # its neighbour is read, patched and written again
    off = [cs[0] - 1] + [0] * (data.ndim - 1)
    shp = [cs[0] + 1] + list(cs[1:])
    a.write(off, np.full(shp, fill, data.dtype))
    assert a.last_write_info["blosc_device_frames"] > 0
    want = data.copy()
    want[tuple(slice(o, o + n) for o, n in zip(off, shp))] = fill
    gone = tuple([1] + [0] * (data.ndim - 1))
    objs = _objects(a)
    assert objs[gone] is None and sum(v is None for v in objs.values()) == 1
    np.testing.assert_array_equal(cls.open(a.storeHandle).read(), want)


def test_other_cnames_still_store_memcpyed_frames(dev, tmp_path):
    a = z.Array.create(_store("memory", tmp_path, "m"),
                       _v3(lambda c: c.withBytes("LITTLE").withBlosc()))
    a.write(None, DATA3)
    info = a.last_write_info
    assert info["blosc_device_frames"] == 0 and info["blosc_host_frames"] == 2
    assert info["stored_bytes"] == info["raw_bytes"] + 16 * 2
    for b in _objects(a).values():
        assert b[2] & 0x02 and len(b) == 8 * 16 * 32 * 2 + 16
    np.testing.assert_array_equal(z.Array.open(a.storeHandle).read(), DATA3)
