"""Blosc frames with zlib streams compressed on the device (zh_blosc_encode_batch_ex with
ZH_BLOSC_ENC_ZLIB and ZH_BLOSC_ENC_DYNAMIC, zarr-java_amd/csrc/zh_blosc_enc_kernels.hip) and the
write path that uses it (ZH_BLOSC_ZLIB_ENCODE=1 or 2).  Every expected frame is
zh_blosc_compress_ex on the same bytes, byte for byte (test_blosc_zlib_encode_host.py holds that
one to the frame built in Python); the frames are decoded again on the device; the arrays are read
back through both read routes and compared with what the host route stores."""
import numpy as np
import pytest

import blosc_enc_inputs as bi
import blosc_frames as bf
import blosc_zlib_enc_inputs as be
import blosc_zlib_inputs as bz
import zarrhip as z
from test_gpu_blosc_encode import DATA2, DATA3, Uploaded, _objects, _store, _v3
from zarrhip import _lib, v2

pytestmark = pytest.mark.gpu


def encode(dev, buffers, ts, sh, bs, flags):
    """zh_blosc_encode_batch_ex twice over the uploaded buffers (sources at every alignment): the
    frames, checked for placement and for being the same both times."""
    up = Uploaded(dev, buffers)
    try:
        out, rows = dev.blosc_encode_batch_raw(up.sources, ts, sh, bs, flags=flags)
        out2, rows2 = dev.blosc_encode_batch_raw(up.sources, ts, sh, bs, zlib=True,
                                                 dynamic=flags == be.FLAG_DYN)
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
    """The frames decoded on the device, zlib streams included."""
    ptr, rows = dev.blosc_decode_batch(frames, flags=bz.FLAG)
    try:
        raw = dev.d2h(ptr, max([o + n for o, n, _ in rows] + [1]))
    finally:
        dev.free(ptr)
    assert all(where in (0, 2) for _, _, where in rows)    # none is left to the host
    return [raw[o:o + n] for o, n, _ in rows]


def host(data, ts, sh, bs, flags):
    return _lib.blosc_compress(data, ts, sh, bs, flags=flags)


# ---- batch level -----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", be.FLAGS)
def test_matrix_equals_the_host_writer(dev, flags):
    groups = {}
    for label, data, ts, sh, bs in bi.matrix():
        groups.setdefault((ts, sh, bs), []).append((label, data))
    assert len(groups) == len(bi.TYPESIZES) * len(bi.SHUFFLES) * 3
    kinds = set()
    for (ts, sh, bs), items in groups.items():
        labels, buffers = zip(*items)
        frames = encode(dev, buffers, ts, sh, bs, flags)
        for label, data, f in zip(labels, buffers, frames):
            assert f == host(data, ts, sh, bs, flags), label
            kinds.add((f[2] >> 5, f[2] & 0x02))
        assert decode(dev, frames) == list(buffers), (ts, sh, bs)
    assert kinds == {(3, 0), (3, 2)}
    assert _lib.lib().zh_debug_blosc_encode_kernel_ms() > 0


@pytest.mark.parametrize("flags", be.FLAGS)
@pytest.mark.parametrize("ts,sh,bs", [(4, 1, 0), (2, 2, 512), (1, 0, 256), (8, 1, 1024)])
def test_three_hundred_small_frames(dev, ts, sh, bs, flags):
    """More frames than one table row of 256 bytes and more pieces than one workgroup's four; with
    typesize 8 and blocks of 1 KiB (128 elements: split) a block has eight streams."""
    rng = np.random.default_rng(3)
    buffers = []
    for k in range(300):
        n = int(rng.integers(0, 1400))
        a = (np.arange(n) // (1 + k % 7) % (2 + k % 50)).astype(np.uint8)
        if k % 11 == 0:
            a = rng.integers(0, 256, n, dtype=np.uint8)   # stored raw or MEMCPYED
        buffers.append(a.tobytes())
    frames = encode(dev, buffers, ts, sh, bs, flags)
    for k, (data, f) in enumerate(zip(buffers, frames)):
        assert f == host(data, ts, sh, bs, flags), k
    assert decode(dev, frames) == buffers
    assert {f[2] & 0x02 for f in frames} == {0, 2}
    if ts >= 8:
        assert any(r[0] == 0 and r[5] == ts for f in frames if not f[2] & 0x02
                   for r in _lib.blosc_streams(f, bz.FLAG))


@pytest.mark.parametrize("flags", be.FLAGS)
@pytest.mark.parametrize("bs", be.CAPACITIES)
def test_every_block_capacity(dev, bs, flags):
    """The shuffle kernel is built for blocks of at most 16, 32 and 64 KiB; a slab takes the
    smallest form that holds its blocks: block sizes at and next to each threshold, streams of one
    to four 16 KiB pieces and of a piece plus four bytes."""
    rng = np.random.default_rng(41)
    noise = rng.integers(0, 256, 16 << 10, dtype=np.uint8).tobytes()
    buffers = [bi.img(), bi.ramp(), bi.smooth(100001), bytes(70000), b"\xff" * (64 << 10),
               noise + bytes(48 << 10), bytes(48 << 10) + noise]
    for ts, sh in ((2, 1), (4, 2), (1, 0)):
        frames = encode(dev, buffers, ts, sh, bs, flags)
        for k, (data, f) in enumerate(zip(buffers, frames)):
            assert f == host(data, ts, sh, bs, flags), (bs, ts, sh, k)
        assert decode(dev, frames) == buffers


@pytest.mark.parametrize("flags", be.FLAGS)
def test_multi_segment_streams(dev, flags):
    """The multi-segment inputs of the host test: the 0xFF stream, stored and fixed segments in
    one stream, the Adler-32's stream lengths."""
    groups = {}
    for label, data, ts, sh, bs in be.multi_segment():
        groups.setdefault((ts, sh, bs), []).append((label, data))
    for (ts, sh, bs), items in groups.items():
        labels, buffers = zip(*items)
        frames = encode(dev, buffers, ts, sh, bs, flags)
        for label, data, f in zip(labels, buffers, frames):
            assert f == host(data, ts, sh, bs, flags), label
        assert decode(dev, frames) == list(buffers), (ts, sh, bs)


def test_edges(dev):
    for flags in be.FLAGS:
        out, rows = dev.blosc_encode_batch_raw([], 4, 1, flags=flags)
        assert rows == []
        assert encode(dev, [b"", b"", b""], 4, 1, 0, flags) == [host(b"", 4, 1, 0, flags)] * 3
        with pytest.raises(_lib.ZhError) as e:
            dev.blosc_encode_batch_raw([(0, 0)], 0, 1, flags=flags)
        assert e.value.status == bf.ZH_EINVAL
    up = Uploaded(dev, [bi.smooth(1000)])
    try:
        for flags in be.BAD_FLAGS:
            with pytest.raises(_lib.ZhError) as e:
                dev.blosc_encode_batch_raw(up.sources, 4, 1, flags=flags)
            assert e.value.status == bf.ZH_EINVAL
        with pytest.raises(_lib.ZhError):
            dev.blosc_encode_batch_raw(up.sources, 4, 1, dynamic=True)
        # flags 0 and 1 are the writers of before
        assert dev.blosc_encode_batch(up.sources, 4, 1) == \
            [_lib.blosc_compress(bi.smooth(1000), 4, 1)]
        assert dev.blosc_encode_batch(up.sources, 4, 1, zstd=True) == \
            [_lib.blosc_compress(bi.smooth(1000), 4, 1, zstd=True)]
    finally:
        up.free()


# ---- array level -----------------------------------------------------------------------------
def _sharded(loc):
    return lambda c: c.withSharding(
        [4, 8, 16], lambda c1: c1.withTranspose([2, 0, 1]).withBytes("BIG")
        .withBlosc("zlib", "shuffle"), loc)


CASES = {
    "unsharded": (z.Array,
                  lambda: _v3(lambda c: c.withBytes("LITTLE").withBlosc("zlib", "shuffle")), DATA3),
    "sharded-end": (z.Array, lambda: _v3(_sharded("end")), DATA3),
    "sharded-start": (z.Array, lambda: _v3(_sharded("start")), DATA3),
    "v2": (v2.Array, lambda: (v2.ArrayMetadataBuilder().withShape(15, 10)
                              .withDataType(v2.DataType.UINT32).withChunks(4, 5).withFillValue(2)
                              .withBloscCompressor("zlib", "shuffle", 6).build()), DATA2),
}


def _memcpyed(b):
    return b[2] & 0x02 and len(b) == int.from_bytes(b[4:8], "little") + 16


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("kind", ["memory", "files"])
@pytest.mark.parametrize("case", list(CASES))
def test_array_write_device_route(dev, case, kind, mode, tmp_path, monkeypatch):
    cls, meta, data = CASES[case]
    monkeypatch.setenv("ZH_BLOSC_ZLIB_ENCODE", mode)
    monkeypatch.setenv("ZH_BLOSC_ENCODE_DEVICE", "1")
    a = cls.create(_store(kind, tmp_path, "dev"), meta())
    a.write(None, data)
    info = a.last_write_info
    assert info["blosc_device_frames"] > 0 and info["blosc_host_frames"] == 0
    assert info["raw_bytes"] >= data.nbytes and info["stored_bytes"] < info["raw_bytes"]
    stored = _objects(a)
    assert info["stored_bytes"] == sum(len(b) for b in stored.values())
    if case in ("unsharded", "v2"):       # a chunk is one frame: compressor code 3, not MEMCPYED
        assert all(o[2] >> 5 == 3 for o in stored.values())
        assert any(not o[2] & 0x02 for o in stored.values())
    # full and partial reads, the zlib streams decoded on the host and on the device
    for route in ("0", "1"):
        monkeypatch.setenv("ZH_BLOSC_ZLIB_DEVICE", route)
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
    # with the switch unset: the MEMCPYED frames of before
    monkeypatch.delenv("ZH_BLOSC_ZLIB_ENCODE")
    monkeypatch.delenv("ZH_BLOSC_ENCODE_DEVICE")
    c = cls.create(_store(kind, tmp_path, "plain"), meta())
    c.write(None, data)
    info = c.last_write_info
    assert info["blosc_device_frames"] == 0 and info["blosc_host_frames"] > 0
    assert info["stored_bytes"] > info["raw_bytes"]
    if case in ("unsharded", "v2"):       # a chunk is one frame
        assert all(_memcpyed(o) for o in _objects(c).values())
    np.testing.assert_array_equal(cls.open(c.storeHandle).read(), data)


@pytest.mark.parametrize("case", list(CASES))
def test_partial_write_deletes_all_fill_chunks(dev, case, tmp_path, monkeypatch):
    cls, meta, data = CASES[case]
    monkeypatch.setenv("ZH_BLOSC_ZLIB_ENCODE", "1")
    monkeypatch.setenv("ZH_BLOSC_ENCODE_DEVICE", "1")
    a = cls.create(_store("files", tmp_path, "p"), meta())
    a.write(None, data)
    assert all(v is not None for v in _objects(a).values())
    fill = a.metadata.fill_value
    cs = a.metadata.chunk_shape
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
