"""Gzip members with dynamic-Huffman segments compressed on the device (zh_gzip_encode_batch
with zh_gzip_enc_params::dynamic = 1: gzip_deflate_dyn_kernel in zarr-java_amd/csrc/
zh_gzip_enc_kernels.hip) and the write path that uses it when asked to (ZH_GZIP_ENCODE_DEVICE=2).
Every expected member is zh_gzip_compress(..., dynamic=True) on the same bytes, byte for byte;
the stored members are decoded with zlib and compared with the oracle's encoding of the chunk; the
arrays are read back through both read routes and through the device's own DEFLATE reader; with
the switch at 1 or unset every stored byte is what it was before."""
import gzip
import zlib

import numpy as np
import pytest

import gzip_dyn_inputs as gd
import gzip_enc_inputs as gi
import oracle as O
import test_gpu_gzip_encode as ge
import zarrhip as z
from zarrhip import _abi as A
from zarrhip import _lib

pytestmark = pytest.mark.gpu


def encode(dev, buffers, bs, dynamic=True, align=None):
    """zh_gzip_encode_batch twice over the uploaded buffers: the members, checked for placement
    and for being the same both times."""
    up = ge.Uploaded(dev, buffers, align)
    try:
        out, rows = dev.gzip_encode_batch_raw(up.sources, bs, dynamic=dynamic)
        out2, rows2 = dev.gzip_encode_batch_raw(up.sources, bs, dynamic=dynamic)
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
    """The matrix of test_gzip_dynamic_host.py, one batch per block size; then the same batch
    without the dynamic form: the writer of before, in the same process."""
    groups = {}
    for label, data, bs in gd.matrix():
        groups.setdefault(bs, []).append((label, data))
    assert len(groups) == len(gi.BLOCKSIZES)
    forms = set()
    for bs, items in groups.items():
        labels, buffers = zip(*items)
        members = encode(dev, buffers, bs)
        for label, data, f in zip(labels, buffers, members):
            assert f == _lib.gzip_compress(data, bs, dynamic=True), label
        forms |= {s["form"] for f in members[-12:] for s in gd.segments(f)}
        parts = _lib.gzip_encode_kernel_parts_ms()
        assert set(parts) == {"match", "coder", "crc", "gather"}
        assert all(v > 0 for v in parts.values()), parts
        for label, data, f in zip(labels, buffers, encode(dev, buffers, bs, dynamic=False)):
            assert f == _lib.gzip_compress(data, bs), label
    assert forms == {"stored", "fixed", "dynamic"}


def test_both_block_capacities(dev):
    """Block sizes at and next to the threshold between the kernel's two forms."""
    buffers = [gi.labels(), gi.text(), gi.mix(), gi.far(), gd.noisy(1 << 16),
               gi.random_bytes(70001), b""]
    for bs in (16 << 10, (16 << 10) + 4, 32 << 10):
        members = encode(dev, buffers, bs)
        for k, (data, f) in enumerate(zip(buffers, members)):
            assert f == _lib.gzip_compress(data, bs, dynamic=True), (bs, k)


def test_three_hundred_small_members(dev):
    """More blocks than one workgroup's, all three forms among them."""
    rng = np.random.default_rng(3)
    buffers = []
    for k in range(300):
        n = int(rng.integers(0, 3000))
        a = (np.arange(n) // (1 + k % 7) % (2 + k % 50)).astype(np.uint8)
        if k % 11 == 0:
            a = rng.integers(0, 256, n, dtype=np.uint8)   # stored segments
        if k % 11 == 1:
            a = rng.integers(0, 12, n, dtype=np.uint8)    # few values, no order: dynamic
        buffers.append(a.tobytes())
    members = encode(dev, buffers, 1024)
    forms = set()
    for k, (data, f) in enumerate(zip(buffers, members)):
        assert f == _lib.gzip_compress(data, 1024, dynamic=True), k
        assert zlib.decompress(f, 31) == data, k
        if k < 60:
            forms |= {s["form"] for s in gd.segments(f)}
    assert forms == {"stored", "fixed", "dynamic"}


def test_segments_one_byte_under_stored(dev):
    """Dynamic segments of exactly n + 4 bytes: the end-of-block code ends in the last byte
    before the marker, at every bit of it (test_gzip_dynamic_host.py checks that they do)."""
    rows = gd.edge_rows()
    members = encode(dev, [r[1] for r in rows], 1024)
    for (label, data, bs, _), f in zip(rows, members):
        assert f == _lib.gzip_compress(data, bs, dynamic=True), label
        assert len(f) == 20 + len(data) + 4, label
        assert zlib.decompress(f, 31) == data, label


def test_every_source_alignment(dev):
    data = gi.text()[:20011]
    members = encode(dev, [data] * 16, 0, align=list(range(16)))
    assert members == [_lib.gzip_compress(data, 0, dynamic=True)] * 16
    assert "dynamic" in {s["form"] for s in gd.segments(members[0])}


def test_params(dev):
    with pytest.raises(_lib.ZhError) as e:
        dev.gzip_encode_batch_raw([(0, 0)], 0, dynamic=2)
    assert e.value.status == A.ZH_EINVAL and "dynamic is 0 or 1" in str(e.value)
    assert encode(dev, [b"", b""], 0) == [_lib.gzip_compress(b"")] * 2


def test_code_lengths_on_the_device(dev):
    """The only place where the length limiter runs on the device: no block reaches it."""
    for label, nsym, limit, rows in gd.histogram_sets():
        assert dev.gzip_code_lengths(rows, limit) == _lib.gzip_code_lengths(rows, limit), label


# ---- array level -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ge.CODECS))
def test_array_write_device_route(dev, case, tmp_path, monkeypatch):
    data = ge._data()
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "2")
    a = z.Array.create(z.FilesystemStore(tmp_path).resolve("dev"), ge._meta(ge.CODECS[case]))
    a.write(None, data)
    info = a.last_write_info
    assert info["gzip_device_frames"] > 0 and info["gzip_host_frames"] == 0
    assert info["blosc_device_frames"] == 0 and info["zstd_device_frames"] == 0
    stored = ge._objects(a)
    assert {c for c, b in stored.items() if b is None} == ge.ABSENT
    assert info["stored_bytes"] == sum(len(b) for b in stored.values() if b is not None)
    want = dict(zip(stored, O.array_write(a.zmeta, data.tobytes(), [0, 0, 0], [16, 16, 16])))
    seen, forms = 0, set()
    for c, f, raw in ge._pairs(a, stored, want):
        assert zlib.decompress(f, 31) == raw, c
        assert f == _lib.gzip_compress(raw, dynamic=True), c          # one writer, two places
        kinds = {s["form"] for s in gd.segments(f)}
        if c == ge.NOISE:
            assert kinds == {"stored"} and len(f) == gi.bound(len(raw), 0), c
        forms |= kinds
        seen += 1
    assert seen == info["gzip_device_frames"]
    # a chunk of 256 bytes takes the dynamic form; an inner chunk of 64 bytes is too short for a
    # header of its own (test_sharded_write_with_dynamic_members has larger ones)
    if a.chain.chain["sharded"]:
        assert forms == {"stored", "fixed"}
    else:
        assert {"stored", "dynamic"} <= forms
    ge._read_both_ways(a, data, monkeypatch)
    # the device's own reader on the dynamic blocks the device wrote
    monkeypatch.setenv("ZH_GZIP_DEVICE", "2")
    r = z.Array.open(a.storeHandle)
    np.testing.assert_array_equal(r.read(), data)
    t = r.last_read_timing
    assert t["gzip_device_frames"] > 0 and t["gzip_host_frames"] == 0
    monkeypatch.delenv("ZH_GZIP_DEVICE")
    # a partial write: chunk (2, 0, 0) is read, patched and encoded on the device again
    a.write([2, 0, 0], np.zeros((3, 4, 8), np.int32))
    assert a.last_write_info["gzip_host_frames"] == 0
    assert a.last_write_info["gzip_device_frames"] > 0
    data[2:5, 0:4, 0:8] = 0
    assert {c for c, b in ge._objects(a).items() if b is None} == ge.ABSENT | {(1, 0, 0)}
    ge._read_both_ways(a, data, monkeypatch)


@pytest.mark.parametrize("location", ["start", "end"])
def test_sharded_write_with_dynamic_members(dev, location, tmp_path, monkeypatch):
    """The inner chunks of the four chains above are 64 bytes, too short for a dynamic header.
    Here a shard of (4, 8, 16) holds inner chunks of (2, 4, 8), 256 bytes: the shard route (only
    the index comes back, it is rewritten and its crc32c recomputed) with dynamic members."""
    data = ge._data()
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "2")
    meta = (z.ArrayMetadataBuilder().withShape(16, 16, 16).withDataType(z.DataType.INT32)
            .withChunkShape(4, 8, 16).withFillValue(0)
            .withCodecs(lambda c: c.withSharding(
                [2, 4, 8], lambda c1: c1.withBytes("LITTLE").withGzip(), location)).build())
    a = z.Array.create(z.FilesystemStore(tmp_path).resolve("dev"), meta)
    a.write(None, data)
    info = a.last_write_info
    assert info["gzip_device_frames"] == 64 - 2 and info["gzip_host_frames"] == 0
    stored = ge._objects(a)
    assert len(stored) == 8 and all(b is not None for b in stored.values())
    want = dict(zip(stored, O.array_write(a.zmeta, data.tobytes(), [0, 0, 0], [16, 16, 16])))
    seen, forms = 0, set()
    for c, f, raw in ge._pairs(a, stored, want):
        assert len(raw) == 256 and zlib.decompress(f, 31) == raw, c
        assert f == _lib.gzip_compress(raw, dynamic=True), c
        forms |= {s["form"] for s in gd.segments(f)}
        seen += 1
    assert seen == info["gzip_device_frames"] and forms == {"stored", "dynamic"}
    ge._read_both_ways(a, data, monkeypatch)
    monkeypatch.setenv("ZH_GZIP_DEVICE", "2")
    np.testing.assert_array_equal(z.Array.open(a.storeHandle).read(), data)
    monkeypatch.delenv("ZH_GZIP_DEVICE")
    a.write([2, 0, 0], np.zeros((3, 4, 8), np.int32))
    assert a.last_write_info["gzip_host_frames"] == 0
    assert a.last_write_info["gzip_device_frames"] > 0
    data[2:5, 0:4, 0:8] = 0
    ge._read_both_ways(a, data, monkeypatch)


@pytest.mark.parametrize("case", list(ge.CODECS))
def test_switch_one_and_unset_keep_their_bytes(dev, case, tmp_path, monkeypatch):
    data = ge._data()
    for switch in ("1", None):
        if switch is None:
            monkeypatch.delenv("ZH_GZIP_ENCODE_DEVICE", raising=False)
        else:
            monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", switch)
        a = z.Array.create(z.FilesystemStore(tmp_path).resolve(f"s{switch}"),
                           ge._meta(ge.CODECS[case]))
        a.write(None, data)
        info = a.last_write_info
        assert (info["gzip_device_frames"] > 0) == (switch == "1")
        assert (info["gzip_host_frames"] > 0) == (switch is None)
        stored = ge._objects(a)
        want = dict(zip(stored, O.array_write(a.zmeta, data.tobytes(), [0, 0, 0], [16, 16, 16])))
        for c, f, raw in ge._pairs(a, stored, want):
            if switch == "1":
                assert f == _lib.gzip_compress(raw), c
            else:
                assert f == gzip.compress(raw, ge.LEVEL[case], mtime=0), c


# ---- a seeded fuzz ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_fuzz_gzip_arrays_round_trip(dev, tmp_path, monkeypatch, seed):
    meta, a, rng = ge.random_gzip_array(seed)
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "2")
    arr = z.Array.create(z.FilesystemStore(tmp_path).resolve("a"), meta)
    arr.write(None, a)
    info = arr.last_write_info
    assert info["gzip_host_frames"] == 0, seed
    stored = ge._objects(arr)
    want = dict(zip(stored, O.array_write(arr.zmeta, a.tobytes(), [0] * a.ndim, list(a.shape))))
    seen = 0
    for c, f, raw in ge._pairs(arr, stored, want):
        assert zlib.decompress(f, 31) == raw, (seed, c)
        assert f == _lib.gzip_compress(raw, dynamic=True), (seed, c)
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
