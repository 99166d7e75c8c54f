"""Batched device decode of gzip members (zh_gzip_decode_batch, zarr-java_amd/csrc/
zh_gzip_dec_kernels.hip) and the read path that uses it (ZH_GZIP_DEVICE).  Every expected value is
the source data and zh_gzip_decompress on the same member, bit-exact; the array reads are compared
with the host route (ZH_GZIP_DEVICE=0, zlib) and with the source data.  Only the fixed corrupt
list of gzip_dec_inputs runs on the device, each entry first shown rejected on the CPU."""
import struct

import numpy as np
import pytest

import gzip_dec_inputs as gi
import zarrhip as z
from zarrhip import _abi as A
from zarrhip import _lib

pytestmark = pytest.mark.gpu


def decode_batch(dev, frames):
    """zh_gzip_decode_batch → ([decoded bytes per frame], [where per frame])."""
    ptr, rows = dev.gzip_decode_batch(frames)
    try:
        total = max([o + n for o, n, _ in rows] + [1])
        raw = dev.d2h(ptr, total)
    finally:
        dev.free(ptr)
    return [bytes(raw[o:o + n]) for o, n, _ in rows], [w for _, _, w in rows]


# ---- the valid set ------------------------------------------------------------------------------
def test_valid_set_in_one_batch(dev):
    valid = gi.valid()
    got, where = decode_batch(dev, [m for _, _, m in valid])
    for (label, data, m), g, w in zip(valid, got, where):
        # where == 0: decoded by the kernel, and not flagged and rescued by the host decoder
        # (zh_gzip_decode_batch sets where = 1 on a member it had to hand over)
        assert w == 0, label
        assert g == data, label
        assert g == gi.host_decode(m)[1], label
    assert _lib.lib().zh_debug_gzip_decode_kernel_ms() > 0


def test_single_member_batches_and_host_routed_frames(dev):
    small = [v for v in gi.valid() if len(v[1]) <= 1000]
    assert len(small) >= 8
    for label, data, m in small:
        got, where = decode_batch(dev, [m])
        assert (got, where) == ([data], [0]), label
    routed = gi.host_routed()
    frames, keep = gi.frames_of(routed)
    a, b = small[0], small[-1]
    mixed = [a[2]] + frames + [b[2]]
    got, where = decode_batch(dev, mixed)
    assert where == [0] + [1] * len(routed) + [0]
    assert got == [a[1]] + [d for _, d, _, _ in routed] + [b[1]]
    # one frame between device frames, every position
    for k, (label, data, _, _) in enumerate(routed):
        got, where = decode_batch(dev, [a[2], frames[k], b[2]])
        assert (got, where) == ([a[1], data, b[1]], [0, 1, 0]), label
    ptr, rows = dev.gzip_decode_batch([])
    dev.free(ptr)
    assert rows == []


# ---- corrupt members ----------------------------------------------------------------------------
def test_corrupt_members_are_reported_with_the_host_text(dev):
    good = [gi.valid()[k][2] for k in (1, 3)]
    corrupt = gi.corrupt()
    texts = {}
    for kind, m in corrupt:
        st, _, msg = gi.host_decode(m)
        assert st == A.ZH_EDATA and msg == gi.TEXTS[kind], kind   # rejected cleanly on the CPU
        texts[kind] = msg
        with pytest.raises(_lib.ZhError) as e:
            dev.gzip_decode_batch([good[0], good[1], m, good[0]])
        assert (e.value.status, str(e.value)) == (st, msg), kind
    # the first bad frame in batch order is the one named: a kernel-flagged member, a CRC
    # mismatch and a header the plan refuses, in every order of two
    bad = dict(corrupt)
    picks = ["distance too far back", "CRC mismatch", "FHCRC mismatch"]
    for first in picks:
        for second in picks:
            if first == second:
                continue
            with pytest.raises(_lib.ZhError) as e:
                dev.gzip_decode_batch([good[0], bad[first], good[1], bad[second]])
            assert str(e.value) == texts[first], (first, second)
    # the context decodes a good batch afterwards
    got, where = decode_batch(dev, good * 3)
    assert where == [0] * 6 and got == [gi.host_decode(m)[1] for m in good * 3]


# ---- array level --------------------------------------------------------------------------------
def _source(shape):
    rng = np.random.default_rng(11)
    base = np.add.outer(np.add.outer(np.arange(shape[0]) * 700, np.arange(shape[1]) * 40),
                        np.arange(shape[2]))
    return ((base + rng.integers(0, 3, shape)) % 65536).astype(np.uint16)


SHAPE, CHUNK = [24, 32, 64], [8, 16, 32]
# the whole array; an unaligned part; the slab that holds the missing chunk
REGIONS = [([0, 0, 0], SHAPE), ([3, 5, 7], [13, 20, 41]), ([16, 0, 0], [8, 32, 64])]


def _codecs(kind):
    if kind == "plain":
        return lambda c: c.withBytes("BIG").withGzip(5)
    loc = "start" if kind == "shard_start" else "end"
    return lambda c: c.withSharding(
        [4, 8, 16], lambda c1: c1.withTranspose([2, 0, 1]).withBytes("LITTLE").withGzip(5), loc)


def _array(kind, writer, data, store, monkeypatch):
    m = (z.ArrayMetadataBuilder().withShape(*SHAPE).withDataType(z.DataType.UINT16)
         .withChunkShape(*CHUNK).withFillValue(7).withCodecs(_codecs(kind)).build())
    h = store.resolve(kind + writer)
    a = z.Array.create(h, m)
    assert a._gzip_chain()
    monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", "1" if writer == "own" else "0")
    a.write(None, data)
    assert a.last_write_info["gzip_device_frames" if writer == "own" else "gzip_host_frames"] > 0
    monkeypatch.delenv("ZH_GZIP_ENCODE_DEVICE")
    coords = a._chunk_coords([0, 0, 0], SHAPE)
    a._handle(coords[-1]).delete()   # a missing chunk: the fill value
    return z.Array.open(h)


@pytest.mark.parametrize("writer", ["own", "zlib"])
@pytest.mark.parametrize("kind", ["plain", "shard_start", "shard_end"])
def test_array_read_routes(dev, kind, writer, tmp_path, monkeypatch):
    data = _source(SHAPE)
    store = z.MemoryStore() if kind == "shard_end" else z.FilesystemStore(tmp_path)
    a = _array(kind, writer, data, store, monkeypatch)
    want_all = data.copy()
    last = a._chunk_coords([0, 0, 0], SHAPE)[-1]
    want_all[tuple(slice(c * k, (c + 1) * k) for c, k in zip(last, CHUNK))] = 7
    for off, shp in REGIONS:
        sl = tuple(slice(o, o + n) for o, n in zip(off, shp))
        monkeypatch.setenv("ZH_GZIP_DEVICE", "0")
        host = a.read(off, shp)
        t = a.last_read_timing
        assert t["gzip_device_frames"] == 0 and t["gzip_host_frames"] > 0
        monkeypatch.setenv("ZH_GZIP_DEVICE", "2")
        got = a.read(off, shp)
        t = a.last_read_timing
        assert t["gzip_device_frames"] > 0 and t["gzip_host_frames"] == 0
        assert t["zstd_device_frames"] == 0 and t["blosc_device_frames"] == 0
        np.testing.assert_array_equal(got, host)
        np.testing.assert_array_equal(got, want_all[sl])
        nb = got.nbytes
        d = dev.malloc(nb)
        try:
            a.read_device(off, shp, d, dev)
            back = np.frombuffer(dev.d2h(d, nb), np.uint16).reshape(shp)
        finally:
            dev.free(d)
        np.testing.assert_array_equal(back, got)


class _FailingStore(z.MemoryStore):
    """A MemoryStore whose reads of one key fail."""
    bad = None

    def get(self, keys, start=None, end=None):
        if self.bad is not None and tuple(keys) == tuple(self.bad):
            raise z.StoreException.read_failed("memory", keys, OSError("injected"))
        return super().get(keys, start, end)


def test_errors_through_array_read(dev, monkeypatch):
    data = _source(SHAPE)
    bad = dict(gi.corrupt())["distance too far back"]
    assert gi.host_decode(bad)[0] == A.ZH_EDATA
    monkeypatch.setenv("ZH_GZIP_DEVICE", "2")
    for kind in ("plain", "shard_end"):
        store = _FailingStore()
        a = _array(kind, "zlib", data, store, monkeypatch)
        coords = a._chunk_coords([0, 0, 0], SHAPE)
        mid = coords[len(coords) // 2]
        if kind == "plain":
            a._handle(mid).set(bad)
        else:                           # the first stored inner chunk's bytes become the bad member
            sh = bytearray(a._handle(mid).read())
            n_in = a._n_inner()
            o, nb = struct.unpack("<QQ", bytes(sh[len(sh) - 16 * n_in - 4:])[:16])
            assert nb >= len(bad)
            sh[o:o + len(bad)] = bad
            ib = struct.pack("<QQ", o, len(bad)) + bytes(sh[len(sh) - 16 * n_in - 4 + 16:-4])
            a._handle(mid).set(bytes(sh[:len(sh) - 16 * n_in - 4]) +
                               a.chain.index_codecs[1].encode(ib))
        with pytest.raises(z.ZarrException) as e:
            a.read()
        assert str(e.value) == "Error in decoding gzip.", kind
        # a store error in an earlier chunk is reported first
        store.bad = a._handle(coords[1]).keys
        with pytest.raises(Exception) as e:
            a.read()
        assert "injected" in str(e.value), kind
        store.bad = None


def test_default_route_follows_the_rule(dev, monkeypatch):
    """ZH_GZIP_DEVICE unset or 1: a read goes to the device when it has GZIP_DEVICE_MIN_FRAMES
    members; None sends nothing."""
    from zarrhip import array as zarray
    assert zarray.GZIP_DEVICE_DEFAULT == "1"
    data = _source(SHAPE)
    a = _array("shard_end", "zlib", data, z.MemoryStore(), monkeypatch)
    n_read = 8 * a._n_inner()            # [16, 32, 64]: 2 x 2 x 2 shards
    assert n_read == 64
    for floor, device in ((None, False), (n_read, True), (n_read + 1, False)):
        monkeypatch.setattr(zarray, "GZIP_DEVICE_MIN_FRAMES", floor)
        for mode in (None, "1"):
            if mode is None:
                monkeypatch.delenv("ZH_GZIP_DEVICE", raising=False)
            else:
                monkeypatch.setenv("ZH_GZIP_DEVICE", mode)
            got = a.read([0, 0, 0], [16, 32, 64])
            np.testing.assert_array_equal(got, data[:16])
            t = a.last_read_timing
            assert (t["gzip_device_frames"] > 0) == device
            assert (t["gzip_host_frames"] > 0) == (not device)
