"""Batched device decode of zstd frames (zh_zstd_decode_batch, zarr-java_amd/csrc/
zh_zstd_dec_kernels.hip) and the read path that uses it (ZH_ZSTD_DEVICE).  Every expected value is
the source data and zh_zstd_decompress on the same frame, bit-exact; the array reads are compared
with the host route (ZH_ZSTD_DEVICE=0) and with the source data."""
import os
import struct

import numpy as np
import pytest

import zarrhip as z
import zstd_dec_inputs as zi
from helpers import GOLDEN
from zarrhip import _abi as A
from zarrhip import _lib

pytestmark = pytest.mark.gpu

OME_ARRAYS = ["v0.5/0", "v0.5/1", "v0.5/labels/nuclei/0", "v0.5_hcs/A/1/0/0"]


def decode_batch(dev, frames):
    """zh_zstd_decode_batch → ([decoded bytes per frame], [where per frame])."""
    ptr, rows = dev.zstd_decode_batch(frames)
    try:
        total = max([o + n for o, n, _ in rows] + [1])
        raw = dev.d2h(ptr, total)
    finally:
        dev.free(ptr)
    return [bytes(raw[o:o + n]) for o, n, _ in rows], [w for _, _, w in rows]


# ---- the valid matrix ---------------------------------------------------------------------------
def test_valid_set_in_one_batch(dev):
    valid = zi.valid()
    got, where = decode_batch(dev, [f for _, _, f in valid])
    for (label, data, f), g, w in zip(valid, got, where):
        # where == 0: decoded by the kernel, and not flagged and rescued by the host decoder
        # (zh_zstd_decode_batch sets where = 1 on a frame it had to hand over)
        assert w == 0, label
        assert g == data, label
        assert g == zi.host_decode(f)[1], label


def test_single_frame_batches_and_host_routed_frames(dev):
    small = [v for v in zi.valid() if len(v[1]) <= 1000]
    assert len(small) >= 8
    for label, data, f in small:
        got, where = decode_batch(dev, [f])
        assert (got, where) == ([data], [0]), label
    routed = zi.host_routed()
    mixed = [small[0][2]] + [f for _, _, f in routed] + [small[1][2]]
    got, where = decode_batch(dev, mixed)
    assert where == [0] + [1] * len(routed) + [0]
    assert got == [small[0][1]] + [d for _, d, _ in routed] + [small[1][1]]
    ptr, rows = dev.zstd_decode_batch([])
    dev.free(ptr)
    assert rows == []


# ---- corrupt frames -----------------------------------------------------------------------------
def test_corrupt_frames_are_reported_with_the_host_text(dev):
    good = [zi.valid()[k][2] for k in (20, 25)]
    corrupt = zi.corrupt() + [("impossible content size", zi.impossible_size())]
    texts = []
    for kind, f in corrupt:
        st, _, msg = zi.host_decode(f)
        assert st != A.ZH_OK, kind           # rejected cleanly on the CPU (test_zstd_batch_host)
        texts.append(msg)
        with pytest.raises(_lib.ZhError) as e:
            dev.zstd_decode_batch([good[0], good[1], f, good[0]])
        assert (e.value.status, str(e.value)) == (st, msg), kind
    # the first bad frame in batch order is the one named: a kernel-flagged frame, a checksum
    # mismatch and a host-decoded frame in every order of two
    names = [k for k, _ in corrupt]
    picks = [names.index("literals overrun"), names.index("checksum mismatch"),
             names.index("block larger than 128 KiB")]
    for a in picks:
        for b in picks:
            if a == b:
                continue
            with pytest.raises(_lib.ZhError) as e:
                dev.zstd_decode_batch([good[0], corrupt[a][1], good[1], corrupt[b][1]])
            assert str(e.value) == texts[a]
    # a size query failure comes first only when no earlier frame is bad
    with pytest.raises(_lib.ZhError) as e:
        dev.zstd_decode_batch([good[0], corrupt[picks[0]][1], b"\x27" + good[1][1:]])
    assert str(e.value) == texts[picks[0]]
    with pytest.raises(_lib.ZhError) as e:
        dev.zstd_decode_batch([good[0], b"\x27" + good[1][1:], corrupt[picks[0]][1]])
    assert str(e.value) == "zstd: unknown frame magic"
    # the context decodes a good batch afterwards
    got, where = decode_batch(dev, good * 3)
    assert where == [0] * 6 and got == [zi.host_decode(f)[1] for f in good * 3]


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
        return lambda c: c.withBytes("BIG").withZstd(3, True)
    loc = "start" if kind == "shard_start" else "end"
    return lambda c: c.withSharding(
        [4, 8, 16], lambda c1: c1.withTranspose([2, 0, 1]).withBytes("LITTLE").withZstd(5, False),
        loc)


def _recompress(frame):
    st, raw, msg = zi.host_decode(frame)
    assert st == A.ZH_OK, msg
    return zi.libzstd(raw, 3)


def _rewrap_shard(a, shard):
    """The shard with every inner chunk's frame replaced by libzstd's frame of the same bytes."""
    ch = a.chain.chain
    n_in = a._n_inner()
    isz = 16 * n_in + 4
    start = ch["index_location"] == A.ZH_INDEX_START
    idx = shard[:isz] if start else shard[len(shard) - isz:]
    pos = isz if start else 0
    payload, new = b"", []
    for k in range(n_in):
        o, nb = struct.unpack("<QQ", idx[16 * k:16 * k + 16])
        if o == 2 ** 64 - 1:
            new.append((o, nb))
            continue
        f = _recompress(shard[o:o + nb])
        new.append((pos + len(payload), len(f)))
        payload += f
    ib = b"".join(struct.pack("<QQ", *e) for e in new)
    ib = a.chain.index_codecs[1].encode(ib)
    return ib + payload if start else payload + ib


def _array(kind, writer, data, store):
    m = (z.ArrayMetadataBuilder().withShape(*SHAPE).withDataType(z.DataType.UINT16)
         .withChunkShape(*CHUNK).withFillValue(7).withCodecs(_codecs(kind)).build())
    h = store.resolve(kind + writer)
    a = z.Array.create(h, m)
    assert a._zstd_chain()
    a.write(None, data)
    coords = a._chunk_coords([0, 0, 0], SHAPE)
    if writer == "libzstd":        # the store keys set here, frames by libzstd
        for c in coords:
            b = bytes(a._handle(c).read())
            a._handle(c).set(_recompress(b) if kind == "plain" else _rewrap_shard(a, b))
    a._handle(coords[-1]).delete()   # a missing chunk: the fill value
    return z.Array.open(h)


@pytest.mark.parametrize("writer", ["own", "libzstd"])
@pytest.mark.parametrize("kind", ["plain", "shard_start", "shard_end"])
def test_array_read_routes(dev, kind, writer, tmp_path, monkeypatch):
    data = _source(SHAPE)
    store = z.MemoryStore() if kind == "shard_end" else z.FilesystemStore(tmp_path)
    a = _array(kind, writer, data, store)
    want_all = data.copy()
    last = a._chunk_coords([0, 0, 0], SHAPE)[-1]
    want_all[tuple(slice(c * k, (c + 1) * k) for c, k in zip(last, CHUNK))] = 7
    for off, shp in REGIONS:
        sl = tuple(slice(o, o + n) for o, n in zip(off, shp))
        monkeypatch.setenv("ZH_ZSTD_DEVICE", "0")
        host = a.read(off, shp)
        t = a.last_read_timing
        assert t["zstd_device_frames"] == 0 and t["zstd_host_frames"] > 0
        assert t["blosc_device_frames"] == 0 and t["blosc_host_frames"] == 0
        monkeypatch.setenv("ZH_ZSTD_DEVICE", "2")
        got = a.read(off, shp)
        t = a.last_read_timing
        assert t["zstd_device_frames"] > 0 and t["zstd_host_frames"] == 0
        assert t["blosc_device_frames"] == 0 and t["blosc_host_frames"] == 0
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


@pytest.mark.parametrize("name", OME_ARRAYS)
def test_ome_arrays_device_route_equals_host_route(dev, name, monkeypatch):
    h = z.FilesystemStore(os.path.join(GOLDEN, "ome_zstd")).resolve(*name.split("/"))
    a = z.Array.open(h)
    shape = list(a.metadata.shape)
    off = [s // 3 for s in shape]
    shp = [max(1, s - o - 1) for s, o in zip(shape, off)]
    monkeypatch.setenv("ZH_ZSTD_DEVICE", "0")
    want, want_part = a.read(), a.read(off, shp)
    assert a.last_read_timing["zstd_device_frames"] == 0
    assert a.last_read_timing["zstd_host_frames"] > 0
    staged = a.staged_bytes
    monkeypatch.setenv("ZH_ZSTD_DEVICE", "2")
    b = z.Array.open(h)
    got = b.read()
    assert b.last_read_timing["zstd_device_frames"] > 0
    assert b.last_read_timing["zstd_host_frames"] == 0
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(b.read(off, shp), want_part)
    assert b.staged_bytes == staged           # the compressed bytes, as on the host route


class _FailingStore(z.MemoryStore):
    """A MemoryStore whose reads of one key fail."""
    bad = None

    def get(self, keys, start=None, end=None):
        if self.bad is not None and tuple(keys) == tuple(self.bad):
            raise z.StoreException.read_failed("memory", keys, OSError("injected"))
        return super().get(keys, start, end)


def test_errors_through_array_read_are_the_host_route_errors(dev, monkeypatch):
    data = _source(SHAPE)
    names = [k for k, _ in zi.corrupt()]
    bad = zi.corrupt()[names.index("literals overrun")][1]
    for kind in ("plain", "shard_end"):
        store = _FailingStore()
        a = _array(kind, "own", data, store)
        coords = a._chunk_coords([0, 0, 0], SHAPE)
        mid = coords[len(coords) // 2]
        if kind == "plain":
            a._handle(mid).set(bad)
        else:                           # the first stored inner chunk's bytes become the bad frame
            sh = bytearray(a._handle(mid).read())
            n_in = a._n_inner()
            o, nb = struct.unpack("<QQ", bytes(sh[len(sh) - 16 * n_in - 4:])[:16])
            assert nb >= len(bad)
            sh[o:o + len(bad)] = bad
            ib = struct.pack("<QQ", o, len(bad)) + bytes(sh[len(sh) - 16 * n_in - 4 + 16:-4])
            a._handle(mid).set(bytes(sh[:len(sh) - 16 * n_in - 4]) +
                               a.chain.index_codecs[1].encode(ib))
        seen = []
        for route in ("0", "2"):
            monkeypatch.setenv("ZH_ZSTD_DEVICE", route)
            with pytest.raises(z.ZarrException) as e:
                a.read()
            seen.append((type(e.value), str(e.value)))
        assert seen[0] == seen[1], kind
        assert seen[0][1] == "Error in decoding zstd: zstd: sequence reads past the literals"
        # a store error in an earlier chunk comes first, on both routes
        store.bad = a._handle(coords[1]).keys
        seen = []
        for route in ("0", "2"):
            monkeypatch.setenv("ZH_ZSTD_DEVICE", route)
            with pytest.raises(Exception) as e:
                a.read()
            seen.append((type(e.value), str(e.value)))
        assert seen[0] == seen[1], kind
        assert "injected" in seen[0][1]
        store.bad = None


def test_default_route_is_the_host_route(dev, monkeypatch):
    """ZH_ZSTD_DEVICE unset or 1: the rule of DESIGN.md sends no read to the device."""
    from zarrhip import array as zarray
    assert zarray.ZSTD_DEVICE_DEFAULT == "1" and zarray.ZSTD_DEVICE_MIN_FRAMES is None
    data = _source(SHAPE)
    a = _array("shard_end", "own", data, z.MemoryStore())
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("ZH_ZSTD_DEVICE", raising=False)
        else:
            monkeypatch.setenv("ZH_ZSTD_DEVICE", mode)
        got = a.read([0, 0, 0], [16, 32, 64])
        np.testing.assert_array_equal(got, data[:16])
        t = a.last_read_timing
        assert t["zstd_device_frames"] == 0 and t["zstd_host_frames"] > 0


def test_zero_length_chunk_is_the_host_route_error(dev, monkeypatch):
    data = _source(SHAPE)
    a = _array("plain", "own", data, z.MemoryStore())
    a._handle(a._chunk_coords([0, 0, 0], SHAPE)[0]).set(b"")
    seen = []
    for route in ("0", "2"):
        monkeypatch.setenv("ZH_ZSTD_DEVICE", route)
        with pytest.raises(z.ZarrException) as e:
            a.read()
        seen.append((type(e.value), str(e.value)))
    assert seen[0] == seen[1] and seen[0][1] == "Error in decoding zstd: zstd: no frame"
