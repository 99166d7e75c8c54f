"""Seeded, model-based fuzz of Array.write / Array.read over compressed chains with the frames made
on the device (ZH_BLOSC_ENCODE_DEVICE / ZH_ZSTD_ENCODE_DEVICE = 1).  The cases are
compressed_cases.random_case's; what the store must hold after each write is kept with the C
oracle (chunk bytes, shard layout, elision), and every stored frame is decoded by libzstd / liblz4
(independent_codecs.py): nothing is compared with the library's own codecs except the host-route
twin, which must store the same bytes.  Everything is byte-exact."""
import numpy as np
import pytest

import compressed_cases as cc
import independent_codecs as ic
import zarrhip as z
from zarrhip import v2

pytestmark = pytest.mark.gpu

COUNTERS = ("blosc_device_frames", "blosc_host_frames", "zstd_device_frames", "zstd_host_frames")


def _store(kind, tmp_path, name):
    return (z.MemoryStore() if kind == "memory" else z.FilesystemStore(tmp_path)).resolve(name)


def _frames(a, obj, want, ax):
    """The frames of one stored object against the units of the oracle's object `want`: decoded
    by the independent decoders only.  A shard's index is read with the case's own endianness and
    crc32c; its frames and its index tile the object exactly.  Returns the number of frames."""
    if not a.chain.chain["sharded"]:
        pairs = [(obj, want)]
    else:
        ents, isz = cc.shard_entries(a, obj)
        wunits = cc.units(a, want)
        assert [e is None for e in ents] == [u is None for u in wunits]
        start = ax["index_location"] == "start"
        lo, hi = (isz, len(obj)) if start else (0, len(obj) - isz)
        end = lo
        for off, nb in sorted(e for e in ents if e is not None):
            assert off >= end and nb > 0 and off + nb <= hi      # inside, never overlapping
            end = off + nb
        assert sum(e[1] for e in ents if e is not None) + isz == len(obj)
        pairs = [(obj[e[0]:e[0] + e[1]], u) for e, u in zip(ents, wunits) if e is not None]
    for f, raw in pairs:
        if ax["codec"] == "blosc":
            assert ic.blosc_lz4_decode(f) == raw
            assert f[3] == ax["frame_typesize"]
            if not f[2] & 0x02:
                assert bool(f[2] & 0x01) == (ax["shuffle"] == "shuffle")
                assert bool(f[2] & 0x04) == (ax["shuffle"] == "bitshuffle")
        else:
            assert ic.zstd_decode(f, len(raw)) == raw
            assert ic.zstd_has_checksum(f) == ax["checksum"]
    return len(pairs)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(cc.bits(got), cc.bits(want), err_msg=str(what))


def run_case(case, tmp_path, monkeypatch, seed=0):
    ax = case.axes
    kind = ax["codec"]
    env = f"ZH_{kind.upper()}_ENCODE_DEVICE"
    monkeypatch.setenv(env, "1")
    a = case.cls.create(_store(case.store, tmp_path, "dev"), case.meta())
    assert a._encode_device() == kind
    b = case.cls.create(_store(case.store, tmp_path, "host"), case.meta())
    model = cc.Model(a)
    rng = np.random.default_rng(50_000 + seed)
    shape = model.shape
    for k, (off, data) in enumerate(case.steps):
        monkeypatch.setenv(env, "1")
        a.write(off, data)
        info = a.last_write_info
        monkeypatch.setenv(env, "0")
        b.write(off, data)
        changed = model.write(off, data)
        # 1. keys
        stored = cc.stored_objects(a)
        assert {c for c, o in stored.items() if o is None} == \
            {c for c, o in model.objs.items() if o is None}, (k, "keys")
        # 2. stored objects
        nframes = {c: _frames(a, o, model.objs[c], ax) for c, o in stored.items() if o is not None}
        # 3. write info: the frames and bytes of the objects this step set
        mine = [c for c, o in changed.items() if o is not None]
        assert info[kind + "_device_frames"] == sum(nframes[c] for c in mine), (k, info)
        assert [info[n] for n in COUNTERS if n != kind + "_device_frames"] == [0, 0, 0], (k, info)
        assert info["stored_bytes"] == sum(len(stored[c]) for c in mine), (k, info)
        # 4. reads of a freshly opened array: the whole array and two regions, bit for bit
        want = model.read()
        regions = [(None, None)]
        for _ in range(2):
            o = [int(rng.integers(0, s)) for s in shape]
            regions.append((o, [int(rng.integers(1, s - x + 1)) for s, x in zip(shape, o)]))
        for route in (("0", "1") if kind == "blosc" else ("1",)):
            monkeypatch.setenv("ZH_BLOSC_DEVICE", route)
            r = case.cls.open(a.storeHandle)
            for o, n in regions:
                sl = tuple(slice(x, x + m) for x, m in zip(o, n)) if o is not None else ()
                _same(r.read(o, n), want[sl], (k, route, o, n))
        # 5. the host route stores the same bytes
        assert cc.stored_objects(b) == stored, (k, "host route")
        hinfo = b.last_write_info
        assert hinfo[kind + "_host_frames"] == info[kind + "_device_frames"], (k, hinfo)
        assert hinfo[kind + "_device_frames"] == 0, (k, hinfo)


@pytest.mark.parametrize("seed", cc.SEEDS)
def test_compressed_write_fuzz(dev, seed, tmp_path, monkeypatch):
    run_case(cc.random_case(seed), tmp_path, monkeypatch, seed)


def test_no_fill_value_zero_chunk_takes_the_device_route(dev, tmp_path, monkeypatch):
    """v2 "fill_value": null never deletes a key: a chunk of zeros is stored, and its frame is
    made on the device with the others (it used to be compressed on the host, and counted so,
    while the write's other frames came from the device)."""
    data = (np.arange(12 * 10, dtype="<u4").reshape(12, 10) % 7 + 1)
    data[4:8] = 0                                      # chunk rows 1: two chunks of zeros

    def meta():
        return (v2.ArrayMetadataBuilder().withShape(12, 10).withDataType(v2.DataType.UINT32)
                .withChunks(4, 5).withFillValue(None).withZstdCompressor(3, True).build())
    ax = dict(codec="zstd", checksum=True)
    run_case(cc.Case(meta, v2.Array, np.dtype("<u4"), "memory",
                     [(None, data), ([4, 0], np.zeros((8, 5), "<u4"))], ax),
             tmp_path, monkeypatch)
