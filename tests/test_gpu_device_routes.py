"""Seeded fuzz of the opt-in device codec routes (device_route_cases.py).  Frame level: the
frames of foreign encoders through zh_gzip_decode_batch, zh_zstd_decode_batch and
zh_blosc_decode_batch_ex(ZH_BLOSC_ZSTD_DEVICE); every frame must come back from the kernel
(where == 0: the batch calls decode on the host what a wave refuses, so a wave that wrongly refuses
valid frames shows only there) with the bytes it was made from.  Array level: random_route_case's
arrays, written by the library's host writer, its device writer or a foreign encoder, read after
every step through the route's switch: bit-identical to the oracle's model, no frame handed to the
host (last_read_timing), and for ZH_GZIP_ENCODE_DEVICE=1 / 2 every stored member the host twin's.
Valid frames only: the corrupt lists stay with the per-codec tests."""
import zlib

import numpy as np
import pytest

import blosc_zstd_inputs as bz
import compressed_cases as cc
import device_route_cases as rc
import zarrhip as z
from zarrhip import _lib

pytestmark = pytest.mark.gpu

COUNTERS = ("blosc_device_frames", "blosc_host_frames", "zstd_device_frames", "zstd_host_frames",
            "gzip_device_frames", "gzip_host_frames")


# ---- frame level ---------------------------------------------------------------------------------
def decode_batch(dev, codec, fs):
    if codec == "gzip":
        ptr, rows = dev.gzip_decode_batch(fs)
    elif codec == "zstd":
        ptr, rows = dev.zstd_decode_batch(fs)
    else:
        ptr, rows = dev.blosc_decode_batch(fs, flags=bz.FLAG)
    try:
        raw = dev.d2h(ptr, max([o + n for o, n, _ in rows] + [1]))
    finally:
        dev.free(ptr)
    return raw, rows


@pytest.mark.parametrize("codec", rc.CODECS)
def test_frames_of_foreign_encoders(dev, codec):
    nframes = nbytes = 0
    for batch in rc.batches(codec, rc.N_FRAMES):
        raw, rows = decode_batch(dev, codec, [f for _, _, f in batch])
        pos = 0
        for (label, data, _), (off, nb, where) in zip(batch, rows):
            # decoded by the kernel, not flagged by its wave and rescued by the host decoder
            assert where == 0, label
            assert (off, nb) == (pos, len(data)) and off % 256 == 0, label
            assert bytes(raw[off:off + nb]) == data, label
            pos = -(-(pos + nb) // 256) * 256
        nframes += len(batch)
        nbytes += sum(len(d) for _, d, _ in batch)
    print(f"{codec}: {nframes} frames, {nbytes} bytes decoded on the device with where == 0")


def test_constant_buffer_in_blosc_zstd_frames(dev):
    """Frames several thousand times smaller than their content (test_device_routes_host.py:
    the header's bound follows the compressor), alone and between other frames."""
    const = rc.constant_blosc_frames()
    for batch in [[c] for c in const] + [[rc.frames("blosc-zstd")[6]] + const]:
        raw, rows = decode_batch(dev, "blosc-zstd", [f for _, _, f in batch])
        for (label, data, _), (off, nb, where) in zip(batch, rows):
            assert where == 0 and bytes(raw[off:off + nb]) == data, label


# ---- array level ---------------------------------------------------------------------------------
def _store(kind, tmp_path, name):
    return (z.MemoryStore() if kind == "memory" else z.FilesystemStore(tmp_path)).resolve(name)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(cc.bits(got), cc.bits(want), err_msg=str(what))


def _members(a, obj, want, ax):
    """The gzip members of one stored object against the units of the oracle's object: decoded by
    zlib, equal to the host twin, a shard's members and index tiling the object.  Returns their
    number."""
    if not a.chain.chain["sharded"]:
        pairs = [(obj, want)]
    else:
        ents, isz = cc.shard_entries(a, obj)
        wunits = cc.units(a, want)
        assert [e is None for e in ents] == [u is None for u in wunits]
        lo, hi = (isz, len(obj)) if ax["index_location"] == "start" else (0, len(obj) - isz)
        end = lo
        for off, nb in sorted(e for e in ents if e is not None):
            assert off >= end and nb > 0 and off + nb <= hi
            end = off + nb
        assert sum(e[1] for e in ents if e is not None) + isz == len(obj)
        pairs = [(obj[e[0]:e[0] + e[1]], u) for e, u in zip(ents, wunits) if e is not None]
    for f, raw in pairs:
        assert zlib.decompress(f, 31) == raw
        assert f == _lib.gzip_compress(raw, dynamic=ax["route"] == "gzip-enc-2")
    return len(pairs)


def _reads(case, a, model, rng, dev, monkeypatch, what):
    """The whole array and two regions of a freshly opened array through the route's switch and
    with it at "0", and one read_device of the whole array."""
    ax = case.axes
    codec = rc.COUNTER[ax["route"]]
    env, on = rc.READ_SWITCH[ax["route"]]
    want = model.read()
    shape = model.shape
    regions = [(None, None)]
    for _ in range(2):
        o = [int(rng.integers(0, s)) for s in shape]
        regions.append((o, [int(rng.integers(1, s - x + 1)) for s, x in zip(shape, o)]))
    r = case.cls.open(a.storeHandle)
    decoded = 0
    for o, n in regions:
        sl = tuple(slice(x, x + m) for x, m in zip(o, n)) if o is not None else ()
        monkeypatch.setenv(env, on)
        got = r.read(o, n)
        t = r.last_read_timing
        _same(got, want[sl], what + (env, on, o, n))
        touched = rc.present_units(a, model, ax["unit"], o, n)
        # the rescue detector: no frame of the read was decoded on the host
        assert t[codec + "_host_frames"] == 0, what + (o, n, t)
        assert (t[codec + "_device_frames"] > 0) == (touched > 0), what + (o, n, t)
        if o is None:
            assert t[codec + "_device_frames"] == touched, what + (t,)
            decoded = touched
        assert [t[c] for c in COUNTERS if not c.startswith(codec)] == [0] * 4, what + (t,)
        monkeypatch.setenv(env, "0")
        _same(r.read(o, n), want[sl], what + (env, "0", o, n))
        assert r.last_read_timing[codec + "_device_frames"] == 0, what + (o, n)
    monkeypatch.setenv(env, on)
    d = dev.malloc(max(1, want.nbytes))
    try:
        r.read_device([0] * model.n, shape, d, dev)
        back = np.frombuffer(dev.d2h(d, want.nbytes), want.dtype).reshape(shape)
    finally:
        dev.free(d)
    _same(back, want, what + ("read_device",))
    return decoded, sum(len(u) for obj in model.objs.values() if obj is not None
                        for u in cc.units(a, obj) if u is not None)


def run_case(case, tmp_path, monkeypatch, dev, seed):
    ax = case.axes
    route, writer = ax["route"], ax["writer"]
    encode = route.startswith("gzip-enc")
    for env in ("ZH_ZSTD_DEVICE", "ZH_GZIP_DEVICE", "ZH_BLOSC_ZSTD_DEVICE", "ZH_BLOSC_DEVICE",
                "ZH_ZSTD_ENCODE_DEVICE", "ZH_GZIP_ENCODE_DEVICE"):
        monkeypatch.delenv(env, raising=False)
    a = case.cls.create(_store(case.store, tmp_path, "a"), case.meta())
    model = cc.Model(a)
    rng = np.random.default_rng(70_000 + seed)
    frames = nbytes = 0
    for k, (off, data) in enumerate(case.steps):
        changed = model.write(off, data)
        mine = [c for c, o in changed.items() if o is not None]
        if writer == "foreign":       # the oracle's objects, compressed and tiled on this side
            for c, obj in changed.items():
                h = a._handle(c)
                if obj is None:
                    h.delete()
                else:
                    h.set(rc.foreign_object(a, ax, obj))
        else:
            if encode:
                monkeypatch.setenv("ZH_GZIP_ENCODE_DEVICE", route[-1])
                assert a._encode_device() == "gzip" and a._gzip_dynamic() == (route[-1] == "2")
            else:
                env, host, device = rc.WRITE_SWITCH[route]
                monkeypatch.setenv(env, device if writer == "device" else host)
                assert (a._encode_device() is not None) == (writer == "device")
            a.write(off, data)
            info = a.last_write_info
        stored = cc.stored_objects(a)
        # keys
        assert {c for c, o in stored.items() if o is None} == \
            {c for c, o in model.objs.items() if o is None}, (seed, k, "keys")
        if encode:
            n = {c: _members(a, o, model.objs[c], ax) for c, o in stored.items() if o is not None}
            assert info["gzip_device_frames"] == sum(n[c] for c in mine), (seed, k, info)
            assert [info[c] for c in COUNTERS if c != "gzip_device_frames"] == [0] * 5, \
                (seed, k, info)
            assert info["stored_bytes"] == sum(len(stored[c]) for c in mine), (seed, k, info)
        elif writer in ("host", "device"):
            kind = rc.COUNTER[route] + ("_device_frames" if writer == "device" else "_host_frames")
            assert info[kind] == sum(
                sum(u is not None for u in cc.units(a, model.objs[c])) for c in mine), \
                (seed, k, info)
        got = _reads(case, a, model, rng, dev, monkeypatch, (seed, k))
        frames, nbytes = frames + got[0], nbytes + got[1]
    return frames, nbytes


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_route_fuzz(dev, seed, tmp_path, monkeypatch):
    case = rc.random_route_case(seed)
    frames, nbytes = run_case(case, tmp_path, monkeypatch, dev, seed)
    ax = case.axes
    print(f"route case {seed}: {ax['route']} {ax['format']} writer {ax['writer']}: whole-array "
          f"reads of {frames} frames, {nbytes} bytes decoded on the device with where == 0")
