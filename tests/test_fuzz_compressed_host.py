"""The CPU half of the compressed-write fuzz: the independent decoders of independent_codecs.py
against test-side frames and against the library's host writers, the coverage of the case
generator (compressed_cases.py) over its default seeds, and every case's chunks through the codec
objects' host encode.  The device half is test_gpu_fuzz_compressed.py.  No GPU."""
import functools

import numpy as np
import pytest

import blosc_enc_inputs as bi
import compressed_cases as cc
import independent_codecs as ic
import spec_blosc as sb
import zarrhip as z
import zstd_enc_inputs as zi
from test_zstd_encode_host import MATRIX as ZSTD_MATRIX
from test_zstd_encode_host import frames as zstd_frames  # noqa: F401 (fixture)
from zarrhip import _lib


# ---- the decoders against test-side frames -----------------------------------------------------
@pytest.fixture
def liblz4_streams(monkeypatch):
    """spec_blosc.frame with its LZ4 streams written by liblz4: spec_blosc's own greedy writer may
    start a match inside the last 12 bytes of a stream, which the library's decoder takes and
    liblz4, the decoder on this side, refuses."""
    lz = ic.pa.Codec("lz4_raw")
    monkeypatch.setattr(sb, "lz4_compress", lambda part: lz.compress(bytes(part), asbytes=True))


def _elements(ts, ne, seed):
    """ne elements of ts bytes: low bytes that vary, high bytes that do not (bit planes that
    compress and bit planes that do not)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((ne, ts), np.uint8)
    a[:, 0] = rng.integers(0, 256, ne)
    if ts > 1:
        a[:, 1] = np.arange(ne) // 5 % 7
    return a.tobytes()


@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("ne", [7, 8, 9, 127, 128, 1000])
@pytest.mark.parametrize("ts", [1, 2, 4, 8, 17])
def test_bit_shuffle_decoder(liblz4_streams, ts, ne, version):
    """spec_blosc's bit-shuffled frames (test-side code on both sides): one block, blocks of 8 and
    of 40 elements with a leftover, and a ragged tail behind the last element."""
    for tail in (0, 3):
        data = _elements(ts, ne, 31 * ts + ne) + bytes(range(1, tail + 1))
        assert ic.bit_unshuffle(sb.bit_shuffle(data, ts, version), ts, version) == data
        for bs in (len(data), 8 * ts, 40 * ts):
            f = sb.frame(data, ts, bs, "lz4", bitshuffle=True, version=version)
            assert f[2] & 0x04 and not f[2] & 0x01
            assert ic.blosc_lz4_decode(f) == data, (bs, tail)
    if ne % 8:   # format 2 leaves such a block as it is, format 3 shuffles its prefix
        blk = _elements(ts, ne, 5)
        assert (sb.bit_shuffle(blk, ts, version) == blk) == (version == 2 or ne < 8)


@pytest.mark.parametrize("ts,bs", [(1, 256), (2, 512), (4, 1024), (8, 2048), (16, 4096)])
def test_split_frames_with_a_large_leftover(liblz4_streams, ts, bs):
    """spec_blosc's split frames: the full blocks are typesize streams, the leftover block one
    stream although it holds 128 elements or more."""
    data = _elements(ts, 2 * (bs // ts) + 131, 9) + b"\x07"
    f = sb.frame(data, ts, bs, "lz4", True, True)
    assert not f[2] & 0x10 and len(data) % bs == 131 * ts + 1
    assert ic.blosc_lz4_decode(f) == data
    assert ic.blosc_lz4_decode(sb.frame(data, ts, bs, "lz4", True, False)) == data


def test_memcpyed_and_empty_frames():
    c = z.BloscCodec("zstd", 5, "shuffle", 4)      # a cname the library writes MEMCPYED
    f = c.encode(b"abcdefgh" * 9)
    assert f[2] & 0x02 and ic.blosc_lz4_decode(f) == b"abcdefgh" * 9
    assert ic.blosc_lz4_decode(sb.frame(b"", 4, 256, "lz4")) == b""


# ---- the decoders against the library's host writers -------------------------------------------
def test_blosc_matrix_decodes():
    for label, data, ts, sh, bs in bi.matrix():
        f = _lib.blosc_compress(data, ts, sh, bs)
        assert ic.blosc_lz4_decode(f) == data, label


def test_blosc_matrix_with_large_leftovers():
    """The same buffers under block sizes that leave 128 elements or more in the leftover block
    (two full blocks and a fifth of the elements): c-blosc never splits a leftover block, and a
    walk that splits by the element count alone cannot read these frames."""
    seen = split = 0
    for label, data, ts, sh, _ in bi.matrix():
        ne = len(data) // ts
        if ne < 700:
            continue
        bs = ne * 2 // 5 * ts
        f = _lib.blosc_compress(data, ts, sh, bs)
        assert ic.blosc_lz4_decode(f) == data, label
        if f[2] & 0x02:
            continue
        assert int.from_bytes(f[8:12], "little") == bs
        assert (len(data) % bs) // ts >= 128 and bs // ts >= 128, label
        seen += 1
        split += not f[2] & 0x10
    assert seen >= 3 * len(bi.TYPESIZES) and split >= len(bi.TYPESIZES) - 1
    # a configured block size past the 64 KiB clamp: three blocks and a leftover of 3392 bytes
    data = bi.smooth(200000)
    for ts, sh in ((4, 1), (1, 0), (8, 2), (17, 1)):
        assert ic.blosc_lz4_decode(_lib.blosc_compress(data, ts, sh, 1 << 20)) == data


def test_zstd_matrix_decodes(zstd_frames):  # noqa: F811
    """The frames test_zstd_encode_host.py makes of zstd_enc_inputs.matrix(), through this
    module's decoder."""
    for (label, data, cs, _), f in zip(ZSTD_MATRIX, zstd_frames):
        assert ic.zstd_decode(f, len(data)) == data, label
        assert ic.zstd_has_checksum(f) == cs, label


# ---- the generated cases -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk(seed):
    """One case through the model, every unit (chunk or inner chunk) of every object a step sets
    through the codec object's host encode and back through the independent decoders.  Returns
    the counts the coverage test adds up."""
    case = cc.random_case(seed)
    ax = case.axes
    a = case.cls.create(z.MemoryStore().resolve("a"), case.meta())
    codec = cc.bb_codec(a)
    # a chain _encode_device() sends to the device (the codec is the only byte-to-byte stage)
    if ax["codec"] == "blosc":
        assert a._blosc_chain() and codec.lz4()
    else:
        assert a._zstd_chain()
    assert list(a.metadata.shape) == ax["shape"] and a.metadata.data_type.numpy == case.dtype
    ds = case.dtype.itemsize
    model = cc.Model(a)
    st = dict(deleting_steps=0, unaligned_steps=0, raw_units=0, units=0, max_unit=0, absent=0)
    for k, (off, data) in enumerate(case.steps):
        assert data.dtype == case.dtype and (k > 0 or off is None)
        before = dict(model.objs)
        changed = model.write(off, data)
        st["unaligned_steps"] += not cc.aligned(a, off, data)
        st["deleting_steps"] += any(o is None and before[c] is not None
                                    for c, o in changed.items())
        for c, obj in changed.items():
            if obj is None:
                continue
            for u in cc.units(a, obj):
                if u is None:
                    st["absent"] += 1
                    continue
                if ax["codec"] == "blosc":
                    f = codec.encode(u, ds)
                    assert ic.blosc_lz4_decode(f) == u, (seed, k, c)
                    assert f[3] == ax["frame_typesize"]
                    raw = bool(f[2] & 0x02)
                else:
                    f = codec.encode(u)
                    assert ic.zstd_decode(f, len(u)) == u, (seed, k, c)
                    assert ic.zstd_has_checksum(f) == ax["checksum"]
                    raw = all(t == 0 for t, _, _ in zi.blocks(f))
                st["units"] += 1
                st["raw_units"] += raw
                st["max_unit"] = max(st["max_unit"], len(u))
    return st


@pytest.mark.parametrize("seed", cc.SEEDS)
def test_host_form(seed):
    """Every chunk or inner chunk of the case, as the oracle hands it to the compressor, through
    the codec object's host encode: the frame decodes with libzstd / liblz4 to those bytes."""
    st = walk(seed)
    assert st["units"] > 0


def test_generator_coverage():
    """Conditions on the inputs over the default seeds, whatever ZH_FUZZ_CCASES says (a generator
    that stops drawing an axis fails here, not silently)."""
    cases = [cc.random_case(s).axes for s in range(cc.DEFAULT_SEEDS)]
    stats = [walk(s) for s in range(cc.DEFAULT_SEEDS)]
    blosc = [ax for ax in cases if ax["codec"] == "blosc"]
    sharded = [ax for ax in cases if ax["format"] == "sharded"]
    count = {
        "format x codec": len({(ax["format"], ax["codec"]) for ax in cases}),
        "shuffles": {s: sum(ax["shuffle"] == s for ax in blosc) for s in cc.SHUFFLES},
        "explicit typesizes": {t: sum(ax["typesize"] == t for ax in blosc)
                               for t in cc.EXPLICIT_TYPESIZES},
        "blocksizes": sorted({ax["blocksize"] for ax in blosc}),
        "index big/little": [sum(ax["index_big"] for ax in sharded),
                             sum(not ax["index_big"] for ax in sharded)],
        "index crc yes/no": [sum(ax["index_crc"] for ax in sharded),
                             sum(not ax["index_crc"] for ax in sharded)],
        "index start/end": [sum(ax["index_location"] == "start" for ax in sharded),
                            sum(ax["index_location"] == "end" for ax in sharded)],
        "odd inner byte size": sum(ax["odd_inner"] for ax in sharded),
        "units over 128 KiB": {k: sum(ax["codec"] == k and st["max_unit"] > 128 << 10
                                      for ax, st in zip(cases, stats)) for k in cc.CODECS},
        "deleting steps": sum(st["deleting_steps"] for st in stats),
        "cases with a raw unit": sum(st["raw_units"] > 0 for st in stats),
        "unaligned steps": sum(st["unaligned_steps"] for st in stats),
        "dtypes": sorted({ax["dtype"] for ax in cases}),
        "ranks": sorted({ax["rank"] for ax in cases}),
        "stores": sorted({ax["store"] for ax in cases}),
        "no fill value": sum(ax["fill"] is None for ax in cases),
        "units": sum(st["units"] for st in stats),
    }
    print("coverage:", count)
    assert count["format x codec"] == len(cc.FORMATS) * len(cc.CODECS)
    assert all(v > 0 for v in count["shuffles"].values())
    assert all(v > 0 for v in count["explicit typesizes"].values())
    assert {0, 256, 4096, cc.ODD_BLOCK, cc.ODD_BLOCK_LARGE} <= set(count["blocksizes"])
    assert all(v > 0 for v in count["index big/little"])
    assert all(v > 0 for v in count["index crc yes/no"])
    assert all(v > 0 for v in count["index start/end"])
    assert count["odd inner byte size"] >= 2
    assert all(v >= 3 for v in count["units over 128 KiB"].values())
    assert count["deleting steps"] >= 5
    assert count["cases with a raw unit"] >= 5
    assert count["unaligned steps"] >= 5
    assert count["dtypes"] == sorted(cc.DTYPES) and count["ranks"] == [1, 2, 3, 4]
    assert count["stores"] == ["files", "memory"] and count["no fill value"] >= 1
