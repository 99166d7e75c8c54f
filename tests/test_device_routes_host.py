"""The CPU half of the fuzz of the opt-in device codec routes (device_route_cases.py): every
generated frame is planned for the device and decodes to its data by an independent decoder (zlib,
libzstd) and by the library's host decoder; the frames reach the block types, literal forms and
match distances they are there for; the three stand-alone sanitizer checkers take them; and every
array case walks through the oracle's model with its frames made on the host.  The device half is
test_gpu_device_routes.py.  No GPU."""
import functools
import struct
import subprocess
import zlib

import pytest

import blosc_frames as bf
import blosc_zstd_inputs as bz
import compressed_cases as cc
import device_route_cases as rc
import spec_blosc as sb
import zarrhip as z
import zstd_dec_inputs as zi
from test_blosc_zstd_host import checker as blosc_zstd_checker  # noqa: F401 (fixture)
from test_gzip_decode_host import checker as gzip_checker  # noqa: F401 (fixture)
from test_zstd_batch_host import checker as zstd_checker  # noqa: F401 (fixture)
from zarrhip import _abi as A
from zarrhip import _lib


def host_decode(codec, f):
    if codec == "gzip":
        return _lib.gzip_decompress(f)
    st, out, msg = zi.host_decode(f) if codec == "zstd" else bf.host_decode(f)
    assert st == A.ZH_OK, msg
    return out


# ---- the frames --------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", rc.CODECS)
def test_every_frame_is_planned_for_the_device(codec):
    """No frame is filtered out: the generator makes only what the plan's rules admit."""
    for batch in [rc.frames(codec)] + rc.batches(codec):
        total, rows = rc.plan(codec, [f for _, _, f in batch])
        pos = 0
        for (label, data, _), (off, nb, where) in zip(batch, rows):
            assert where == 0, label
            assert (off, nb) == (pos, len(data)) and off % 256 == 0, label
            pos = -(-(pos + nb) // 256) * 256
        assert total == pos
    for batch in rc.batches(codec):      # every batch mixes empty, tiny and large frames
        sizes = {len(d) for _, d, _ in batch}
        assert 16 <= len(batch) <= 64 and {0, 1, 64, 200_000} <= sizes


@pytest.mark.parametrize("codec", rc.CODECS)
def test_every_frame_decodes_to_its_data(codec):
    for label, data, f in rc.frames(codec):
        assert rc.independent_decode(codec, f, len(data)) == data, label
        assert host_decode(codec, f) == data, label


def _zstd_coverage(streams):
    seen = {"block": set(), "literals": set(), "huffman streams": set(), "table modes": set()}
    for s in streams:
        for r in _lib.zstd_blocks(s):
            seen["block"].add(r[0])
            if r[0] != 2:
                continue
            seen["literals"].add(r[3])
            if r[3] >= 2:
                seen["huffman streams"].add(r[4])
            if r[6]:
                seen["table modes"] |= set(r[7:10])
    return {k: sorted(v) for k, v in seen.items()}


def test_frame_coverage():
    """Conditions on the generator over the default frames, whatever ZH_FUZZ_RFRAMES says."""
    gz = rc.frames("gzip")
    rows = [r for _, _, f in gz for r in _lib.gzip_blocks(f)]
    cov = {
        "frames": {c: len(rc.frames(c)) for c in rc.CODECS},
        "raw bytes": {c: sum(len(d) for _, d, _ in rc.frames(c)) for c in rc.CODECS},
        "gzip block types": sorted({r[0] for r in rows}),
        "gzip largest distance": max(r[8] for r in rows),
        "gzip members of several blocks": sum(len(_lib.gzip_blocks(f)) > 1 for _, _, f in gz),
        "zstd": _zstd_coverage(f for _, _, f in rc.frames("zstd")),
        "blosc-zstd": _zstd_coverage(s for _, _, f in rc.frames("blosc-zstd")
                                     for s in bz.zstd_streams(f)),
        "zstd frames of several blocks": sum(len(_lib.zstd_blocks(f)) > 1
                                             for _, _, f in rc.frames("zstd")),
        "blosc blocks over the LDS window": sum(
            any(r[0] == 0 and r[2] > bz.LDS_BLOCK for r in _lib.blosc_streams(f, bz.FLAG))
            for _, _, f in rc.frames("blosc-zstd")),
        "blosc split frames": sum(not f[2] & 0x10 and len(d) > 0
                                  for _, d, f in rc.frames("blosc-zstd")),
        "blosc shuffles": sorted({f[2] & 0x05 for _, _, f in rc.frames("blosc-zstd")}),
        "blosc typesizes": sorted({f[3] for _, _, f in rc.frames("blosc-zstd")}),
        "encoders": {c: sorted({lb.split()[3] for lb, _, _ in rc.frames(c)}) for c in rc.CODECS},
    }
    print("frame coverage:", cov)
    assert all(1 << 20 <= v <= 2.5 * (1 << 20) for v in cov["raw bytes"].values())
    assert all({len(d) for _, d, _ in rc.frames(c)} == set(rc.SIZES) for c in rc.CODECS)
    assert cov["gzip block types"] == [0, 1, 2]
    assert 32_000 <= cov["gzip largest distance"] <= 32_768
    assert cov["gzip members of several blocks"] >= 10
    # raw, Huffman and treeless literals, one and four Huffman streams, predefined, FSE and
    # repeated tables, raw, RLE and compressed blocks.  RLE literals and RLE-mode tables are
    # not reached by libzstd over these bytes: zstd_dec_inputs' hand-built frames hold them.
    assert set(cov["zstd"]["block"]) == {0, 1, 2}
    assert set(cov["zstd"]["literals"]) >= {0, 2, 3}
    assert cov["zstd"]["huffman streams"] == [1, 4]
    assert set(cov["zstd"]["table modes"]) >= {0, 2, 3}
    assert cov["zstd frames of several blocks"] >= 10
    # the streams of the blosc frames: RLE-mode tables are reached here
    assert set(cov["blosc-zstd"]["literals"]) >= {0, 2}
    assert cov["blosc-zstd"]["huffman streams"] == [1, 4]
    assert set(cov["blosc-zstd"]["table modes"]) >= {0, 1, 2}
    assert cov["blosc blocks over the LDS window"] >= 5 and cov["blosc split frames"] >= 5
    assert cov["blosc shuffles"] == [0, 1, 4]
    assert cov["blosc typesizes"] == sorted(rc.BLOSC_TYPESIZES)
    assert cov["encoders"] == {"gzip": ["own", "zlib"], "zstd": ["libzstd", "own"],
                               "blosc-zstd": ["libzstd1", "libzstd5", "own"]}


def test_blosc_header_bound_follows_the_compressor():
    """Found by this fuzz at ZH_FUZZ_RFRAMES=480: zh_blosc_decompress and the batch plan refused a
    valid frame of a constant buffer ("corrupt blosc header") because nbytes exceeded 2048 times
    the frame's length, DEFLATE's bound; a zstd RLE block is 128 KiB from 4 bytes.  The bound is
    32768 for zstd streams now, and still 2048 for the others."""
    for label, data, f in rc.constant_blosc_frames():
        assert len(data) > 2048 * len(f) + 65536, label
        assert rc.blosc_zstd_decode(f) == data, label
        assert bf.host_decode(f)[:2] == (bf.ZH_OK, data), label
        assert z.BloscCodec().decode(f) == data, label
        assert rc.plan("blosc-zstd", [f])[1] == [(0, len(data), 0)], label
        bad = bytearray(f)
        bad[4:8] = struct.pack("<I", 32768 * len(f) + 65536 + 1)
        assert bf.host_decode(bytes(bad))[::2] == (bf.ZH_EDATA, "corrupt blosc header"), label
    lz4 = bytearray(sb.frame(bytes(8192), 1, 4096, "lz4"))
    assert bf.host_decode(bytes(lz4))[:2] == (bf.ZH_OK, bytes(8192))
    lz4[4:8] = struct.pack("<I", 2048 * len(lz4) + 65536 + 1)
    assert bf.host_decode(bytes(lz4))[::2] == (bf.ZH_EDATA, "corrupt blosc header")


# ---- the frames through the stand-alone sanitizer checkers -------------------------------------
def _run(checker, frames, tmp_path):
    p = tmp_path / "frames.bin"
    with open(p, "wb") as fh:
        for f in frames:
            fh.write(struct.pack("<I", len(f)) + f)
    r = subprocess.run([checker, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames)
    return [ln.split() for ln in lines]


def test_gzip_frames_under_sanitizers(gzip_checker, tmp_path):  # noqa: F811
    fs = rc.frames("gzip")
    for (label, data, _), ln in zip(fs, _run(gzip_checker, [f for _, _, f in fs], tmp_path)):
        assert ln == ["0", "0", str(len(data)), "ok"], label


def test_zstd_frames_under_sanitizers(zstd_checker, tmp_path):  # noqa: F811
    L = _lib.lib()
    fs = rc.frames("zstd")
    for (label, data, _), ln in zip(fs, _run(zstd_checker, [f for _, _, f in fs], tmp_path)):
        assert (int(ln[0]), int(ln[1])) == (0, A.ZH_OK), label
        assert int(ln[2], 16) == L.zh_xxh64(data, len(data), 0), label


def test_blosc_zstd_frames_under_sanitizers(blosc_zstd_checker, tmp_path):  # noqa: F811
    L = _lib.lib()
    fs = rc.frames("blosc-zstd") + rc.constant_blosc_frames()
    streams = 0
    for (label, data, _), ln in zip(fs, _run(blosc_zstd_checker, [f for _, _, f in fs],
                                             tmp_path)):
        assert (int(ln[0]), int(ln[1])) == (0, bf.ZH_OK), label
        assert int(ln[2], 16) == L.zh_xxh64(data, len(data), 0), label
        streams += int(ln[3])
    assert streams >= len(fs)


# ---- the array cases -----------------------------------------------------------------------------
def unit_frames(a, ax, obj):
    """[(unit bytes, its frame as the case's writer makes it on the host)] of one object of the
    oracle's; a foreign writer's shard is tiled by device_route_cases.foreign_object and read
    back through its index here."""
    us = [u for u in cc.units(a, obj) if u is not None]
    route = ax["route"]
    if ax["writer"] == "foreign":
        stored = rc.foreign_object(a, ax, obj)
        if not a.chain.chain["sharded"]:
            return [(obj, stored)]
        ents, isz = cc.shard_entries(a, stored)
        assert [e is None for e in ents] == [u is None for u in cc.units(a, obj)]
        assert sum(e[1] for e in ents if e is not None) + isz == len(stored)
        return list(zip(us, [stored[e[0]:e[0] + e[1]] for e in ents if e is not None]))
    if route.startswith("gzip-enc"):
        return [(u, _lib.gzip_compress(u, dynamic=route == "gzip-enc-2")) for u in us]
    return [(u, cc.bb_codec(a).encode(u)) for u in us]


@functools.lru_cache(maxsize=None)
def walk(seed):
    """One case through the model, every unit of every object a step sets through its writer's
    host form and back through the independent decoder.  Returns the counts the coverage test
    adds up."""
    case = rc.random_route_case(seed)
    ax = case.axes
    route = ax["route"]
    a = case.cls.create(z.MemoryStore().resolve("a"), case.meta())
    codec = rc.COUNTER[route]
    assert {"zstd": a._zstd_chain, "gzip": a._gzip_chain, "blosc": a._blosc_chain}[codec]()
    assert list(a.metadata.shape) == ax["shape"] and a.metadata.data_type.numpy == case.dtype
    plan_codec = {"zstd": "zstd", "gzip": "gzip", "blosc": "blosc-zstd"}[codec]
    model = cc.Model(a)
    st = dict(deleting_steps=0, unaligned_steps=0, units=0, max_unit=0, dynamic=0, two_blocks=0)
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
            for u, f in unit_frames(a, ax, obj):
                assert rc.independent_decode(plan_codec, f, len(u)) == u, (seed, k, c)
                # what the route's reads meet is what the device takes
                assert rc.plan(plan_codec, [f])[1][0] == (0, len(u), 0), (seed, k, c)
                if route.startswith("gzip-enc"):
                    rows = _lib.gzip_blocks(f)
                    st["dynamic"] += any(r[0] == 2 for r in rows)
                    st["two_blocks"] += len(u) > 16 << 10 and len(rows) > 1
                st["units"] += 1
                st["max_unit"] = max(st["max_unit"], len(u))
    # what a read of the whole array touches is every stored unit, except under a NaN fill value:
    # there an all-NaN inner chunk is not elided, and a boundary shard stores some that lie
    # outside the array
    stored = sum(u is not None for o in model.objs.values() if o is not None
                 for u in cc.units(a, o))
    touched = rc.present_units(a, model, ax["unit"])
    nan_fill = isinstance(ax["fill"], float) and ax["fill"] != ax["fill"]
    assert touched == stored or (nan_fill and ax["format"] == "sharded" and touched < stored)
    return st


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_route_case_host_form(seed):
    assert walk(seed)["units"] > 0


def test_route_generator_coverage():
    """Conditions on the array cases over the default seeds, whatever ZH_FUZZ_RCASES says."""
    cases = [rc.random_route_case(s).axes for s in range(rc.DEFAULT_SEEDS)]
    stats = [walk(s) for s in range(rc.DEFAULT_SEEDS)]
    sharded = [ax for ax in cases if ax["format"] == "sharded"]
    both = list(zip(cases, stats))
    count = {
        "route x format": sorted({(ax["route"], ax["format"]) for ax in cases}),
        "writers": {r: sorted({ax["writer"] for ax in cases if ax["route"] == r})
                    for r in rc.WRITERS},
        "dtypes": sorted({ax["dtype"] for ax in cases}),
        "ranks": sorted({ax["rank"] for ax in cases}),
        "stores": sorted({ax["store"] for ax in cases}),
        "index big/little": [sum(ax["index_big"] for ax in sharded),
                             sum(not ax["index_big"] for ax in sharded)],
        "index crc yes/no": [sum(ax["index_crc"] for ax in sharded),
                             sum(not ax["index_crc"] for ax in sharded)],
        "index start/end": [sum(ax["index_location"] == "start" for ax in sharded),
                            sum(ax["index_location"] == "end" for ax in sharded)],
        "deleting steps": sum(st["deleting_steps"] for st in stats),
        "unaligned steps": sum(st["unaligned_steps"] for st in stats),
        "cases with a unit over 128 KiB": {r: sum(ax["route"] == r and st["max_unit"] > 128 << 10
                                                  for ax, st in both) for r in rc.ROUTES},
        "gzip-enc-2 cases with a dynamic block": sum(
            ax["route"] == "gzip-enc-2" and st["dynamic"] > 0 for ax, st in both),
        "gzip-enc-2 cases with a member of several blocks": sum(
            ax["route"] == "gzip-enc-2" and st["two_blocks"] > 0 for ax, st in both),
        "units": sum(st["units"] for st in stats),
        "largest case": max(int(cc.np.prod(ax["shape"])) * cc.np.dtype(ax["dtype"]).itemsize
                            for ax in cases),
    }
    print("coverage:", count)
    assert count["route x format"] == sorted((r, f) for r in rc.ROUTES for f in rc.FORMATS[r])
    assert count["writers"] == {r: sorted(w) for r, w in rc.WRITERS.items()}
    assert count["dtypes"] == sorted(cc.DTYPES) and count["ranks"] == [1, 2, 3, 4]
    assert count["stores"] == ["files", "memory"]
    assert all(v > 0 for v in count["index big/little"] + count["index crc yes/no"] +
               count["index start/end"])
    assert count["deleting steps"] >= 5 and count["unaligned steps"] >= 5
    assert all(v >= 2 for v in count["cases with a unit over 128 KiB"].values())
    assert count["gzip-enc-2 cases with a dynamic block"] >= 2
    assert count["gzip-enc-2 cases with a member of several blocks"] >= 1
    assert count["largest case"] <= rc.RAW_LIMIT


def test_zlib_stays_inside_its_window():
    """The 32 768 edge is gzip_dec_inputs' hand-built member's: zlib's matcher stops 262 bytes
    short of the window, which is where the generator's far copies aim."""
    rng = cc.np.random.default_rng(1)
    data = rc.lane_edge_data(rng, 70_000)
    m = rc.zlib_member(data, 9, 9, zlib.Z_DEFAULT_STRATEGY)
    assert max(r[8] for r in _lib.gzip_blocks(m)) <= rc.ZLIB_MAX_DIST
