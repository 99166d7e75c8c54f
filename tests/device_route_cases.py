"""Seeded inputs for the opt-in device codec routes (ZH_ZSTD_DEVICE=2, ZH_GZIP_DEVICE=2,
ZH_BLOSC_ZSTD_DEVICE=1, ZH_GZIP_ENCODE_DEVICE=1 / 2), shared by test_device_routes_host.py (CPU)
and test_gpu_device_routes.py.  Two generators:

frames(codec): gzip members, zstd frames and blosc frames with zstd streams made by foreign
encoders (zlib, libzstd through pyarrow) and by the library's host writers over lane_edge_data:
bytes aimed at the wave-only code of the decoders (matches whose offset is shorter than their
length, literal runs around 64, copies from a window's far edge) in frames around the block and
window sizes of the three formats.  Every frame is one its plan sends to the device.

random_route_case(seed): arrays over compressed_cases' axes with the route rotating with the seed,
and, for the three decode routes, the writer of the stored frames (the library's host writer, its
device writer, or a foreign encoder over the oracle's objects: foreign_object).

No axis value of the issue's lists had to be dropped: every generated frame is planned where == 0.
Test infrastructure only; nothing here needs a device."""
import functools
import os
import struct
import zlib

import numpy as np

import blosc_zstd_inputs as bz
import compressed_cases as cc
import independent_codecs as ic
import oracle as O
import zarrhip as z
from compressed_cases import _counts, _dims, _mixture, bits
from zarrhip import _abi as A
from zarrhip import _lib, v2

# ---- bytes aimed at the lanes ------------------------------------------------------------------
PERIODS = (1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
NOISE_RUNS = (1, 2, 63, 64, 65, 127, 128, 129)
ZLIB_MAX_DIST = 32768 - 262       # deflate.h MAX_DIST: what zlib's matcher reaches back
SKEW = np.r_[np.full(4, 0.15), np.full(12, 0.025), np.full(240, 0.1 / 240)]


def skewed(rng, n, first):
    """n bytes from a distribution that Huffman coding shortens: 16 frequent values from `first`."""
    return ((rng.choice(256, n, p=SKEW) + first) % 256).astype(np.uint8).tobytes()


def lane_edge_data(rng, n):
    """n bytes of seeded segments: periodic runs longer than their period (a match whose offset is
    below its length), noise runs of the lengths around a wave's 64 literals, copies of earlier
    slices (32 768 back, and at the far edge of zlib's window, once the data is that long), short
    constant runs and runs from a skewed distribution (one per call: a later zstd block can
    reuse the Huffman table of the block before it)."""
    out = bytearray()
    first = int(rng.integers(256))
    while len(out) < n:
        kind = int(rng.integers(5))
        if kind == 0:
            p = int(rng.choice(PERIODS))
            length = p + int(rng.integers(1, 3 * p + 70))
            unit = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
            out += (unit * (length // p + 1))[:length]
        elif kind == 1:
            edge = rng.random() < 0.7
            length = int(rng.choice(NOISE_RUNS)) if edge else int(rng.integers(3, 400))
            out += rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        elif kind == 2 and out:
            r = rng.random()
            if len(out) >= 32768 and r < 0.15:
                dist = 32768
            elif len(out) >= 32768 and r < 0.3:
                dist = int(rng.integers(32000, ZLIB_MAX_DIST + 1))
            else:
                dist = int(rng.integers(1, len(out) + 1))
            length = int(rng.integers(3, 300))
            seg = bytes(out[len(out) - dist:len(out) - dist + min(length, dist)])
            out += (seg * (length // len(seg) + 1))[:length]
        elif kind == 3:
            out += bytes([int(rng.integers(256))]) * int(rng.integers(3, 40))
        else:
            out += skewed(rng, int(rng.integers(20, 2000)), first)
    return bytes(out[:n])


# ---- frames from foreign encoders ---------------------------------------------------------------
CODECS = ("gzip", "zstd", "blosc-zstd")
# around zstd's 128 KiB block, the gzip writer's 16 KiB blocks, the blosc kernel's 64 KiB window
SIZES = (0, 1, 63, 64, 65, 300, 4096, 20_000, 40_000, 70_000, 140_000, 200_000)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY,
              zlib.Z_FIXED)
ZSTD_LEVELS = (-5, 1, 3, 9, 19)
BLOSC_TYPESIZES = (1, 2, 3, 4, 8, 17)
BLOSC_BLOCKS = (256, 1001, 4096, bz.LDS_BLOCK + 512, None)      # None: the whole buffer
BATCH = 20
# ZH_FUZZ_RFRAMES widens the search (default 60 frames per codec: five of every size)
DEFAULT_FRAMES = 60
N_FRAMES = int(os.environ.get("ZH_FUZZ_RFRAMES", str(DEFAULT_FRAMES)))


def zlib_member(data, level, mem_level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level, strategy)
    return c.compress(data) + c.flush()


def libzstd(data, level):
    return ic.pa.Codec("zstd", compression_level=level).compress(bytes(data), asbytes=True)


def _frame_data(rng, n):
    """Mostly lane_edge_data; one frame in eight constant (zstd's RLE block) and one in eight
    skewed alone (Huffman literals without matches)."""
    r = rng.random()
    if r < 0.125:
        return "constant", bytes([int(rng.integers(256))]) * n
    if r < 0.25:
        return "skewed", skewed(rng, n, int(rng.integers(256)))
    return "lanes", lane_edge_data(rng, n)


def _blosc_frame(rng, data):
    ts = int(rng.choice(BLOSC_TYPESIZES))
    shuffle = ("none", "byte", "bit")[int(rng.integers(3))]
    bs = BLOSC_BLOCKS[int(rng.integers(len(BLOSC_BLOCKS)))] or max(1, len(data))
    # a split block is typesize streams of blocksize / typesize bytes
    split = bool(bs % ts == 0 and rng.random() < 0.5)
    version = int(rng.choice([2, 3]))
    src = int(rng.integers(3))
    zfn = (bz.libzstd(1), bz.libzstd(5), bz.own)[src]
    label = f"{('libzstd1', 'libzstd5', 'own')[src]} ts{ts} {shuffle} bs{bs} split{int(split)}"
    return label, bz.frame(data, ts, bs, zfn, shuffle=shuffle, split=split, version=version)


@functools.lru_cache(maxsize=None)
def frames(codec, n=DEFAULT_FRAMES):
    """[(label, data, frame)]: frame k has size SIZES[k % 12], its data and encoder drawn from
    np.random.default_rng([codec number, k])."""
    out = []
    for k in range(n):
        rng = np.random.default_rng([CODECS.index(codec), k])
        kind, data = _frame_data(rng, SIZES[k % len(SIZES)])
        if codec == "gzip":
            if rng.random() < 0.6:
                level, mem = int(rng.choice([1, 4, 6, 9])), int(rng.choice([1, 8, 9]))
                st = int(rng.integers(len(STRATEGIES)))
                label = f"zlib L{level} mem{mem} strategy{st}"
                f = zlib_member(data, level, mem, STRATEGIES[st])
            else:
                bs, dyn = int(rng.choice([1 << 10, 16 << 10, 32 << 10])), bool(rng.integers(2))
                label = f"own bs{bs} dynamic{int(dyn)}"
                f = _lib.gzip_compress(data, bs, dyn)
        elif codec == "zstd":
            if rng.random() < 0.6:
                level = int(rng.choice(ZSTD_LEVELS))
                label = f"libzstd L{level}"
                f = libzstd(data, level)
            else:
                cs, bs = bool(rng.integers(2)), int(rng.choice([0, 1 << 10, 64 << 10]))
                label = f"own checksum{int(cs)} bs{bs}"
                f = _lib.zstd_compress(data, cs, bs)
        else:
            label, f = _blosc_frame(rng, data)
        out.append((f"{k}: {kind} {len(data)} {label}", data, f))
    return out


def batches(codec, n=DEFAULT_FRAMES):
    """The frames in batches of BATCH consecutive ones (every size at least once), each in an
    order shuffled by its number: [[(label, data, frame)]]."""
    fs = frames(codec, n)
    out = []
    for b in range(0, len(fs), BATCH):
        part = fs[b:b + BATCH]
        order = np.random.default_rng([7, CODECS.index(codec), b]).permutation(len(part))
        out.append([part[int(i)] for i in order])
    return out


def constant_blosc_frames():
    """[(label, data, frame)]: a constant buffer of 200 000 bytes as one unsplit block and one of
    600 000 bytes as typesize 4 split into four streams, by libzstd: RLE blocks, a frame several
    thousand times smaller than its content (DEFLATE's 1032 is not the bound of a blosc header
    whose streams are zstd frames)."""
    data, more = bytes([7]) * 200_000, bytes([9]) * 600_000
    return [("one block", data, bz.frame(data, 1, len(data), bz.libzstd(1))),
            ("split in four", more, bz.frame(more, 4, len(more), bz.libzstd(5), shuffle="byte",
                                             split=True))]


def plan(codec, fs):
    """(total, [(dst_off, nbytes, where)]) of the codec's batch plan."""
    if codec == "gzip":
        return _lib.gzip_batch_plan(fs)
    if codec == "zstd":
        return _lib.zstd_batch_plan(fs)
    return _lib.blosc_batch_plan(fs, bz.FLAG)


def blosc_zstd_decode(frame):
    """A blosc1 frame with zstd streams -> its bytes: the layout walked here as
    independent_codecs.blosc_lz4_decode walks an LZ4 frame, the streams decoded by libzstd."""
    frame = bytes(frame)
    ver, _, flags, ts = frame[:4]
    nbytes, blocksize, cbytes = struct.unpack("<III", frame[4:16])
    assert cbytes == len(frame) and flags >> 5 == 4 and not flags & 0x02
    if nbytes == 0:
        return b""
    nblocks = -(-nbytes // blocksize)
    bstarts = struct.unpack(f"<{nblocks}I", frame[16:16 + 4 * nblocks])
    out = bytearray()
    for b in range(nblocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        nsplits = ts if not flags & 0x10 and bsize == blocksize else 1
        assert bsize % nsplits == 0
        want = bsize // nsplits
        pos, blk = bstarts[b], bytearray()
        for _ in range(nsplits):
            (cs,) = struct.unpack("<i", frame[pos:pos + 4])
            pos += 4
            assert 0 < cs <= want and pos + cs <= len(frame)
            blk += frame[pos:pos + cs] if cs == want else ic.zstd_decode(frame[pos:pos + cs], want)
            pos += cs
        if flags & 0x01:
            blk = ic.byte_unshuffle(blk, ts)
        elif flags & 0x04:
            blk = ic.bit_unshuffle(blk, ts, ver)
        out += blk
    assert len(out) == nbytes
    return bytes(out)


def independent_decode(codec, frame, nbytes):
    if codec == "gzip":
        return zlib.decompress(frame, 31)
    if codec == "zstd":
        return ic.zstd_decode(frame, nbytes)
    return blosc_zstd_decode(frame)


# ---- arrays over the five routes -------------------------------------------------------------
ROUTES = ("zstd-dec", "gzip-dec", "blosc-zstd-dec", "gzip-enc-1", "gzip-enc-2")
# the codec whose counters a route's reads and writes move, and the read switch
COUNTER = {"zstd-dec": "zstd", "gzip-dec": "gzip", "blosc-zstd-dec": "blosc",
           "gzip-enc-1": "gzip", "gzip-enc-2": "gzip"}
READ_SWITCH = {"zstd-dec": ("ZH_ZSTD_DEVICE", "2"), "gzip-dec": ("ZH_GZIP_DEVICE", "2"),
               "blosc-zstd-dec": ("ZH_BLOSC_ZSTD_DEVICE", "1"),
               "gzip-enc-1": ("ZH_GZIP_DEVICE", "2"), "gzip-enc-2": ("ZH_GZIP_DEVICE", "2")}
# Array._gzip_chain takes the v3 GzipCodec alone
FORMATS = {r: ("v3", "sharded") if "gzip" in r else ("v3", "sharded", "v2") for r in ROUTES}
# the library stores cname zstd as MEMCPYED frames: only a foreign writer makes zstd streams
WRITERS = {"zstd-dec": ("host", "device", "foreign"), "gzip-dec": ("host", "device", "foreign"),
           "blosc-zstd-dec": ("foreign",)}
# the switch of the library's device writer, and its values for "host" and "device"
WRITE_SWITCH = {"zstd-dec": ("ZH_ZSTD_ENCODE_DEVICE", "0", "1"),
                "gzip-dec": ("ZH_GZIP_ENCODE_DEVICE", "0", "1")}
RAW_LIMIT = cc.RAW_LIMIT

# ZH_FUZZ_RCASES widens the search (default 30 cases: six per route)
DEFAULT_SEEDS = 30
SEEDS = list(range(int(os.environ.get("ZH_FUZZ_RCASES", str(DEFAULT_SEEDS)))))


def random_route_case(seed):
    """A compressed_cases.Case whose axes also name the route, the writer (decode routes) and the
    foreign encoder's parameters.  The route is seed % 5; with k = seed // 5 the format is
    FORMATS[route][k % len], the writer rotates so that six consecutive k hold every writer with
    every format of a route twice over, and k % 6 in (2, 3) is the large band."""
    rng = np.random.default_rng([20251021, seed])
    route = ROUTES[seed % 5]
    k = seed // 5
    fmts = FORMATS[route]
    fmt = fmts[k % len(fmts)]
    writer = None
    if route in WRITERS:
        ws = WRITERS[route]
        writer = ws[(k + (k // 3 if len(fmts) == 3 else 0)) % len(ws)]
    sharded = fmt == "sharded"
    band = "large" if k % 6 in (2, 3) else ("tiny", "middle")[int(rng.random() < 0.6)]
    odd_inner = sharded and band != "large" and rng.random() < 0.45
    name = str(rng.choice(cc.DTYPES[:2] if odd_inner else cc.DTYPES))
    dt = np.dtype(name if name == "bool" else "<" + np.dtype(name).str[1:])
    ds = dt.itemsize
    n = int(rng.integers(1, 5))
    big = bool(ds > 1 and rng.random() < 0.5)
    order = None
    if fmt != "v2" and rng.random() < 0.5:
        order = [int(x) for x in rng.permutation(n)]

    # ---- shapes, as compressed_cases.random_case draws them
    if band == "tiny":
        unit = _dims(rng, n, int(rng.integers(1, 64 // ds + 1)))
    elif band == "middle":
        unit = _dims(rng, n, int(rng.integers(4096 // ds, 40960 // ds + 1)))
    else:
        unit = _dims(rng, n, int(rng.integers((140 << 10) // ds, (200 << 10) // ds + 1)))
        while int(np.prod(unit)) * ds < 129 << 10:
            unit[int(np.argmax(unit))] += 1
    if odd_inner:
        unit = [x if x % 2 else x + 1 for x in unit]
    unit_bytes = int(np.prod(unit)) * ds
    budget = max(1, RAW_LIMIT // unit_bytes)
    if sharded:
        mult = _counts(rng, n, min(12, max(1, budget // 2)))
        if int(np.prod(mult)) == 1 and budget >= 2:
            mult[int(rng.integers(n))] = 2
        chunk = [u * m for u, m in zip(unit, mult)]
        counts = _counts(rng, n, max(1, min(8, budget // int(np.prod(mult)))))
    else:
        chunk = list(unit)
        counts = _counts(rng, n, min(24, budget))
    shape = [c * q if rng.random() < 0.25 else int(rng.integers((c - 1) * q + 1, c * q + 1))
             for c, q in zip(counts, chunk)]

    if name == "bool":
        fill = bool(rng.integers(0, 2))
    elif dt.kind == "f":
        fill = cc.FLOAT_FILLS[int(rng.integers(4))]
    else:
        fill = int(rng.choice([0, 0, 1, 3]))
    if fmt == "v2" and rng.random() < 0.25:
        fill = None
    np_fill = np.array(0 if fill is None else fill, dt)

    # ---- the codec of the metadata, and what a foreign writer encodes with
    ax = dict(seed=seed, route=route, format=fmt, writer=writer, band=band, dtype=name, rank=n,
              big=big, order=order, fill=fill, unit=unit, chunk=chunk, shape=shape,
              odd_inner=odd_inner)
    level = int(rng.integers(1, 10))
    checksum = bool(rng.random() < 0.5)
    shuffle = cc.SHUFFLES[int(rng.integers(3))]
    foreign = dict(
        level=int(rng.choice(ZSTD_LEVELS if route == "zstd-dec" else [1, 4, 6, 9])),
        mem_level=int(rng.choice([1, 8, 9])), strategy=int(rng.integers(len(STRATEGIES))),
        typesize=int(rng.choice(BLOSC_TYPESIZES)),
        shuffle=("none", "byte", "bit")[int(rng.integers(3))],
        blocksize=BLOSC_BLOCKS[int(rng.integers(len(BLOSC_BLOCKS)))],
        split=bool(rng.integers(2)), source=int(rng.integers(3)), version=int(rng.choice([2, 3])))
    ax.update(level=level, checksum=checksum, foreign=foreign)
    if sharded:
        loc = ("start", "end")[int(rng.random() < 0.5)]
        index_big = bool(rng.random() < 0.5)
        index_crc = bool(rng.random() < 0.5)
        ax.update(index_location=loc, index_big=index_big, index_crc=index_crc)
    store = ("memory", "files")[int(rng.random() < 0.4)]
    ax.update(store=store)
    endian = "big" if big else "little"

    def compressor():
        if route == "zstd-dec":
            return z.ZstdCodec(level, checksum)
        if route == "blosc-zstd-dec":
            return z.BloscCodec("zstd", level, shuffle, None, 0)
        return z.GzipCodec(level)

    def meta():
        if fmt == "v2":
            b = (v2.ArrayMetadataBuilder().withShape(shape).withChunks(chunk)
                 .withDataType(getattr(v2.DataType, name.upper() + ("_BE" if big else "")))
                 .withFillValue(fill))
            if route == "zstd-dec":
                return b.withZstdCompressor(level, checksum).build()
            return b.withBloscCompressor("zstd", shuffle, level, 0).build()
        b = (z.ArrayMetadataBuilder().withShape(shape).withDataType(name).withChunkShape(chunk)
             .withFillValue(fill))
        cs = [z.TransposeCodec(order)] if order is not None else []
        cs += [z.BytesCodec(None if ds == 1 else endian), compressor()]
        if sharded:
            index = [z.BytesCodec("big" if index_big else "little")] + \
                ([z.Crc32cCodec()] if index_crc else [])
            cs = [z.ShardingIndexedCodec(unit, cs, index, loc)]
        b.codecs = cs
        return b.build()

    # ---- the write steps, as compressed_cases.random_case draws them
    grids = [unit, chunk] if sharded else [chunk]
    first = _mixture(rng, shape, dt, np_fill, grids)
    if bits(first).tobytes() == bits(np.full(shape, np_fill, dt)).tobytes():
        first.flat[0] = not fill if name == "bool" else 9     # step 0 stores something
    steps = [(None, first)]
    kinds = []
    for _ in range(int(rng.integers(2, 4))):
        kind = ("unaligned", "aligned", "fill")[int(rng.integers(3))]
        kinds.append(kind)
        if kind == "unaligned":
            off = [int(rng.integers(0, s)) for s in shape]
            shp = [int(rng.integers(1, s - o + 1)) for s, o in zip(shape, off)]
        else:   # whole chunks; a fill step may start below a chunk boundary on one axis
            c0 = [int(rng.integers(0, c)) for c in counts]
            c1 = [int(rng.integers(a + 1, c + 1)) for a, c in zip(c0, counts)]
            off = [a * q for a, q in zip(c0, chunk)]
            end = [min(b * q, s) for b, q, s in zip(c1, chunk, shape)]
            if kind == "fill" and rng.random() < 0.5:
                d = int(rng.integers(n))
                off[d] = max(0, off[d] - int(rng.integers(1, chunk[d] + 1)))
            shp = [e - o for e, o in zip(end, off)]
        if kind == "fill":
            data = np.full(shp, np_fill, dt)
        else:
            whole = _mixture(rng, shape, dt, np_fill, grids)
            data = np.ascontiguousarray(whole[tuple(slice(o, o + q) for o, q in zip(off, shp))])
        steps.append((off, data))
    ax.update(steps=kinds)
    return cc.Case(meta, v2.Array if fmt == "v2" else z.Array, dt, store, steps, ax)


# ---- the foreign writer ------------------------------------------------------------------------
def foreign_frame(ax, unit):
    """One unit (a chunk, or an inner chunk of a shard) by the case's foreign encoder."""
    f, route = ax["foreign"], ax["route"]
    if route == "zstd-dec":
        return libzstd(unit, f["level"])
    if route == "gzip-dec":
        return zlib_member(unit, f["level"], f["mem_level"], STRATEGIES[f["strategy"]])
    ts, bs = f["typesize"], f["blocksize"] or max(1, len(unit))
    zfn = (bz.libzstd(1), bz.libzstd(5), bz.own)[f["source"]]
    return bz.frame(unit, ts, bs, zfn, shuffle=f["shuffle"], split=f["split"] and bs % ts == 0,
                    version=f["version"])


def foreign_object(a, ax, obj):
    """What a foreign writer stores for the oracle's uncompressed object `obj`: the chunk's frame,
    or the shard tiled again from the frames of its inner chunks, the index written with the
    chain's own place, endianness and crc32c."""
    if not a.chain.chain["sharded"]:
        return foreign_frame(ax, obj)
    ch = a.chain.chain
    ents, isz = cc.shard_entries(a, obj)
    start = ch["index_location"] == A.ZH_INDEX_START
    fmt = ">QQ" if ch["index_endian"] == A.ZH_ENDIAN_BIG else "<QQ"
    pos, payload, index = (isz if start else 0), [], b""
    for e in ents:
        if e is None:
            index += struct.pack(fmt, 2 ** 64 - 1, 2 ** 64 - 1)
            continue
        f = foreign_frame(ax, obj[e[0]:e[0] + e[1]])
        index += struct.pack(fmt, pos, len(f))
        payload.append(f)
        pos += len(f)
    if ch["index_crc32c"]:
        index += struct.pack("<I", O.crc32c(index))
    body = b"".join(payload)
    return index + body if start else body + index


def present_units(a, model, inner, offset=None, shape=None):
    """The number of stored units (chunks, or inner chunks of shards of inner shape `inner`) of
    the model that a region touches (default: the whole array)."""
    n = model.n
    offset = [0] * n if offset is None else offset
    shape = model.shape if shape is None else shape
    cs = model.cs
    sharded = a.chain.chain["sharded"]
    count = 0
    for c, obj in model.objs.items():
        if obj is None:
            continue
        lo = [max(o, ci * q) for o, ci, q in zip(offset, c, cs)]
        hi = [min(o + s, (ci + 1) * q) for o, s, ci, q in zip(offset, shape, c, cs)]
        if any(x >= y for x, y in zip(lo, hi)):
            continue
        if not sharded:
            count += 1
            continue
        grid = [q // u for q, u in zip(cs, inner)]
        for e, u in enumerate(cc.units(a, obj)):
            if u is None:
                continue
            ic_ = np.unravel_index(e, grid)
            ulo = [ci * q + int(i) * w for ci, q, i, w in zip(c, cs, ic_, inner)]
            if all(max(o, x) < min(o + s, x + w)
                   for o, s, x, w in zip(offset, shape, ulo, inner)):
                count += 1
    return count
