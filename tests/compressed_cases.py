"""Seeded random cases of Array.write over compressed chains (blosc LZ4 and zstd, the two codecs
whose frames Array.write makes on the device), and the oracle-kept model of what a store must hold
after each write.  Shared by test_fuzz_compressed_host.py (CPU) and test_gpu_fuzz_compressed.py.

A case draws, from np.random.default_rng(seed): dtype, rank, bytes endianness, transpose order,
chunk / inner / array shapes (boundary chunks and boundary shards), codec parameters (blosc cname,
shuffle, blocksize, typesize; zstd checksum and level), the shard index's place, endianness and
crc32c, the fill value, the store and the write steps.  Three axes rotate with the seed instead, so
that every run of 42 consecutive seeds holds all their combinations: the format (seed % 3), the
codec ((seed // 3) % 2) and the large size band (seed % 7 == 3).  Test infrastructure only."""
import os
import struct

import numpy as np

import oracle as O
import zarrhip as z
from zarrhip import _abi as A
from zarrhip import v2

FORMATS = ("v3", "sharded", "v2")
CODECS = ("blosc", "zstd")
DTYPES = ("bool", "uint8", "int16", "uint16", "uint32", "float32", "float64", "uint64")
SHUFFLES = ("noshuffle", "shuffle", "bitshuffle")
EXPLICIT_TYPESIZES = (1, 3, 8, 17)
# a block size that is no multiple of any typesize above 1 used here (2, 3, 4, 8, 17); the second
# lies past the writer's 64 KiB clamp, for chunks that hold several such blocks
ODD_BLOCK, ODD_BLOCK_LARGE = 1001, 100001
FLOAT_FILLS = (0.0, -0.0, float("nan"), 1.5)
RAW_LIMIT = 1126 << 10        # the whole array: about 1 MiB raw

# ZH_FUZZ_CCASES widens the search (default 48 cases)
DEFAULT_SEEDS = 48
SEEDS = list(range(int(os.environ.get("ZH_FUZZ_CCASES", str(DEFAULT_SEEDS)))))


class Case:
    """meta(): fresh metadata; cls: z.Array or v2.Array; dtype: numpy dtype; store: "memory" or
    "files"; steps: [(offset or None, ndarray)]; axes: what was drawn, by name."""

    def __init__(self, meta, cls, dtype, store, steps, axes):
        self.meta, self.cls, self.dtype, self.store = meta, cls, dtype, store
        self.steps, self.axes = steps, axes


def _dims(rng, n, nel):
    """n sizes whose product is at most nel and near it."""
    dims, rem = [], max(1, int(nel))
    for d in range(n - 1):
        r = rem ** (1.0 / (n - d))
        x = min(int(rng.integers(1, max(2, int(2 * r) + 1))), rem)
        dims.append(x)
        rem = max(1, rem // x)
    dims.append(rem)
    return [int(x) for x in rng.permutation(dims)]


def _counts(rng, n, limit):
    """1..3 per axis, their product at most limit."""
    k = [int(rng.integers(1, 4)) for _ in range(n)]
    while int(np.prod(k)) > limit:
        k[int(np.argmax(k))] -= 1
    return k


def _box(rng, shape, grid):
    """A box of 1..2 grid cells per axis at a grid position, cut at the array."""
    sl = []
    for s, g in zip(shape, grid):
        lo = int(rng.integers(0, -(-s // g))) * g
        sl.append(slice(lo, min(s, lo + g * int(rng.integers(1, 3)))))
    return tuple(sl)


def _noise(rng, shape, dt):
    if dt == np.bool_:
        return rng.integers(0, 2, shape).astype(dt)
    n = int(np.prod(shape)) * dt.itemsize
    return rng.integers(0, 256, n, dtype=np.uint8).view(dt).reshape(shape)


def _mixture(rng, shape, dt, fill, grids):
    """Piecewise-constant runs, with boxes of noise and boxes of the fill value on the grids."""
    n = int(np.prod(shape))
    if dt == np.bool_:
        palette = np.array([0, 1], dt)
    elif dt.kind == "f":
        palette = np.array([1.0, -0.0, 2.5, 0.0, -3.75, 1e-3, -0.0, 7.0], dt)
    else:
        palette = rng.integers(0, 50, 8).astype(dt)
    m = n // 3 + 1
    lengths = rng.integers(3, min(400, max(5, n // 4)), m)
    a = np.repeat(palette[rng.integers(0, len(palette), m)], lengths)[:n].reshape(shape).copy()
    for _ in range(int(rng.integers(1, 3))):
        sl = _box(rng, shape, grids[int(rng.integers(len(grids)))])
        a[sl] = _noise(rng, a[sl].shape, dt)
    covered = np.zeros(shape, bool)
    for _ in range(int(rng.integers(1, 3))):
        sl = _box(rng, shape, grids[int(rng.integers(len(grids)))])
        more = covered.copy()
        more[sl] = True
        if 2 * int(more.sum()) <= a.size:   # at most half the array: the rest is a fill step's
            covered = more
            a[sl] = fill
    return a


def random_case(seed):
    rng = np.random.default_rng(seed)
    fmt = FORMATS[seed % 3]
    codec = CODECS[(seed // 3) % 2]
    sharded = fmt == "sharded"
    band = "large" if seed % 7 == 3 else ("tiny", "middle")[int(rng.random() < 0.6)]
    # an inner shape of an odd byte size: inner-chunk offsets in the shard at every alignment
    odd_inner = sharded and band != "large" and rng.random() < 0.45
    name = str(rng.choice(DTYPES[:2] if odd_inner else DTYPES))
    dt = np.dtype(name if name == "bool" else "<" + np.dtype(name).str[1:])
    ds = dt.itemsize
    n = int(rng.integers(1, 5))
    big = bool(ds > 1 and rng.random() < 0.5)
    order = None
    if fmt != "v2" and rng.random() < 0.5:
        order = [int(x) for x in rng.permutation(n)]

    # ---- shapes: the unit is what one frame holds (the inner chunk of a shard, else the chunk)
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
    shape = [k * c if rng.random() < 0.25 else int(rng.integers((k - 1) * c + 1, k * c + 1))
             for k, c in zip(counts, chunk)]

    # ---- fill
    if name == "bool":
        fill = bool(rng.integers(0, 2))
    elif dt.kind == "f":
        fill = FLOAT_FILLS[int(rng.integers(4))]
    else:
        fill = int(rng.choice([0, 0, 1, 3]))
    if fmt == "v2" and rng.random() < 0.25:
        fill = None
    np_fill = np.array(0 if fill is None else fill, dt)

    # ---- codec parameters
    ax = dict(seed=seed, format=fmt, codec=codec, band=band, dtype=name, rank=n, big=big,
              order=order, fill=fill, unit=unit, chunk=chunk, shape=shape, odd_inner=odd_inner)
    if codec == "blosc":
        cname = str(rng.choice(["lz4", "lz4hc"]))
        shuffle = SHUFFLES[int(rng.integers(3))]
        if band == "large":   # mostly blocks of 16 KiB and more: a leftover of 128 elements
            blocksize = int(rng.choice([0, ODD_BLOCK_LARGE, 4096, ODD_BLOCK_LARGE, 256]))
        else:
            blocksize = int(rng.choice([0, 256, 4096, ODD_BLOCK]))
        r = rng.random()
        if r < 0.5:
            ts_mode = int(rng.choice([t for t in EXPLICIT_TYPESIZES if t != ds]))
        else:
            ts_mode = "unset" if r < 0.65 and fmt != "v2" else "dtype"
        typesize = {"unset": None, "dtype": ds}.get(ts_mode, ts_mode)
        clevel = int(rng.integers(1, 10))
        ax.update(cname=cname, shuffle=shuffle, blocksize=blocksize, typesize=ts_mode,
                  frame_typesize=typesize or ds)
        # what the builders can express (v2's takes a block size, v3's does not)
        plain = ts_mode == "dtype" and (blocksize == 0 or fmt == "v2")
    else:
        checksum = bool(rng.random() < 0.5)
        level = int(rng.choice([1, 3, 5]))
        ax.update(checksum=checksum)
        plain = True
    if sharded:
        loc = ("start", "end")[int(rng.random() < 0.5)]
        index_big = bool(rng.random() < 0.5)
        index_crc = bool(rng.random() < 0.5)
        ax.update(index_location=loc, index_big=index_big, index_crc=index_crc)
        plain = plain and not index_big and index_crc
    builder = bool(plain and rng.random() < 0.6)
    store = ("memory", "files")[int(rng.random() < 0.4)]
    ax.update(builder=builder, store=store)
    endian = "big" if big else "little"

    def bb3():
        if codec == "blosc":
            return z.BloscCodec(cname, clevel, shuffle, typesize, blocksize)
        return z.ZstdCodec(level, checksum)

    def chain(c):
        """transpose?, bytes, the compressor: through the CodecBuilder."""
        if order is not None:
            c = c.withTranspose(order)
        c = c.withBytes(endian.upper())
        return c.withBlosc(cname, shuffle, clevel) if codec == "blosc" else \
            c.withZstd(level, checksum)

    def codecs3():
        """The same chain as codec objects."""
        cs = [z.TransposeCodec(order)] if order is not None else []
        return cs + [z.BytesCodec(None if ds == 1 else endian), bb3()]

    def meta():
        if fmt == "v2":
            b = (v2.ArrayMetadataBuilder().withShape(shape).withChunks(chunk)
                 .withDataType(getattr(v2.DataType, name.upper() + ("_BE" if big else "")))
                 .withFillValue(fill))
            if codec == "zstd":
                return b.withZstdCompressor(level, checksum).build()
            if builder:
                return b.withBloscCompressor(cname, shuffle, clevel, blocksize).build()
            # typesize 0: the dtype's, as the metadata fills it in
            return b.withCompressor(v2.BloscCodec(cname, clevel, shuffle,
                                                  0 if ts_mode == "dtype" else typesize,
                                                  blocksize)).build()
        b = (z.ArrayMetadataBuilder().withShape(shape).withDataType(name).withChunkShape(chunk)
             .withFillValue(fill))
        if not sharded:
            if builder:
                return b.withCodecs(chain).build()
            b.codecs = codecs3()
            return b.build()
        if builder:
            return b.withCodecs(lambda c: c.withSharding(unit, chain, loc)).build()
        index = [z.BytesCodec("big" if index_big else "little")] + \
            ([z.Crc32cCodec()] if index_crc else [])
        b.codecs = [z.ShardingIndexedCodec(unit, codecs3(), index, loc)]
        return b.build()

    # ---- the write steps
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
            c0 = [int(rng.integers(0, k)) for k in counts]
            c1 = [int(rng.integers(a + 1, k + 1)) for a, k in zip(c0, counts)]
            off = [a * c for a, c in zip(c0, chunk)]
            end = [min(b * c, s) for b, c, s in zip(c1, chunk, shape)]
            if kind == "fill" and rng.random() < 0.5:
                d = int(rng.integers(n))
                off[d] = max(0, off[d] - int(rng.integers(1, chunk[d] + 1)))
            shp = [e - o for e, o in zip(end, off)]
        if kind == "fill":
            data = np.full(shp, np_fill, dt)
        else:
            whole = _mixture(rng, shape, dt, np_fill, grids)
            data = np.ascontiguousarray(whole[tuple(slice(o, o + k) for o, k in zip(off, shp))])
        steps.append((off, data))
    ax.update(steps=kinds)
    return Case(meta, v2.Array if fmt == "v2" else z.Array, dt, store, steps, ax)


# ---- the model: what the store must hold, kept with the oracle ---------------------------------
def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def aligned(a, offset, data):
    """The write covers whole chunks (no read-modify-write)."""
    cs, shape = a.metadata.chunk_shape, a.metadata.shape
    offset = [0] * a.ndim if offset is None else offset
    return all(o % c == 0 and ((o + k) % c == 0 or o + k == s)
               for o, k, c, s in zip(offset, data.shape, cs, shape))


class Model:
    """{chunk coords: the object before the compressor, or None for an absent key} of an array
    (`a`: only its metadata and zh_array_meta are used), advanced by the oracle alone."""

    def __init__(self, a):
        self.a, self.n = a, a.ndim
        self.shape = list(a.metadata.shape)
        self.cs = list(a.metadata.chunk_shape)
        self.dt = a.metadata.data_type.numpy
        self.coords = O.compute_chunk_coords(self.shape, self.cs, [0] * self.n, self.shape)
        self.objs = {c: None for c in self.coords}
        # no fill value (v2 "fill_value": null): a chunk of zeros is stored, never deleted
        self.keep = getattr(a.metadata, "fill_value", 0) is None

    def read(self, offset=None, shape=None):
        raw = O.array_read(self.a.zmeta, [self.objs[c] for c in self.coords], [0] * self.n,
                           self.shape)
        out = np.frombuffer(raw, self.dt).reshape(self.shape)
        if offset is None:
            return out
        return out[tuple(slice(o, o + k) for o, k in zip(offset, shape))]

    def write(self, offset, data):
        """→ {coords: object or None} of the chunks this write sets or deletes."""
        offset = [0] * self.n if offset is None else list(offset)
        lo = [(o // c) * c for o, c in zip(offset, self.cs)]
        hi = [min(-(-(o + k) // c) * c, s)
              for o, k, c, s in zip(offset, data.shape, self.cs, self.shape)]
        ext = [h - l for l, h in zip(lo, hi)]
        hull = self.read(lo, ext).copy()
        hull[tuple(slice(o - l, o - l + k) for o, l, k in zip(offset, lo, data.shape))] = data
        objs = O.array_write(self.a.zmeta, hull.tobytes(), lo, ext)
        coords = O.compute_chunk_coords(self.shape, self.cs, lo, ext)
        assert len(objs) == len(coords)
        changed = {}
        for c, o in zip(coords, objs):
            if o is None and self.keep:
                o = bytes(int(np.prod(self.cs)) * self.dt.itemsize)
            self.objs[c] = changed[c] = o
        return changed


def shard_entries(a, shard):
    """([(offset, nbytes) or None] per inner chunk, index size) of a shard (the oracle's or a stored
    one), its index read with the chain's own place, endianness and crc32c; the crc is checked."""
    ch = a.chain.chain
    n = a._n_inner()
    crc = bool(ch["index_crc32c"])
    isz = 16 * n + (4 if crc else 0)
    assert len(shard) >= isz
    idx = shard[:isz] if ch["index_location"] == A.ZH_INDEX_START else shard[len(shard) - isz:]
    fmt = ">QQ" if ch["index_endian"] == A.ZH_ENDIAN_BIG else "<QQ"
    ents = [struct.unpack(fmt, idx[16 * e:16 * e + 16]) for e in range(n)]
    if crc:
        assert struct.unpack("<I", idx[16 * n:])[0] == O.crc32c(idx[:16 * n])
    for off, nb in ents:
        assert (off == 2 ** 64 - 1) == (nb == 2 ** 64 - 1)
    return [None if off == 2 ** 64 - 1 else (off, nb) for off, nb in ents], isz


def units(a, obj):
    """The pieces of an uncompressed object that the compressor sees one at a time: the chunk,
    or the inner chunks of a shard ([bytes or None])."""
    if not a.chain.chain["sharded"]:
        return [obj]
    ents, _ = shard_entries(a, obj)
    return [None if e is None else obj[e[0]:e[0] + e[1]] for e in ents]


def stored_objects(a):
    """{chunk coords: stored bytes or None} over the whole array."""
    shape = list(a.metadata.shape)
    out = {}
    for c in a._chunk_coords([0] * len(shape), shape):
        h = a._handle(c)
        out[c] = bytes(h.read()) if h.exists() else None
    return out


def bb_codec(a):
    """The chain's one compressor object."""
    return (a.chain.inner_host_bb if a.chain.chain["sharded"] else a.chain.host_bb)[0]
