"""v3 Array — the read/write surface of dev.zarr.zarrjava.v3.Array / core.Array, with the
chunk codec work done by the HIP path through the C-ABI (libzarrhip.so).

  Array.open / create        M/v3/Array.java:41-50, 142-154
  read(offset, shape)        M/core/Array.java:378-441   → zh_array_read (one call, all chunks;
                                                          zh_array_read_multi over ZH_DEVICES)
  readChunk(coords)          M/core/Array.java:167-182
  write(offset, data)        M/core/Array.java:83-133    → zh_array_write (whole chunks)
  access()                   M/core/Array.java:483-536   (ArrayAccessor)

Byte-to-byte compressors stay on the host (north star): their frames are decoded here and
the raw chunk bytes are handed to the device — except blosc and zstd frames
and gzip members, which one batched call decodes on the device when the codec is the chain's only
host stage (ZH_BLOSC_DEVICE, zh_blosc_decode_batch; ZH_ZSTD_DEVICE, zh_zstd_decode_batch;
ZH_GZIP_DEVICE, zh_gzip_decode_batch), and blosc LZ4 and zstd frames, which Array.write
compresses on the device (ZH_BLOSC_ENCODE_DEVICE, zh_blosc_encode_batch; ZH_ZSTD_ENCODE_DEVICE,
zh_zstd_encode_batch), as it does gzip members when asked to (ZH_GZIP_ENCODE_DEVICE=1, or 2
for dynamic-Huffman segments as well; zh_gzip_encode_batch) and blosc frames with zstd streams
(ZH_BLOSC_ZSTD_ENCODE=1; zh_blosc_encode_batch_ex) or zlib streams (ZH_BLOSC_ZLIB_ENCODE=1 or 2).
"""
import atexit
import ctypes as C
import json
import os
import struct
import time
import threading

import numpy as np

from . import _abi as A
from . import _lib
from .codecs import BloscCodec, GzipCodec, ZstdCodec, device_chain, host_bb_decode, host_bb_encode
from .errors import UnsupportedChainError, ZarrException, raise_for
from .metadata import ZARR_JSON, ArrayMetadata

_ctx = None
_ctx_lock = threading.Lock()

# ZH_BLOSC_DEVICE: chains whose only host byte-to-byte stage is blosc hand their frames to the
# device in one batch (zh_blosc_decode_batch) instead of decoding them here one at a time.
# The default follows the measurement in DESIGN.md ("Blosc frames on the device").
BLOSC_DEVICE_DEFAULT = "1"
# ZH_BLOSC_ZSTD_DEVICE: on that route, "1" passes ZH_BLOSC_ZSTD_DEVICE to the batch, so frames
# whose streams are plain zstd frames (c-blosc's, and the codec's default cname) are decoded on
# the device as well; "0" passes no flag and such frames are decoded by zh_blosc_decompress inside
# the batch call, as before.  The default follows the measurement in DESIGN.md ("Blosc zstd
# streams on the device").
BLOSC_ZSTD_DEVICE_DEFAULT = "0"
# ZH_BLOSC_ZLIB_DEVICE: on the same route, "1" passes ZH_BLOSC_ZLIB_DEVICE to the batch, so frames
# whose streams are zlib streams with compress2's header (c-blosc's for cname zlib) are inflated
# on the device as well; "0" passes no flag and such frames are decoded by zh_blosc_decompress
# inside the batch call, as before.  The measurement is in DESIGN.md ("Blosc zlib streams on the
# device").
BLOSC_ZLIB_DEVICE_DEFAULT = "0"
# ZH_ZSTD_DEVICE: the same for chains whose only host byte-to-byte stage is zstd
# (zh_zstd_decode_batch).  "0": the host route; "2": every eligible read goes to the device;
# "1" (the default): the rule of DESIGN.md ("Zstd frames on the device"), a read goes to the
# device when it holds at least ZSTD_DEVICE_MIN_FRAMES frames.  In the record
# (profiles/zstd_decode/lab.json) few large frames lose outright and many small frames do not
# clear the rule's margin on every array, so the default sends nothing to the device:
# ZSTD_DEVICE_MIN_FRAMES is None, and the device route is behind ZH_ZSTD_DEVICE=2.
ZSTD_DEVICE_DEFAULT = "1"
ZSTD_DEVICE_MIN_FRAMES = None
# ZH_GZIP_DEVICE: the same for chains whose only host byte-to-byte stage is one v3 GzipCodec
# (zh_gzip_decode_batch), with the same three values.  "1" (the default) follows the rule of
# DESIGN.md ("Gzip members on the device"): a read goes to the device when it holds at least
# GZIP_DEVICE_MIN_FRAMES members.  In the record (profiles/gzip_decode/lab.json) few large members
# lose outright and many small members have the lower median but not by more than the spread, so
# the default sends nothing to the device: GZIP_DEVICE_MIN_FRAMES is None, and the device route is
# behind ZH_GZIP_DEVICE=2.
GZIP_DEVICE_DEFAULT = "1"
GZIP_DEVICE_MIN_FRAMES = None
# ZH_BLOSC_ENCODE_DEVICE: Array.write compresses a blosc LZ4 chain's frames on the device in one
# batch (zh_blosc_encode_batch) instead of copying every raw chunk back and compressing it here.
# It stays "1" whatever the write times say: the stored size is what the codec was asked for,
# and both routes store the same bytes (DESIGN.md "Blosc frames encoded on the device").
BLOSC_ENCODE_DEVICE_DEFAULT = "1"
# ZH_BLOSC_ZSTD_ENCODE (read by BloscCodec, codecs.py; default "0"): "1" compresses a blosc chain
# whose cname is zstd, the codec's default, with zstd streams (zh_blosc_compress_ex /
# zh_blosc_encode_batch_ex with ZH_BLOSC_ENC_ZSTD) on the route ZH_BLOSC_ENCODE_DEVICE names;
# unset, such a chain is stored as MEMCPYED frames.  It is opt-in because it changes stored bytes
# (DESIGN.md "Blosc zstd frames encoded on the device").
# ZH_BLOSC_ZLIB_ENCODE (read by BloscCodec; default "0"): the same for cname zlib.  "1": zlib
# streams of stored and fixed segments (ZH_BLOSC_ENC_ZLIB); "2": dynamic segments as well
# (ZH_BLOSC_ENC_DYNAMIC); any other value: MEMCPYED frames (DESIGN.md "Blosc frames with zlib
# streams encoded on the device").
# ZH_ZSTD_ENCODE_DEVICE: the same for a zstd chain (zh_zstd_encode_batch), and "1" for the same
# reason (DESIGN.md "Zstd frames encoded on the device").
ZSTD_ENCODE_DEVICE_DEFAULT = "1"
# ZH_GZIP_ENCODE_DEVICE: "1" sends a gzip chain's members to the device (zh_gzip_encode_batch)
# with stored and fixed-Huffman segments only, so bytes that LZ alone does not shrink are stored
# where zlib would still compress them; "2" does the same with dynamic-Huffman segments in the
# per-block choice (zh_gzip_enc_params::dynamic = 1).  The default is "0" (DESIGN.md "Gzip
# members encoded on the device" and "Dynamic-Huffman segments"): with the switch unset every
# stored byte is zlib's.
GZIP_ENCODE_DEVICE_DEFAULT = "0"


class _Deferred:
    """A store or index error of one chunk's load, kept until the chunks before it have had
    their frames decoded: the first error in chunk order is the one a read reports."""

    def __init__(self, exc):
        self.exc = exc


def _raise_blosc(err):
    """A _lib.ZhError of the batched blosc decode as BloscCodec.decode raises it."""
    if err.status == A.ZH_EUNSUPPORTED:
        raise UnsupportedChainError(str(err)) from None
    if err.status in (A.ZH_EDATA, A.ZH_EINVAL):
        raise ZarrException(f"Error in decoding blosc: {err}") from None
    raise_for(err)


def _raise_zstd(err):
    """A _lib.ZhError of the batched zstd decode as ZstdCodec.decode raises it."""
    if err.status == A.ZH_EUNSUPPORTED:
        raise UnsupportedChainError(str(err)) from None
    if err.status in (A.ZH_EDATA, A.ZH_EINVAL):
        raise ZarrException(f"Error in decoding zstd: {err}") from None
    raise_for(err)


def _raise_gzip(err):
    """A _lib.ZhError of the batched gzip decode as the reference's GzipCodec.decode raises it
    (M/v3/codec/core/GzipCodec.java:42-43)."""
    if err.status in (A.ZH_EDATA, A.ZH_EINVAL):
        raise ZarrException("Error in decoding gzip.") from None
    raise_for(err)


def device():
    """The process-wide DeviceContext (GPU ZH_DEVICE, default LOCAL_RANK or 0)."""
    global _ctx
    with _ctx_lock:
        if _ctx is None:
            dev = int(os.environ.get("ZH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            _ctx = _lib.DeviceContext(dev)
        return _ctx


_multi = {}


def devices():
    """DeviceContexts of ZH_DEVICES="0,1,..." (one per listed GPU, a GPU may repeat), or
    [device()]: Array.read spreads a region over them (zh_array_read_multi)."""
    spec = os.environ.get("ZH_DEVICES", "")
    ids = [int(x) for x in spec.split(",") if x.strip()]
    if len(ids) <= 1:
        return [device()]
    with _ctx_lock:
        if spec not in _multi:
            _multi[spec] = [_lib.DeviceContext(i) for i in ids]
        return _multi[spec]


def _parallel(fn, jobs, width=8):
    """Run fn over jobs on up to `width` threads (store reads release the GIL)."""
    if len(jobs) <= 1:
        for j in jobs:
            fn(j)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(width, len(jobs))) as ex:
        for _ in ex.map(fn, jobs):
            pass


class StagingPool:
    """Host staging buffers (store bytes on their way to the device), reused across reads.
    A fresh multi-GiB numpy buffer per read pays twice: its pages fault in while the store
    read fills it, and they are unmapped when it is dropped at the end of the read (a 2 GiB
    sub-shard read: 194 ms inside Array.read, 283 ms around it).  The reference's JVM heap
    keeps such memory; this pool does the same for the mirror.  Buffers are kept up to `cap`
    bytes; `release()` returns them.

    Buffers of at least `pin_min` bytes are page-aligned, and page-locked (zh_host_register
    through the process's DeviceContext, `pin`) when the pool hands one out a second time, so
    repeated reads' H2D copies run as direct DMA instead of through the runtime's pageable
    staging, while a one-off buffer (or one the cap keeps evicting) never pays for pinning
    (≈40 ms per GiB).  Pinned buffers are unregistered before the pool lets go of them.
    Without a usable device (CPU-only use, or a failing registration) they stay pageable."""
    ROUND = 64 << 20
    PAGE = 4096

    def __init__(self, cap=8 << 30, pin=None, pin_min=64 << 20):
        self.cap = cap
        self.pin = pin  # callable returning a DeviceContext, or None: pageable buffers
        self.pin_min = pin_min
        self._free = []
        self._pinned = {}  # id(buffer) -> (context, address)
        self._lock = threading.Lock()

    def _alloc(self, size):
        if self.pin is None or size < self.pin_min:
            return np.empty(size, np.uint8)
        raw = np.empty(size + self.PAGE, np.uint8)
        a = (-raw.ctypes.data) % self.PAGE
        return raw[a:a + size]  # page-aligned; keeps `raw` alive through .base

    def _register(self, b):  # caller holds the lock
        if self.pin is None or b.nbytes < self.pin_min or id(b) in self._pinned:
            return
        try:
            ctx = self.pin()
            ctx.host_register(b.ctypes.data, b.nbytes)
            self._pinned[id(b)] = (ctx, b.ctypes.data)
        except Exception:  # no device or registration refused: stays pageable
            pass

    def _drop(self, b):
        rec = self._pinned.pop(id(b), None)
        if rec is not None:
            rec[0].host_unregister(rec[1])

    def take(self, n, lease):
        """A uint8 view of at least n bytes; its buffer is appended to `lease` (give back
        with give(lease) once the device has consumed it)."""
        with self._lock:
            fit = [i for i, x in enumerate(self._free) if x.nbytes >= n]
            b = self._free.pop(min(fit, key=lambda i: self._free[i].nbytes)) if fit else None
            if b is not None:
                self._register(b)  # second use: worth page-locking
        if b is None:
            b = self._alloc(max(1, -(-n // self.ROUND) * self.ROUND) if n > self.ROUND else
                            max(n, 1))
        lease.append(b)
        return b[:n]

    def give(self, lease):
        with self._lock:
            self._free.extend(lease)
            tot = sum(b.nbytes for b in self._free)
            while tot > self.cap and self._free:  # drop the oldest first
                b = self._free.pop(0)
                tot -= b.nbytes
                self._drop(b)
        lease.clear()

    def pinned_bytes(self):
        with self._lock:
            return sum(b.nbytes for b in self._free if id(b) in self._pinned)

    def release(self):
        with self._lock:
            for b in self._free:
                self._drop(b)
            self._free.clear()


staging_pool = StagingPool(pin=lambda: devices()[0])
atexit.register(staging_pool.release)  # unregister before the buffers' memory goes


def _new_buf(n, lease=None):
    return np.empty(n, np.uint8) if lease is None else staging_pool.take(n, lease)


def _read_whole(h, piece=64 << 20, lease=None):
    """StoreHandle.read() of a whole chunk; stores that report sizes are read in parallel
    pieces straight into one buffer (a 4 GiB shard is one bytes copy otherwise)."""
    n = h.size() if hasattr(h, "size") else None
    if n is None or n <= piece:
        return h.read()
    out = _new_buf(n, lease)
    mv = memoryview(out)

    def fetch(o):
        ln = min(piece, n - o)
        got = h.read_into(mv[o:o + ln], o, o + ln)
        if got is None or got < ln:
            raise ZarrException(f"Could not load byte data of {h!r}")
    _parallel(fetch, list(range(0, n, piece)))
    return out


def _host_buf(b):
    return (C.c_char * max(1, len(b))).from_buffer_copy(bytes(b) if len(b) else b"\0")


class Array:
    def __init__(self, store_handle, metadata):
        self.storeHandle = store_handle
        self.metadata = metadata
        self.staged_bytes = 0  # encoded bytes read from the store and handed to the device
        self._stage_lock = threading.Lock()  # chunk loads run on several threads
        self.chain = device_chain(metadata.codecs, metadata.ndim,
                                  metadata.data_type.getByteCount(), metadata.chunk_shape)
        self.zmeta = metadata.to_zh_meta(self.chain)
        err = C.create_string_buffer(512)
        st = _lib.lib().zh_validate_meta(C.byref(self.zmeta), err, 512)
        if st != A.ZH_OK:
            raise_for(_lib.ZhError(st, err.value.decode()))

    # ---------------------------------------------------------------- open / create
    META_FILE = ZARR_JSON          # v2.Array: ".zarray"
    METADATA = ArrayMetadata

    @classmethod
    def open(cls, store_handle):
        raw = store_handle.resolve(cls.META_FILE).read()
        if raw is None:
            raise ZarrException(f"No Zarr array found at {store_handle!r}")
        return cls(store_handle, cls.METADATA.from_json(json.loads(raw)))

    @classmethod
    def create(cls, store_handle, metadata, exist_ok=False):
        h = store_handle.resolve(cls.META_FILE)
        if not exist_ok and h.exists():
            raise ZarrException(f"Trying to create a new array in {store_handle!r}. But "
                                f"{cls.META_FILE} already exists.")
        h.set(metadata.dumps().encode())
        return cls(store_handle, metadata)

    # ---------------------------------------------------------------- helpers
    @property
    def ndim(self):
        return self.metadata.ndim

    def _chunk_coords(self, offset, shape):
        n = self.ndim
        L = _lib.lib()
        args = (n, _lib.i64arr(self.metadata.shape), _lib.i32arr(self.metadata.chunk_shape),
                _lib.i64arr(offset), _lib.i64arr(shape))
        num = L.zh_compute_chunk_coords(*args, None, 0)
        if num < 0:
            raise ArithmeticError("Number of chunks exceeds Integer.MAX_VALUE")
        out = (C.c_int64 * max(1, num * n))()
        L.zh_compute_chunk_coords(*args, out, num)
        return [tuple(out[i * n:(i + 1) * n]) for i in range(num)]

    def _handle(self, coords):
        return self.storeHandle.resolve(*self.metadata.chunk_key_encoding.encode_chunk_key(coords))

    def _check_region(self, offset, shape):
        n = self.ndim
        if len(offset) != n:
            raise ValueError(f"'offset' needs to have rank '{n}'.")
        if len(shape) != n:
            raise ValueError(f"'shape' needs to have rank '{n}'.")
        for d in range(n):  # M/core/Array.java:386-390
            if offset[d] < 0 or offset[d] + shape[d] > self.metadata.shape[d]:
                raise ZarrException("Requested data is outside of the array's domain.")

    def _count_staged(self, n):
        with self._stage_lock:
            self.staged_bytes += n

    def _n_inner(self):
        inner = self.chain.chain["inner_chunk_shape"]
        n = 1
        for c, i in zip(self.metadata.chunk_shape, inner):
            n *= c // i
        return n

    def _wrap_inner(self, shard, info=None):
        """Inverse of _unwrap_inner for the write path."""
        ch = self.chain.chain
        n_in = self._n_inner()
        crc = ch["index_crc32c"]
        isz = 16 * n_in + (4 if crc else 0)
        start = ch["index_location"] == A.ZH_INDEX_START
        idx = shard[:isz] if start else shard[len(shard) - isz:]
        body = idx[:16 * n_in]
        fmt = ">QQ" if ch["index_endian"] == A.ZH_ENDIAN_BIG else "<QQ"
        pos = isz if start else 0
        payload, new = [], []
        for k in range(n_in):
            off, nb = struct.unpack(fmt, body[16 * k:16 * k + 16])
            if off == 2 ** 64 - 1:
                new.append((off, nb))
                continue
            if info is not None:
                info["raw_bytes"] += nb
            enc = self._bb_encode(self.chain.inner_host_bb, shard[off:off + nb], info)
            new.append((pos, len(enc)))
            payload.append(enc)
            pos += len(enc)
        ib = b"".join(struct.pack(fmt, *e) for e in new)
        if crc:
            ib = self.chain.index_codecs[1].encode(ib)
        pb = b"".join(payload)
        return ib + pb if start else pb + ib

    def _stage_shard(self, h, part_lo, part_hi, lease, full=False, collect=False):
        """StoreHandleDataProvider semantics (ShardingIndexedCodec.java:190-230, 333-357): one
        range read for the index, zh_shard_ranges for the inner chunks the part references,
        one store read per range (in parallel, straight into one pooled buffer).  The stored
        index goes to the device unchanged — its crc32c and entries are checked there, never
        here — so a corrupt entry cannot size a host allocation.  Inner host byte-to-byte
        stages (zstd, gzip, blosc) are undone per inner chunk: those pieces hold the raw
        payload.  A range the store cannot deliver is left out (the device then reports the
        reference's "Could not load byte data for chunk").  `full`: the part is the whole shard
        (decodePartial → chunkHandle.read() → ByteBufferDataProvider, :246-251, 301-331), so
        the shard is the file as it is — an entry beyond its bytes is an error (Q14), not a
        zero-padded range.  `collect` (the device blosc / zstd route): the inner chunks' frames are
        kept as read, as pieces (offset, stored bytes, frame, None), for one batched decode of
        the whole read.  Returns a ShardSource plus the buffers it points into, or None for
        a missing shard."""
        if not h.exists():
            return None
        isz = _lib.lib().zh_shard_index_size(C.byref(self.zmeta))
        start = self.chain.chain["index_location"] == A.ZH_INDEX_START
        try:
            idx = h.read(0, isz) if start else h.read(-isz)
        except ValueError:  # a suffix longer than the file (the reference's position(< 0))
            idx = h.read()  # what it holds: the device reports "Shard [...] smaller than its index"
        if idx is None:
            return None
        idx = bytes(idx)
        from .store import FilesystemStore
        size = h.size() if hasattr(h, "size") else None
        # a FilesystemStore range read past the end of the file returns zeros
        # (FilesystemStore.get(keys, start, end), FilesystemStore.java:84-102): no entry is out
        # of reach by its offset, so the shard size bounds nothing
        if full and size is not None:
            size = int(size)  # the whole object: sliced, never padded (zh_files.cpp file_sources)
        else:
            size = -1 if size is None or isinstance(h.store, FilesystemStore) else int(size)
        ibuf = np.frombuffer(idx if idx else b"\0", np.uint8)
        keep = [ibuf]
        self._count_staged(len(idx))
        if len(idx) < isz:  # the device reports "Shard [..] is smaller than its index"
            return _lib.ShardSource(ibuf.ctypes.data, len(idx), size, []), keep
        host = self.chain.inner_host_bb
        if host or size < 0:
            # the index decides host work before the device sees it (host decodes of every
            # referenced range; range reads bounded by nothing but the entries): check its
            # crc32c first, as the reference does (ShardingIndexedCodec.java:205)
            try:
                _lib.shard_index_check(self.zmeta, idx)
            except _lib.ZhError as e:
                raise_for(e)
        rs = _lib.shard_ranges(self.zmeta, idx, size, part_lo, part_hi,
                               0 if host else 64 << 20)
        pieces = []
        if host:  # per inner chunk: undo the host codecs
            for o, nb in rs:
                if full and 0 <= size < o + nb:  # beyond the object: left out, the device reports it
                    continue
                blob = h.read(o, o + nb)
                if blob is None or len(blob) < nb:
                    continue
                self._count_staged(nb)
                if collect:
                    pieces.append((o, nb, blob, None))
                    continue
                raw = np.frombuffer(host_bb_decode(host, blob) or b"\0", np.uint8)
                keep.append(raw)
                pieces.append((o, nb, raw.ctypes.data, len(raw)))
            return _lib.ShardSource(ibuf.ctypes.data, len(idx), size, pieces), keep
        buf = _new_buf(max(1, sum(nb for _, nb in rs)), lease)
        keep.append(buf)
        mv = memoryview(buf)
        jobs, pos = [], 0
        for o, nb in rs:
            jobs.append((pos, o, nb))
            pos += nb
        got = [0] * len(jobs)

        def fetch(k):
            p0, o, nb = jobs[k]
            g = h.read_into(mv[p0:p0 + nb], o, o + nb)
            got[k] = g or 0
        _parallel(fetch, list(range(len(jobs))))
        for k, (p0, o, nb) in enumerate(jobs):
            if got[k] >= nb:
                self._count_staged(nb)
                pieces.append((o, nb, buf.ctypes.data + p0, nb))
        return _lib.ShardSource(ibuf.ctypes.data, len(idx), size, pieces), keep

    def _load_source(self, coords, part_lo=None, part_hi=None, lease=None):
        """One stored chunk / shard of a read: None (missing key), ("whole", bytes-like), or
        ("pieces", ShardSource, keepalive) for a sharded part."""
        h = self._handle(coords)
        ch = self.chain.chain
        if ch["sharded"]:
            n = self.ndim
            if part_lo is None:
                part_lo, part_hi = [0] * n, list(self.metadata.chunk_shape)
            full = all(lo == 0 and hi == c for lo, hi, c in
                       zip(part_lo, part_hi, self.metadata.chunk_shape))
            if not full or self.chain.inner_host_bb:  # the index + the referenced ranges
                st = self._stage_shard(h, part_lo, part_hi, lease, full)
                return None if st is None else ("pieces",) + st
        # raw payloads go to the device as they are: parallel reads into one buffer; host
        # byte-to-byte stages take the store's bytes
        b = h.read() if self.chain.host_bb else _read_whole(h, lease=lease)
        if b is None:
            return None
        self._count_staged(len(b))
        if self.chain.host_bb:
            b = host_bb_decode(self.chain.host_bb, b)
        return ("whole", b)

    def _file_paths(self, coords, devs):
        """The chunk files of a read that zh_array_read_files(_multi) can do (FilesystemStore,
        a chain without host byte-to-byte stages; ZH_FILES=0 keeps the store reads here), in
        computeChunkCoords order, else None.  The reads themselves follow
        FilesystemStore.exists / get (M/store/FilesystemStore.java:43-102) in the library."""
        from .store import FilesystemStore
        st = self.storeHandle.store
        if (not isinstance(st, FilesystemStore) or self.chain.host_bb or
                self.chain.inner_host_bb or os.environ.get("ZH_FILES", "1") == "0"):
            return None
        return [st._p(self._handle(c).keys) for c in coords]

    def _file_store(self):
        """The FilesystemStore the chunk files belong to, as (root, FilesystemStore.toString())
        for StoreException's text."""
        st = self.storeHandle.store
        return (st.path, repr(st))

    # ---------------------------------------------------------------- read
    def read(self, offset=None, shape=None, parallel=True):
        """core.Array.read → numpy array (C order, the array's dtype)."""
        t_enter = time.perf_counter()
        n = self.ndim
        offset = [0] * n if offset is None else [int(o) for o in offset]
        shape = list(self.metadata.shape) if shape is None else [int(s) for s in shape]
        self._check_region(offset, shape)
        dt = self.metadata.data_type.numpy
        if any(s == 0 for s in shape):
            return np.zeros(shape, dtype=dt)
        out = np.empty(shape, dtype=dt)
        self._read_into(offset, shape, out.ctypes.data, 0, devices(), parallel, t_enter)
        return out

    def read_into(self, offset, shape, out_addr, dev=None, parallel=True):
        """core.Array.read into caller-owned HOST memory at out_addr (C order, the array's
        dtype; page-locked memory is DMA'd straight into): the per-rank decode of
        zarrhip.parallel.SharedHostRegion.  `dev`: the DeviceContext to read with (default: the
        process's contexts, as read())."""
        t_enter = time.perf_counter()
        offset = [int(o) for o in offset]
        shape = [int(s) for s in shape]
        self._check_region(offset, shape)
        if any(s == 0 for s in shape):
            return
        self._read_into(offset, shape, int(out_addr), 0,
                        [dev] if dev is not None else devices(), parallel, t_enter)

    def read_device(self, offset, shape, out_ptr, dev=None, parallel=True):
        """core.Array.read delivered to device memory: the C-order region is written to
        `out_ptr` on `dev`'s device (a DeviceContext; default the first context) and nothing
        is copied back to the host (ZH_OUT_DEVICE).  The store I/O is the same as read()'s
        (for a FilesystemStore the library's own file reads).  The per-rank decode of
        zarrhip.parallel.array_decoder."""
        t_enter = time.perf_counter()
        offset = [int(o) for o in offset]
        shape = [int(s) for s in shape]
        self._check_region(offset, shape)
        if any(s == 0 for s in shape):
            return
        self._read_into(offset, shape, int(out_ptr), A.ZH_OUT_DEVICE,
                        [dev if dev is not None else device()], parallel, t_enter)

    def _read_into(self, offset, shape, out_addr, flags, devs, parallel, t_enter):
        """The device read of a checked, non-empty region into out_addr (host memory, or
        device memory with flags ZH_OUT_DEVICE and one context)."""
        coords = self._chunk_coords(offset, shape)
        t0 = time.perf_counter()
        paths = self._file_paths(coords, devs)
        if paths is not None:  # the library reads the store's files itself
            t1 = time.perf_counter()
            try:
                if len(devs) > 1:  # one slab per device, each over its own PCIe link
                    _lib.array_read_files_multi(devs, self.zmeta, paths, offset, shape,
                                                out_addr, flags, store=self._file_store())
                else:
                    devs[0].array_read_files(self.zmeta, paths, offset, shape, out_addr,
                                             flags, store=self._file_store())
            except _lib.ZhError as e:
                raise_for(e)
            self.last_read_timing = {"prep_s": t0 - t_enter, "stage_s": t1 - t0,
                                     "device_s": time.perf_counter() - t1, "files": True}
            return
        if self._blosc_device(devs):
            self._read_frames_device(coords, offset, shape, out_addr, flags, devs[0], parallel,
                                     t_enter, t0, self._blosc_decode_batch(devs[0]), _raise_blosc,
                                     "blosc")
            return
        if self._zstd_device(devs, coords):
            self._read_frames_device(coords, offset, shape, out_addr, flags, devs[0], parallel,
                                     t_enter, t0, devs[0].zstd_decode_batch, _raise_zstd, "zstd")
            return
        if self._gzip_device(devs, coords):
            self._read_frames_device(coords, offset, shape, out_addr, flags, devs[0], parallel,
                                     t_enter, t0, devs[0].gzip_decode_batch, _raise_gzip, "gzip")
            return
        lease = []  # staging buffers of this read, back to the pool after the device read
        sharded = self.chain.chain["sharded"]
        try:
            def load(c):
                lo = [max(o, ci * cs) - ci * cs
                      for o, ci, cs in zip(offset, c, self.metadata.chunk_shape)]
                hi = [min(o + s, (ci + 1) * cs) - ci * cs
                      for o, s, ci, cs in zip(offset, shape, c, self.metadata.chunk_shape)]
                return self._load_source(c, lo, hi, lease)
            if parallel and len(coords) > 1:  # the store reads of the chunks, concurrently
                # (core.Array.read's parallel stream over chunks, M/core/Array.java:403-407)
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=min(8, len(coords))) as ex:
                    sources = list(ex.map(load, coords))
            else:
                sources = [load(c) for c in coords]
            t1 = time.perf_counter()
            n_frames = sum(
                0 if s is None else len(s[1].pieces) if s[0] == "pieces" else 1 for s in sources)
            n_blosc = n_frames if self._blosc_chain() else 0
            n_zstd = n_frames if self._zstd_chain() else 0
            n_gzip = n_frames if self._gzip_chain() else 0
            keep = []
            try:
                if sharded:  # index + pieces (or whole objects as one piece at 0)
                    shards = []
                    for s in sources:
                        if s is None:
                            shards.append(None)
                        elif s[0] == "pieces":
                            shards.append(s[1])
                            keep.append(s[2])
                        else:
                            v = np.frombuffer(s[1], np.uint8) if len(s[1]) else \
                                np.zeros(1, np.uint8)
                            keep.append(v)
                            shards.append(_lib.ShardSource(None, 0, len(s[1]),
                                                           [(0, len(s[1]), v.ctypes.data,
                                                             len(s[1]))]))
                    if len(devs) > 1:
                        _lib.array_read_pieces_multi(devs, self.zmeta, shards, offset, shape,
                                                     out_addr, flags)
                    else:
                        devs[0].array_read_pieces(self.zmeta, shards, offset, shape,
                                                  out_addr, flags)
                else:
                    # views of the staged bytes (the library only reads them); an empty but
                    # present chunk keeps a non-null pointer (null = missing key → fill)
                    bufs = [None if s is None else
                            np.frombuffer(s[1] if len(s[1]) else b"\0", np.uint8)
                            for s in sources]
                    keep.append(bufs)
                    srcs = [((int(b.ctypes.data), len(s[1])) if s is not None else (None, 0))
                            for b, s in zip(bufs, sources)]
                    if len(devs) > 1:  # one slab per device, each D2H'd into its slice of `out`
                        _lib.array_read_multi(devs, self.zmeta, srcs, offset, shape,
                                              out_addr, flags)
                    else:
                        devs[0].array_read(self.zmeta, srcs, offset, shape, out_addr, flags)
            except _lib.ZhError as e:
                raise_for(e)
            finally:  # the call has consumed the staged bytes (it returns after its copies)
                del keep, sources
        finally:  # also when a store read or a host codec raised: the lease goes back
            staging_pool.give(lease)
        self.last_read_timing = {"prep_s": t0 - t_enter, "stage_s": t1 - t0,
                                 "device_s": time.perf_counter() - t1,
                                 "blosc_device_frames": 0, "blosc_host_frames": n_blosc,
                                 "zstd_device_frames": 0, "zstd_host_frames": n_zstd,
                                 "gzip_device_frames": 0, "gzip_host_frames": n_gzip}

    def _blosc_chain(self):
        """The chain's host byte-to-byte stages are exactly one BloscCodec (v3 or v2)."""
        bb = self.chain.inner_host_bb if self.chain.chain["sharded"] else self.chain.host_bb
        return len(bb) == 1 and isinstance(bb[0], BloscCodec)

    def _blosc_device(self, devs):
        return (len(devs) == 1 and self._blosc_chain() and
                os.environ.get("ZH_BLOSC_DEVICE", BLOSC_DEVICE_DEFAULT) != "0")

    @staticmethod
    def _blosc_decode_batch(dev):
        """DeviceContext.blosc_decode_batch with the flags of ZH_BLOSC_ZSTD_DEVICE and
        ZH_BLOSC_ZLIB_DEVICE."""
        flags = 0
        if os.environ.get("ZH_BLOSC_ZSTD_DEVICE", BLOSC_ZSTD_DEVICE_DEFAULT) != "0":
            flags |= A.ZH_BLOSC_ZSTD_DEVICE
        if os.environ.get("ZH_BLOSC_ZLIB_DEVICE", BLOSC_ZLIB_DEVICE_DEFAULT) != "0":
            flags |= A.ZH_BLOSC_ZLIB_DEVICE
        return lambda frames: dev.blosc_decode_batch(frames, flags=flags)

    def _zstd_chain(self):
        """The chain's host byte-to-byte stages are exactly one ZstdCodec."""
        bb = self.chain.inner_host_bb if self.chain.chain["sharded"] else self.chain.host_bb
        return len(bb) == 1 and isinstance(bb[0], ZstdCodec)

    def _zstd_device(self, devs, coords=()):
        """One device, a zstd chain and ZH_ZSTD_DEVICE: "0" never, "2" always, "1" when the read
        has at least ZSTD_DEVICE_MIN_FRAMES frames (a shard counts its inner chunks)."""
        if len(devs) != 1 or not self._zstd_chain():
            return False
        mode = os.environ.get("ZH_ZSTD_DEVICE", ZSTD_DEVICE_DEFAULT)
        if mode == "0":
            return False
        if mode == "2":
            return True
        if ZSTD_DEVICE_MIN_FRAMES is None:
            return False
        per = self._n_inner() if self.chain.chain["sharded"] else 1
        return len(coords) * per >= ZSTD_DEVICE_MIN_FRAMES

    def _gzip_device(self, devs, coords=()):
        """One device, a gzip chain and ZH_GZIP_DEVICE: "0" never, "2" always, "1" when the read
        has at least GZIP_DEVICE_MIN_FRAMES members (a shard counts its inner chunks)."""
        if len(devs) != 1 or not self._gzip_chain():
            return False
        mode = os.environ.get("ZH_GZIP_DEVICE", GZIP_DEVICE_DEFAULT)
        if mode == "0":
            return False
        if mode == "2":
            return True
        if GZIP_DEVICE_MIN_FRAMES is None:
            return False
        per = self._n_inner() if self.chain.chain["sharded"] else 1
        return len(coords) * per >= GZIP_DEVICE_MIN_FRAMES

    def _read_frames_device(self, coords, offset, shape, out_addr, flags, dev, parallel, t_enter,
                            t0, decode_batch, raise_frame, codec):
        """_read_into for a chain whose only host stage is blosc, zstd or gzip, on one device: the
        store reads of every chunk (a shard: its index check and per-entry range reads), one
        batched decode (`decode_batch`: DeviceContext.blosc_decode_batch / zstd_decode_batch /
        gzip_decode_batch) over
        all frames of the read, then the device read over sources in the batch buffer.
        `raise_frame` raises a frame's _lib.ZhError as the codec's host decode does; `codec`
        names the counters of last_read_timing."""
        sharded = self.chain.chain["sharded"]
        cs = self.metadata.chunk_shape

        def load(c):
            try:
                h = self._handle(c)
                if not sharded:
                    b = h.read()
                    if b is not None:
                        self._count_staged(len(b))
                    return b
                lo = [max(o, ci * k) - ci * k for o, ci, k in zip(offset, c, cs)]
                hi = [min(o + s, (ci + 1) * k) - ci * k
                      for o, s, ci, k in zip(offset, shape, c, cs)]
                full = all(a == 0 and b == k for a, b, k in zip(lo, hi, cs))
                return self._stage_shard(h, lo, hi, None, full, collect=True)
            except Exception as e:  # reported in chunk order, after earlier chunks' frames
                return _Deferred(e)
        if parallel and len(coords) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(8, len(coords))) as ex:
                sources = list(ex.map(load, coords))
        else:
            sources = [load(c) for c in coords]
        t1 = time.perf_counter()
        bad = next((k for k, s in enumerate(sources) if isinstance(s, _Deferred)), None)
        frames = []
        for s in sources[:bad]:
            if s is None:
                continue
            frames.extend([p[2] for p in s[0].pieces] if sharded else [s])
        views = [np.frombuffer(f if len(f) else b"\0", np.uint8) for f in frames]
        ptr = iptr = None
        try:
            try:
                ptr, rows = decode_batch(
                    [(int(v.ctypes.data), len(f)) for v, f in zip(views, frames)])
            except _lib.ZhError as e:
                raise_frame(e)
            if bad is not None:
                raise sources[bad].exc
            it = iter(rows)
            try:
                if sharded:
                    # the stored indexes, uploaded side by side
                    idx = [None if s is None else s[1][0][:s[0].index_nbytes] for s in sources]
                    ioff, pos = [], 0
                    for a in idx:
                        ioff.append(pos)
                        pos += 0 if a is None else -(-len(a) // 256) * 256
                    ibuf = np.zeros(max(1, pos), np.uint8)
                    for a, o in zip(idx, ioff):
                        if a is not None:
                            ibuf[o:o + len(a)] = a
                    iptr = dev.malloc(ibuf.nbytes, A.ZH_MALLOC_PLAIN)
                    dev.memcpy(iptr, ibuf.ctypes.data, ibuf.nbytes, 0)
                    shards = []
                    for s, o in zip(sources, ioff):
                        if s is None:
                            shards.append(None)
                            continue
                        ps = []
                        for po, pn, _, _ in s[0].pieces:
                            doff, dn, _ = next(it)
                            ps.append((po, pn, ptr + doff, dn))
                        shards.append(_lib.ShardSource(iptr + o, s[0].index_nbytes,
                                                       s[0].shard_nbytes, ps))
                    dev.array_read_pieces(self.zmeta, shards, offset, shape, out_addr,
                                          flags | A.ZH_SRC_DEVICE)
                else:
                    srcs = []
                    for s in sources:
                        if s is None:
                            srcs.append((None, 0))
                        else:
                            doff, dn, _ = next(it)
                            srcs.append((ptr + doff, dn))
                    dev.array_read(self.zmeta, srcs, offset, shape, out_addr,
                                   flags | A.ZH_SRC_DEVICE)
            except _lib.ZhError as e:
                raise_for(e)
        finally:
            dev.free(ptr)
            dev.free(iptr)
            del views, sources
        self.last_read_timing = {
            "prep_s": t0 - t_enter, "stage_s": t1 - t0, "device_s": time.perf_counter() - t1,
            "blosc_device_frames": 0, "blosc_host_frames": 0,
            "zstd_device_frames": 0, "zstd_host_frames": 0,
            "gzip_device_frames": 0, "gzip_host_frames": 0,
            codec + "_device_frames": sum(1 for r in rows if r[2] != 1),
            codec + "_host_frames": sum(1 for r in rows if r[2] == 1)}

    def readChunk(self, coords):
        """core.Array.readChunk (M/core/Array.java:167-182)."""
        cs = self.metadata.chunk_shape
        for d, c in enumerate(coords):
            if c < 0 or c * cs[d] >= self.metadata.shape[d]:
                raise ZarrException("Attempting to read data outside of the array's domain.")
        out = np.empty(cs, dtype=self.metadata.data_type.numpy)
        paths = self._file_paths([tuple(coords)], [device()])
        if paths is not None:  # the chunk file, read by the library (one-chunk view)
            m = A.zh_array_meta.from_buffer_copy(self.zmeta)
            for d in range(self.ndim):
                m.shape[d] = cs[d]
            try:
                device().array_read_files(m, paths, [0] * self.ndim, cs, out.ctypes.data, 0,
                                          store=self._file_store())
            except _lib.ZhError as e:
                raise_for(e)
            return out
        src = self._load_source(tuple(coords))
        if src is None:
            out.view(np.uint8).reshape(-1)[:] = np.frombuffer(
                self.metadata.fill_bytes * int(np.prod(cs)), np.uint8)
            return out
        # one chunk viewed as a one-chunk array: ShardingIndexedCodec.decode / bytes decode
        m = A.zh_array_meta.from_buffer_copy(self.zmeta)
        for d in range(self.ndim):
            m.shape[d] = cs[d]
        try:
            if src[0] == "pieces":
                device().array_read_pieces(m, [src[1]], [0] * self.ndim, cs, out.ctypes.data,
                                           0)
            else:
                b = _host_buf(src[1])
                device().array_read(m, [(C.addressof(b), len(src[1]))], [0] * self.ndim, cs,
                                    out.ctypes.data, 0)
        except _lib.ZhError as e:
            raise_for(e)
        return out

    # ---------------------------------------------------------------- write
    def write(self, offset, data, parallel=True):
        """core.Array.write(offset, array, parallel) (M/core/Array.java:83-156): whole-chunk
        regions are encoded on the device in one call; partial chunks are read-modify-written
        (decode → patch → encode).  `parallel` is the reference's switch between a serial and a
        parallel chunk stream; the device encodes every chunk of a call in one launch either
        way, so it only reaches the read of a read-modify-write."""
        data = np.ascontiguousarray(data, dtype=self.metadata.data_type.numpy)
        n = self.ndim
        offset = [0] * n if offset is None else [int(o) for o in offset]
        shape = list(data.shape)
        self._check_region(offset, shape)
        cs, ash = self.metadata.chunk_shape, self.metadata.shape
        lo = [(o // c) * c for o, c in zip(offset, cs)]
        hi = [min(-(-(o + s) // c) * c, a) for o, s, c, a in zip(offset, shape, cs, ash)]
        if lo != offset or hi != [o + s for o, s in zip(offset, shape)]:
            ext = [h - l for l, h in zip(lo, hi)]
            region = self.read(lo, ext, parallel)
            sl = tuple(slice(o - l, o - l + s) for o, l, s in zip(offset, lo, shape))
            region[sl] = data
            data, offset, shape = region, lo, ext
        coords = self._chunk_coords(offset, shape)
        dev = device()
        keep_fill = getattr(self.metadata, "fill_value", 0) is None and \
            not self.chain.chain["sharded"]
        paths = None if keep_fill else self._file_paths(coords, [dev])
        if paths is not None:  # the library writes (and deletes) the chunk files itself
            try:
                sizes = dev.array_write_files(self.zmeta, data.ctypes.data, offset, shape, paths,
                                              store=self._file_store())
            except _lib.ZhError as e:
                raise_for(e)
            self.last_write_info = {"blosc_device_frames": 0, "blosc_host_frames": 0,
                                    "zstd_device_frames": 0, "zstd_host_frames": 0,
                                    "gzip_device_frames": 0, "gzip_host_frames": 0,
                                    "raw_bytes": sum(sizes), "stored_bytes": sum(sizes)}
            return
        L = _lib.lib()
        cap = L.zh_array_encoded_bound(C.byref(self.zmeta))
        src = dev.malloc(max(1, data.nbytes))
        bufs = []
        info = {"blosc_device_frames": 0, "blosc_host_frames": 0, "zstd_device_frames": 0,
                "zstd_host_frames": 0, "gzip_device_frames": 0, "gzip_host_frames": 0,
                "raw_bytes": 0, "stored_bytes": 0}
        try:
            dev.memcpy(src, data.ctypes.data, data.nbytes, 0)
            bufs = [dev.malloc(cap) for _ in coords]
            try:
                sizes = dev.array_write(self.zmeta, src, offset, shape, [(b, cap) for b in bufs])
            except _lib.ZhError as e:
                raise_for(e)
            kind = self._encode_device()
            if kind and keep_fill:
                # no fill value: an all-zero chunk is stored, never deleted — its frame is made
                # in the same batch as the others, not on the host
                nb = int(np.prod(cs)) * self.metadata.data_type.getByteCount()
                for k, sz in enumerate(sizes):
                    if sz == 0:
                        dev.memset(bufs[k], 0, nb)
                        sizes[k] = nb
                dev.sync()
            stored = self._frames_device(dev, bufs, sizes, info, kind) if kind else {}
            for k, (c, b, sz) in enumerate(zip(coords, bufs, sizes)):
                h = self._handle(c)
                if sz == 0 and not keep_fill:
                    h.delete()  # all fill → writeChunk deletes the key (Array.java:150-151)
                    continue
                if k in stored:  # its frames were made on the device
                    info["stored_bytes"] += len(stored[k])
                    h.set(stored[k])
                    continue
                if sz == 0:
                    # no fill value (v2 "fill_value": null): writeChunk never deletes
                    # (Array.java:150 tests parsedFillValue != null) — store the zero chunk
                    enc = bytes(int(np.prod(cs)) * self.metadata.data_type.getByteCount())
                    if self.chain.chain.get("inner_crc32c"):
                        enc += struct.pack("<I", L.zh_crc32c(0, enc, len(enc)))
                else:
                    enc = dev.d2h(b, sz)
                if self.chain.host_bb:
                    info["raw_bytes"] += len(enc)
                    enc = self._bb_encode(self.chain.host_bb, enc, info)
                elif self.chain.inner_host_bb:
                    enc = self._wrap_inner(enc, info)
                else:
                    info["raw_bytes"] += len(enc)
                info["stored_bytes"] += len(enc)
                h.set(enc)
        finally:
            for b in bufs:
                dev.free(b)
            dev.free(src)
        self.last_write_info = info

    def _bb_encode(self, bb, enc, info=None):
        """host_bb_encode; a blosc chain's codec gets the dtype's byte count for an unset
        typesize, as the device route passes it down."""
        if self._blosc_chain():
            if info is not None:
                info["blosc_host_frames"] += 1
            return bb[0].encode(enc, self.metadata.data_type.getByteCount())
        if info is not None and self._zstd_chain():
            info["zstd_host_frames"] += 1
        if info is not None and self._gzip_chain():
            info["gzip_host_frames"] += 1
        return host_bb_encode(bb, enc)

    def _zstd_chain(self):
        """The chain's host byte-to-byte stages are exactly one ZstdCodec."""
        bb = self.chain.inner_host_bb if self.chain.chain["sharded"] else self.chain.host_bb
        return len(bb) == 1 and isinstance(bb[0], ZstdCodec)

    def _gzip_chain(self):
        """The chain's host byte-to-byte stages are exactly one GzipCodec."""
        bb = self.chain.inner_host_bb if self.chain.chain["sharded"] else self.chain.host_bb
        return len(bb) == 1 and isinstance(bb[0], GzipCodec)

    def _encode_device(self):
        """"blosc" / "zstd" / "gzip" when Array.write makes the chain's frames on the device
        (zh_blosc_encode_batch / zh_zstd_encode_batch / zh_gzip_encode_batch), else None: the
        codec is the only host byte-to-byte stage, one device is in use and the codec's switch
        (ZH_BLOSC_ENCODE_DEVICE / ZH_ZSTD_ENCODE_DEVICE) is not "0", or, for gzip, whose host
        route is zlib and stores other bytes, ZH_GZIP_ENCODE_DEVICE is "1" or "2" ("2": with
        dynamic-Huffman segments, _gzip_dynamic).  Blosc: its cname is
        lz4 / lz4hc, zstd with ZH_BLOSC_ZSTD_ENCODE=1 or zlib with ZH_BLOSC_ZLIB_ENCODE=1 or 2 (the
        blosc compressors written here; clevel is not honoured, as the level of zstd and gzip is
        not)."""
        if len(devices()) != 1:
            return None
        bb = self.chain.inner_host_bb if self.chain.chain["sharded"] else self.chain.host_bb
        if self._blosc_chain():
            on = os.environ.get("ZH_BLOSC_ENCODE_DEVICE", BLOSC_ENCODE_DEVICE_DEFAULT) != "0"
            return "blosc" if on and bb[0].compressed() else None
        if self._zstd_chain():
            on = os.environ.get("ZH_ZSTD_ENCODE_DEVICE", ZSTD_ENCODE_DEVICE_DEFAULT) != "0"
            return "zstd" if on else None
        if self._gzip_chain():
            on = os.environ.get("ZH_GZIP_ENCODE_DEVICE", GZIP_ENCODE_DEVICE_DEFAULT) in ("1", "2")
            return "gzip" if on else None
        return None

    @staticmethod
    def _gzip_dynamic():
        """The device's gzip members may hold dynamic-Huffman segments."""
        return os.environ.get("ZH_GZIP_ENCODE_DEVICE", GZIP_ENCODE_DEVICE_DEFAULT) == "2"

    def _frames_device(self, dev, bufs, sizes, info, kind):
        """The stored objects of the chunks with sz > 0, their frames (`kind`: blosc, zstd, gzip)
        compressed on the device in one batch over the chunk buffers: {chunk number: bytes}.
        Unsharded: the chunk is one frame.  Sharded: only the stored index comes back as it is;
        every present entry is one frame, and the shard is put together as _wrap_inner does."""
        ch = self.chain.chain
        sharded = ch["sharded"]
        codec = (self.chain.inner_host_bb if sharded else self.chain.host_bb)[0]
        if kind == "blosc":
            ts, shuffle, blocksize = codec.enc_params(self.metadata.data_type.getByteCount())
            flags = codec.enc_flags()

            def batch(sources, take):
                out, rows = dev.blosc_encode_batch_raw(sources, ts, shuffle, blocksize,
                                                       take=take, flags=flags)
                mv = memoryview(out)
                return [bytes(mv[o:o + n]) for o, n in rows]
        elif kind == "zstd":
            def batch(sources, take):
                return dev.zstd_encode_batch(sources, bool(codec.checksum), take=take)
        else:
            dynamic = self._gzip_dynamic()

            def batch(sources, take):
                return dev.gzip_encode_batch(sources, take=take, dynamic=dynamic)
        sources, shards = [], {}
        if sharded:
            n_in = self._n_inner()
            isz = _lib.lib().zh_shard_index_size(C.byref(self.zmeta))
            start = ch["index_location"] == A.ZH_INDEX_START
            fmt = ">QQ" if ch["index_endian"] == A.ZH_ENDIAN_BIG else "<QQ"
        for k, (b, sz) in enumerate(zip(bufs, sizes)):
            if sz == 0:
                continue
            if not sharded:
                sources.append((b, sz))
                continue
            idx = dev.d2h(b + (0 if start else sz - isz), isz)
            ents = [struct.unpack(fmt, idx[16 * e:16 * e + 16]) for e in range(n_in)]
            shards[k] = ents
            sources.extend((b + off, nb) for off, nb in ents if off != 2 ** 64 - 1)
        lease = []  # the frames land in a pooled buffer: no fresh pages per write
        try:
            frames = batch(sources, lambda n: staging_pool.take(n, lease))
        except _lib.ZhError as e:
            if e.status == A.ZH_EINVAL:
                raise ZarrException(f"Error in encoding {kind}: {e}") from None
            raise_for(e)
        finally:
            staging_pool.give(lease)
        info[kind + "_device_frames"] += len(frames)
        info["raw_bytes"] += sum(nb for _, nb in sources)
        if not sharded:
            return dict(zip([k for k, sz in enumerate(sizes) if sz > 0], frames))
        it, out = iter(frames), {}
        for k, ents in shards.items():
            pos = isz if start else 0
            payload, new = [], []
            for off, nb in ents:
                if off == 2 ** 64 - 1:
                    new.append((off, nb))
                    continue
                f = next(it)
                new.append((pos, len(f)))
                payload.append(f)
                pos += len(f)
            ib = b"".join(struct.pack(fmt, *e) for e in new)
            if ch["index_crc32c"]:
                ib = self.chain.index_codecs[1].encode(ib)
            pb = b"".join(payload)
            out[k] = ib + pb if start else pb + ib
        return out

    def access(self):
        return ArrayAccessor(self)


class ArrayAccessor:
    """core.Array.ArrayAccessor (M/core/Array.java:483-536)."""

    def __init__(self, array):
        self.array = array
        self.offset = None
        self.shape = None

    def withOffset(self, *offset):
        self.offset = list(offset)
        return self

    def withShape(self, *shape):
        self.shape = list(shape)
        return self

    def read(self):
        return self.array.read(self.offset, self.shape)

    def write(self, data):
        self.array.write(self.offset, data)
