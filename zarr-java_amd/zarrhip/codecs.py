"""Codec model, registry and builder mirroring zarr-java's v3 codec surface.

  Codec JSON polymorphism       M/v3/codec/Codec.java:7-9 (name + configuration)
  CodecRegistry.addType         M/v3/codec/CodecRegistry.java:11-34 (the plug-in point)
  CodecBuilder                  M/v3/codec/CodecBuilder.java:62-176
  CodecPipeline validation      M/core/codec/CodecPipeline.java:18-57

The objects are host-side descriptions; `device_chain` maps a codec list onto the
zh_codec_chain the HIP path executes (bytes/transpose/sharding/crc32c-index).  Byte-to-
byte compressors (gzip, blosc, zstd, inner crc32c) stay on the host (north star): they
are applied by `host_bb_decode` before the bytes reach the device.  Array.read can hand the
frames of a chain whose only such stage is blosc, zstd or gzip to the device in one batch instead
(ZH_BLOSC_DEVICE, ZH_ZSTD_DEVICE, ZH_GZIP_DEVICE; array.py): the codec objects here are not
involved then.
"""
import gzip as _gzip
import os
import struct
import zlib

from . import _abi as A
from .errors import UnsupportedChainError, ZarrException


class Codec:
    name = None
    kind = None  # "aa" (array→array), "ab" (array→bytes), "bb" (bytes→bytes)

    def to_json(self):
        raise NotImplementedError

    @classmethod
    def from_json(cls, cfg, registry):
        raise NotImplementedError

    def __eq__(self, other):
        return type(self) is type(other) and self.to_json() == other.to_json()

    def __repr__(self):
        return f"{type(self).__name__}({self.to_json()})"


class BytesCodec(Codec):
    """v3 BytesCodec (M/v3/codec/core/BytesCodec.java): endian None = no configuration."""
    name, kind = "bytes", "ab"

    def __init__(self, endian="little"):
        if endian is not None:
            endian = str(getattr(endian, "value", endian)).lower()
            if endian not in ("little", "big"):
                raise ZarrException(f"Invalid endian '{endian}'")
        self.endian = endian

    def byte_order(self, dtype_size):
        if dtype_size <= 1:  # core BytesCodec.decode :16-18 (Q9)
            return A.ZH_ENDIAN_BIG
        if self.endian is None:  # v3 BytesCodec.getByteOrder :43-48 (Q11)
            raise ZarrException("BytesCodec configuration is required to determine endianess.")
        return A.ZH_ENDIAN_BIG if self.endian == "big" else A.ZH_ENDIAN_LITTLE

    def to_json(self):
        if self.endian is None:
            return {"name": "bytes"}
        return {"name": "bytes", "configuration": {"endian": self.endian}}

    @classmethod
    def from_json(cls, cfg, registry):
        return cls((cfg or {}).get("endian", "little") if cfg is not None else None)


class TransposeCodec(Codec):
    """TransposeCodec (M/v3/codec/core/TransposeCodec.java:18-93)."""
    name, kind = "transpose", "aa"

    def __init__(self, order):
        self.order = [int(o) for o in order]

    def validate(self, ndim):
        o = self.order
        if not o or sorted(o) != list(range(len(o))):  # Utils.isPermutation :91-100
            raise ZarrException("Order is no permutation array")
        if len(o) != ndim:
            raise ZarrException("Array has not the same ndim as transpose codec order")

    def to_json(self):
        return {"name": "transpose", "configuration": {"order": list(self.order)}}

    @classmethod
    def from_json(cls, cfg, registry):
        return cls(cfg["order"])


class ReshapeCodec(Codec):
    """ReshapeCodec (M/v3/codec/core/ReshapeCodec.java): a ravel-preserving array→array
    reshape.  Each `shape` entry is a positive size, a list of input dims (their product), or
    -1 (once).  Validation and messages follow resolveOutputShape (:148-168) and its steps."""
    name, kind = "reshape", "aa"

    def __init__(self, shape):
        self.shape = [list(s) if isinstance(s, (list, tuple)) else s for s in shape]

    def to_json(self):
        return {"name": "reshape", "configuration": {"shape": [
            list(s) if isinstance(s, list) else s for s in self.shape]}}

    @classmethod
    def from_json(cls, cfg, registry):
        return cls(cfg["shape"])

    def resolve(self, input_shape):
        """→ (output shape, input dims per output entry or None)."""
        ndim, n = len(input_shape), len(self.shape)
        if n == 0:
            raise ZarrException("reshape codec: 'shape' must not be empty.")
        out, dims_per, minus, flat = [0] * n, [None] * n, -1, []
        for i, e in enumerate(self.shape):  # parseConfiguredShape :187-235
            if isinstance(e, list):
                prod = 1
                for d in e:
                    if not isinstance(d, int):
                        raise ZarrException("reshape codec: 'shape' entries must be integers or "
                                            f"arrays of integers, but got {d}.")
                    if d < 0 or d >= ndim:
                        raise ZarrException(f"reshape codec: input dimension {d} is out of range "
                                            f"for an input array with {ndim} dimensions.")
                    prod *= input_shape[d]
                    flat.append(d)
                dims_per[i] = list(e)
                out[i] = prod
            elif isinstance(e, int):
                if e == -1:
                    if minus != -1:
                        raise ZarrException("reshape codec: 'shape' may contain -1 at most once.")
                    minus = i
                    out[i] = -1
                elif e <= 0:
                    raise ZarrException("reshape codec: 'shape' entries must be a positive integer, "
                                        f"-1, or an array of input dimensions, but got {e}.")
                else:
                    out[i] = e
            else:
                raise ZarrException("reshape codec: 'shape' entries must be integers or arrays of "
                                    f"integers, but got {e}.")
        for j in range(1, len(flat)):  # checkNoReordering :241-249
            if flat[j] <= flat[j - 1]:
                raise ZarrException("reshape codec: the flattened list of input dimensions must be "
                                    f"strictly increasing, but got [{', '.join(map(str, flat))}].")
        total = 1
        for s in input_shape:
            total *= s
        if minus != -1:  # resolveInferredDimension :254-267
            known = 1
            for i, s in enumerate(out):
                if i != minus:
                    known *= s
            if known == 0 or total % known != 0:
                raise ZarrException("reshape codec: cannot infer the -1 dimension because "
                                    "prod(output shape) would not equal prod(input shape) "
                                    f"({total}).")
            out[minus] = total // known
        prod_out = 1
        for s in out:
            prod_out *= s
        if prod_out != total:  # checkElementCountPreserved :272-283
            raise ZarrException(f"reshape codec: prod(output shape)={prod_out} does not equal "
                                f"prod(input shape)={total}.")
        for i, dims in enumerate(dims_per):  # checkMergesAligned :291-322
            if not dims:
                continue
            op = 1
            for j in range(i):
                op *= out[j]
            os_ = 1
            for j in range(i + 1, n):
                os_ *= out[j]
            ip = 1
            for d in range(dims[0]):
                ip *= input_shape[d]
            is_ = 1
            for d in range(dims[-1] + 1, ndim):
                is_ *= input_shape[d]
            if op != ip or os_ != is_:
                raise ZarrException(
                    f"reshape codec: output dimension {i} specified by input dimensions "
                    f"[{', '.join(map(str, dims))}] does not align with the raveled input array "
                    f"(prefix {op} vs {ip}, suffix {os_} vs {is_}).")
        for i, s in enumerate(out):  # toIntShape :328-337
            if s > 2 ** 31 - 1:
                raise ZarrException(f"reshape codec: output dimension {i} exceeds "
                                    "Integer.MAX_VALUE.")
        return out, dims_per

    def resolve_array_metadata(self, shape, chunk_shape):
        """resolveArrayMetadata (:99-142): the output chunk shape and the output grid shape
        (a merged output dim multiplies the input chunk counts; a split input dim keeps its
        count on the outermost output dim)."""
        out, _ = self.resolve(chunk_shape)
        mult = [1] * len(out)
        ostart = [1]
        for s in out:
            ostart.append(ostart[-1] * s)
        istart = 1
        for d, c in enumerate(chunk_shape):
            nchunks = shape[d] // c
            target = len(out) - 1
            for i in range(len(out)):
                if ostart[i] <= istart < ostart[i + 1]:
                    target = i
                    break
            mult[target] *= nchunks
            istart *= c
        return [m * s for m, s in zip(mult, out)], out


class Crc32cCodec(Codec):
    """Crc32cCodec (M/v3/codec/core/Crc32cCodec.java:24-60)."""
    name, kind = "crc32c", "bb"

    def decode(self, b):
        from ._lib import lib
        body, stored = b[:-4], struct.unpack("<i", b[-4:])[0]
        computed = struct.unpack("<i", struct.pack("<I", lib().zh_crc32c(0, body, len(body))))[0]
        if computed != stored:
            raise ZarrException("The checksum of the sharding index is invalid. Stored: %d "
                                "Computed: %d" % (stored, computed))
        return body

    def encode(self, b):
        from ._lib import lib
        return bytes(b) + struct.pack("<I", lib().zh_crc32c(0, bytes(b), len(b)))

    def to_json(self):
        return {"name": "crc32c"}

    @classmethod
    def from_json(cls, cfg, registry):
        return cls()


class GzipCodec(Codec):
    """GzipCodec (M/v3/codec/core/GzipCodec.java:35-46) — host only: zlib both ways.
    Array.write makes a gzip chain's members on the device instead when ZH_GZIP_ENCODE_DEVICE
    is 1 (zh_gzip_encode_batch: stored and fixed-Huffman segments, other bytes than zlib's,
    `level` not honoured) or 2 (the same with dynamic-Huffman segments where they are smaller);
    decode reads all of them.  Array.read decodes a gzip chain's members on the device instead
    when ZH_GZIP_DEVICE says so (zh_gzip_decode_batch, the library's own DEFLATE reader; a corrupt member is then
    ZarrException("Error in decoding gzip."), the reference's).  decode() here stays zlib and a
    corrupt member raises the bare zlib.error: moving it to zh_gzip_decompress is a follow-up."""
    name, kind = "gzip", "bb"

    def __init__(self, level=5):
        if not 0 <= int(level) <= 9:
            raise ZarrException("'level' needs to be between 0 and 9.")
        self.level = int(level)

    def decode(self, b):
        return zlib.decompress(bytes(b), 31)

    def encode(self, b):
        return _gzip.compress(bytes(b), compresslevel=self.level, mtime=0)

    def to_json(self):
        return {"name": "gzip", "configuration": {"level": self.level}}

    @classmethod
    def from_json(cls, cfg, registry):
        return cls((cfg or {}).get("level", 5))


class BloscCodec(Codec):
    """BloscCodec (M/v3/codec/core/BloscCodec.java) — host only.  Frames are decoded by
    zh_blosc_decompress (BloscLZ / LZ4 / zlib / zstd payloads, byte and bit shuffle; snappy
    raises UnsupportedChainError).  Array.read hands the frames of a chain whose only host stage
    is this codec to the device in one batch instead (ZH_BLOSC_DEVICE: LZ4 / BloscLZ / raw
    streams; with ZH_BLOSC_ZSTD_DEVICE=1 also frames whose streams are plain zstd frames, the
    default cname's; with ZH_BLOSC_ZLIB_DEVICE=1 also frames whose streams are zlib streams as
    compress2 writes them; without its switch a compressor's payloads stay with
    zh_blosc_decompress).  encode compresses cname lz4 / lz4hc with the library's own
    LZ4 writer (zh_blosc_compress: byte-identical to the frames Array.write makes on the
    device; clevel is not honoured, and blocks are at most 64 KiB).  With ZH_BLOSC_ZSTD_ENCODE=1
    cname zstd is compressed as well (zh_blosc_compress_ex with ZH_BLOSC_ENC_ZSTD: the LZ4
    writer's layout with compressor code 4, every stream one zstd frame as zh_zstd_compress
    writes it, or raw); the switch is off by default, since it changes stored bytes.  With
    ZH_BLOSC_ZLIB_ENCODE=1 cname zlib is compressed too (ZH_BLOSC_ENC_ZLIB: compressor code 3,
    every stream one zlib stream of stored and fixed segments over 16 KiB pieces, or raw), and
    with "2" its segments may be dynamic (ZH_BLOSC_ENC_DYNAMIC); off by default for the same
    reason.  Every other cname, and zstd or zlib with its switch unset, is written as a
    MEMCPYED frame (no compressor for it here)."""
    name, kind = "blosc", "bb"
    SHUFFLE_CODE = {"noshuffle": 0, "shuffle": 1, "bitshuffle": 2}
    ZSTD_ENCODE_DEFAULT = "0"
    ZLIB_ENCODE_DEFAULT = "0"

    def __init__(self, cname="zstd", clevel=5, shuffle="noshuffle", typesize=None, blocksize=0):
        self.cfg = {"typesize": typesize, "cname": cname, "clevel": clevel, "shuffle": shuffle,
                    "blocksize": blocksize}

    def decode(self, b):
        import ctypes as C
        from . import _abi as A
        from ._lib import lib
        b = bytes(b)
        L = lib()
        n = C.c_size_t()
        err = C.create_string_buffer(256)
        st = L.zh_blosc_decompress(b, len(b), None, 0, C.byref(n), err, 256)
        if st == A.ZH_OK:
            out = (C.c_char * max(1, n.value))()
            st = L.zh_blosc_decompress(b, len(b), out, n.value, C.byref(n), err, 256)
        if st == A.ZH_EUNSUPPORTED:
            raise UnsupportedChainError(err.value.decode())
        if st != A.ZH_OK:
            raise ZarrException(f"Error in decoding blosc: {err.value.decode()}")
        return bytes(out)[:n.value]

    def lz4(self):
        return self.cfg.get("cname") in ("lz4", "lz4hc")

    def zstd_enc(self):
        """cname zstd with ZH_BLOSC_ZSTD_ENCODE=1: encode writes zstd streams."""
        return (self.cfg.get("cname") == "zstd" and
                os.environ.get("ZH_BLOSC_ZSTD_ENCODE", self.ZSTD_ENCODE_DEFAULT) == "1")

    def zlib_enc(self):
        """cname zlib with ZH_BLOSC_ZLIB_ENCODE=1 or 2: encode writes zlib streams.  The flags
        of the writer: 0 (no), ZH_BLOSC_ENC_ZLIB, or with "2" ZH_BLOSC_ENC_ZLIB |
        ZH_BLOSC_ENC_DYNAMIC."""
        from . import _abi as A
        if self.cfg.get("cname") != "zlib":
            return 0
        mode = os.environ.get("ZH_BLOSC_ZLIB_ENCODE", self.ZLIB_ENCODE_DEFAULT)
        return {"1": A.ZH_BLOSC_ENC_ZLIB,
                "2": A.ZH_BLOSC_ENC_ZLIB | A.ZH_BLOSC_ENC_DYNAMIC}.get(mode, 0)

    def enc_flags(self):
        """The flags word zh_blosc_compress_ex / zh_blosc_encode_batch_ex take for this codec."""
        from . import _abi as A
        return A.ZH_BLOSC_ENC_ZSTD if self.zstd_enc() else self.zlib_enc()

    def compressed(self):
        """encode compresses (lz4 / lz4hc, or zstd or zlib behind its switch) and is not
        MEMCPYED."""
        return self.lz4() or self.zstd_enc() or bool(self.zlib_enc())

    def enc_params(self, default_typesize=1):
        """(typesize, shuffle code, blocksize) as zh_blosc_enc_params takes them."""
        return (self.cfg.get("typesize") or default_typesize,
                self.SHUFFLE_CODE[self.cfg.get("shuffle") or "noshuffle"],
                int(self.cfg.get("blocksize") or 0))

    def encode(self, b, default_typesize=1):
        b = bytes(b)
        if self.compressed():
            from ._lib import ZhError, blosc_compress
            try:
                return blosc_compress(b, *self.enc_params(default_typesize),
                                      flags=self.enc_flags())
            except ZhError as e:
                raise ZarrException(f"Error in encoding blosc: {e}") from None
        ts = self.cfg.get("typesize") or 1
        hdr = struct.pack("<BBBBIII", 2, 1, 0x02 | 0x01, ts, len(b), len(b), len(b) + 16)
        return hdr + b

    def to_json(self):
        return {"name": "blosc", "configuration": dict(self.cfg)}

    @classmethod
    def from_json(cls, cfg, registry):
        cfg = cfg or {}
        return cls(cfg.get("cname", "zstd"), cfg.get("clevel", 5), cfg.get("shuffle", "noshuffle"),
                   cfg.get("typesize"), cfg.get("blocksize", 0))


class ZstdCodec(Codec):
    """ZstdCodec (M/core/codec/core/ZstdCodec.java:14-22, M/v3/codec/core/ZstdCodec.java) —
    host only.  Decode: zh_zstd_decompress, a from-scratch RFC 8878 frame decoder in the
    library (zstd-jni / libzstd in the reference); the content checksum is verified when a
    frame carries one.  Encode: zh_zstd_compress, the host form of the block writer Array.write
    runs on the device (greedy LZ, raw literals, predefined FSE tables; blocks that do not
    shrink are raw blocks); `level` is not honoured, the metadata keeps it."""
    name, kind = "zstd", "bb"

    def __init__(self, level=5, checksum=True):
        self.level, self.checksum = level, checksum

    def decode(self, b):
        import ctypes as C
        from . import _abi as A
        from ._lib import lib
        b = bytes(b)
        L = lib()
        n = C.c_size_t()
        err = C.create_string_buffer(256)
        st = L.zh_zstd_decompress(b, len(b), None, 0, C.byref(n), err, 256)
        # the size query answers from the frame header without decoding a block: never size an
        # allocation beyond what the frame can expand to (an RLE block: 4 bytes → 128 KiB)
        if st == A.ZH_OK and n.value > len(b) * 32768 + (64 << 10):
            raise ZarrException(f"Error in decoding zstd: frame content size {n.value} exceeds "
                                f"what {len(b)} bytes of frame can hold")
        if st == A.ZH_OK:
            out = (C.c_char * max(1, n.value))()
            st = L.zh_zstd_decompress(b, len(b), out, n.value, C.byref(n), err, 256)
        if st == A.ZH_EUNSUPPORTED:
            raise UnsupportedChainError(err.value.decode())
        if st != A.ZH_OK:
            raise ZarrException(f"Error in decoding zstd: {err.value.decode()}")
        return bytes(out)[:n.value]

    def encode(self, b):
        from ._lib import zstd_compress
        return zstd_compress(b, bool(self.checksum))

    def to_json(self):
        return {"name": "zstd", "configuration": {"level": self.level, "checksum": self.checksum}}

    @classmethod
    def from_json(cls, cfg, registry):
        cfg = cfg or {}
        return cls(cfg.get("level", 5), cfg.get("checksum", True))


class ShardingIndexedCodec(Codec):
    """ShardingIndexedCodec.Configuration (ShardingIndexedCodec.java:267-299)."""
    name, kind = "sharding_indexed", "ab"

    def __init__(self, chunk_shape, codecs=None, index_codecs=None, index_location="end"):
        if index_location is None:
            index_location = "end"
        if index_location not in ("start", "end"):
            raise ZarrException('Only index_location "start" or "end" are supported.')
        self.chunk_shape = [int(c) for c in chunk_shape]
        self.codecs = list(codecs) if codecs is not None else [BytesCodec("little")]
        self.index_codecs = list(index_codecs) if index_codecs is not None else \
            [BytesCodec("little"), Crc32cCodec()]
        self.index_location = index_location

    def to_json(self):
        return {"name": "sharding_indexed", "configuration": {
            "chunk_shape": list(self.chunk_shape),
            "codecs": [c.to_json() for c in self.codecs],
            "index_codecs": [c.to_json() for c in self.index_codecs],
            "index_location": self.index_location}}

    @classmethod
    def from_json(cls, cfg, registry):
        return cls(cfg["chunk_shape"], [registry.codec_from_json(c) for c in cfg["codecs"]],
                   [registry.codec_from_json(c) for c in cfg["index_codecs"]],
                   cfg.get("index_location", "end"))


class CodecRegistry:
    """CodecRegistry (M/v3/codec/CodecRegistry.java:9-35): name → class.  addType replaces
    an existing entry — the hook the device codec uses in the Java integration."""
    map = {}

    @classmethod
    def addType(cls, name, codec_cls):
        cls.map[name] = codec_cls

    @classmethod
    def getNamedTypes(cls):
        return dict(cls.map)

    @classmethod
    def codec_from_json(cls, j):
        name = j.get("name")
        if name not in cls.map:
            raise ZarrException(f"Unknown codec '{name}'")
        return cls.map[name].from_json(j.get("configuration"), cls)


for _c in (TransposeCodec, ReshapeCodec, BytesCodec, BloscCodec, GzipCodec, ZstdCodec,
           Crc32cCodec, ShardingIndexedCodec):
    CodecRegistry.addType(_c.name, _c)


class CodecBuilder:
    """CodecBuilder (M/v3/codec/CodecBuilder.java)."""

    def __init__(self, data_type):
        self.data_type = data_type
        self.codecs = []

    def withTranspose(self, order):
        self.codecs.append(TransposeCodec(order))
        return self

    def withReshape(self, shape):
        self.codecs.append(ReshapeCodec(shape))
        return self

    def withBytes(self, endian="LITTLE"):
        if self.data_type.getByteCount() <= 1:  # :76-82
            self.codecs.append(BytesCodec(None))
        else:
            self.codecs.append(BytesCodec(str(getattr(endian, "value", endian)).lower()))
        return self

    def withGzip(self, level=5):
        self.codecs.append(GzipCodec(level))
        return self

    def withBlosc(self, cname="zstd", shuffle="noshuffle", clevel=5):
        self.codecs.append(BloscCodec(cname, clevel, shuffle, self.data_type.getByteCount(), 0))
        return self

    def withZstd(self, level=5, checksum=True):
        self.codecs.append(ZstdCodec(level, checksum))
        return self

    def withCrc32c(self):
        self.codecs.append(Crc32cCodec())
        return self

    def withSharding(self, chunk_shape, codec_builder=None, index_location="end"):
        """:122-153 — the short form uses inner [bytes LE] and index [bytes LE, crc32c]."""
        if codec_builder is None:
            inner = [BytesCodec("little")]
        else:
            inner = codec_builder(CodecBuilder(self.data_type)).build()
        self.codecs.append(ShardingIndexedCodec(chunk_shape, inner,
                                                [BytesCodec("little"), Crc32cCodec()],
                                                index_location))
        return self

    def build(self):
        """autoInsertBytesCodec (:160-176)."""
        if not any(c.kind == "ab" for c in self.codecs):
            aa = [c for c in self.codecs if c.kind == "aa"]
            bb = [c for c in self.codecs if c.kind == "bb"]
            self.codecs = aa + [BytesCodec("little")] + bb
        return list(self.codecs)


def validate_pipeline(codecs):
    """CodecPipeline constructor checks (M/core/codec/CodecPipeline.java:18-57)."""
    n_ab = sum(1 for c in codecs if c.kind == "ab")
    if n_ab != 1:
        raise ZarrException(f"Exactly 1 ArrayBytesCodec is required. Found {n_ab}.")
    prev = None
    for c in codecs:
        if prev is not None:
            if c.kind == "ab" and prev.kind == "bb":
                raise ZarrException(f"ArrayBytesCodec '{type(c).__name__}' cannot follow after "
                                    f"BytesBytesCodec '{type(prev).__name__}'.")
            if c.kind == "aa" and prev.kind == "ab":
                raise ZarrException(f"ArrayArrayCodec '{type(c).__name__}' cannot follow after "
                                    f"ArrayBytesCodec '{type(prev).__name__}'.")
            if c.kind == "aa" and prev.kind == "bb":
                raise ZarrException(f"ArrayArrayCodec '{type(c).__name__}' cannot follow after "
                                    f"BytesBytesCodec '{type(prev).__name__}'.")
        prev = c


class DeviceChain:
    """How a codec list runs: the zh_codec_chain for the device plus the host byte-to-byte
    stages that wrap it (applied outermost-last on decode, like CodecPipeline.decode)."""

    def __init__(self, chain, host_bb, inner_host_bb, index_codecs=None):
        self.chain = chain                   # zh_codec_chain fields (dict)
        self.host_bb = host_bb               # BB codecs around whole chunks (unsharded)
        self.inner_host_bb = inner_host_bb   # BB codecs around inner chunks (sharded)
        self.index_codecs = index_codecs


def _aa_order(aa, ndim, chunk_shape):
    """Fold the array→array codecs (transpose, reshape) into one permutation of the chunk's
    own dims: the order in which the payload's C-order traverses them (zh_codec_chain
    .transpose_order), or None for the identity.

    A reshape preserves the ravel (ReshapeCodec.java:62-88), so it never moves bytes; it only
    regroups the current dims.  A later transpose is expressible as a chunk-dim permutation
    when every current dim is a whole group of chunk dims (merges, unit dims) — splits followed
    by a transpose are not, and stay unsupported."""
    seq = list(range(ndim))                      # payload traversal order of the chunk dims
    groups = [[d] for d in range(ndim)]          # current dims as groups of chunk dims
    shape = list(chunk_shape) if chunk_shape is not None else None
    for c in aa:
        if isinstance(c, TransposeCodec):
            c.validate(len(groups) if groups is not None else len(shape))
            if list(c.order) == list(range(len(c.order))):
                continue
            if groups is None:
                raise UnsupportedChainError("transpose after a dimension-splitting reshape")
            groups = [groups[o] for o in c.order]
            if shape is not None:
                shape = [shape[o] for o in c.order]
            seq = [d for g in groups for d in g]
        elif isinstance(c, ReshapeCodec):
            if shape is None:
                raise UnsupportedChainError("reshape needs the chunk shape")
            out, _ = c.resolve(shape)
            groups = _regroup(groups, shape, out)
            shape = out
        else:
            raise UnsupportedChainError(f"array→array codec '{c.name}' is not device-supported")
    return None if seq == list(range(ndim)) else seq


def _regroup(groups, cur, out):
    """Groups of chunk dims behind each output dim of a ravel-preserving reshape cur → out,
    or None when some output dim splits a current dim (or groups is already None)."""
    if groups is None:
        return None
    res, j = [], 0
    for s in out:
        if s == 1:
            res.append([])
            continue
        g, prod = [], 1
        while j < len(cur) and prod < s:
            g += groups[j]
            prod *= cur[j]
            j += 1
        if prod != s:
            return None
        res.append(g)
    tail = []
    while j < len(cur):   # trailing unit dims: size 1, so their position is free
        if cur[j] != 1:
            return None
        tail += groups[j]
        j += 1
    if tail:
        if not res:
            res.append([])
        res[-1] = res[-1] + tail
    return res


def _split_inner(codecs, ndim, dsize, chunk_shape=None):
    validate_pipeline(codecs)
    aa = [c for c in codecs if c.kind == "aa"]
    ab = [c for c in codecs if c.kind == "ab"][0]
    bb = [c for c in codecs if c.kind == "bb"]
    if not isinstance(ab, BytesCodec):
        raise UnsupportedChainError("only bytes (or one nested sharding level) is device-supported")
    order = _aa_order(aa, ndim, chunk_shape)
    return order, ab.byte_order(dsize), bb


def _take_crc(bb):
    """A trailing-only [crc32c] byte-to-byte chain runs on the device (zh_codec_chain
    .inner_crc32c); anything else stays a host byte-to-byte stage."""
    if len(bb) == 1 and isinstance(bb[0], Crc32cCodec):
        return [], True
    return bb, False


def _index_chain(sh):
    ic = sh.index_codecs
    if not ic or not isinstance(ic[0], BytesCodec) or \
            any(not isinstance(c, Crc32cCodec) for c in ic[1:]) or len(ic) > 2:
        raise UnsupportedChainError("index codecs must be [bytes, crc32c?]")
    return ic


def device_chain(codecs, ndim, dsize, chunk_shape=None):
    """Map a v3 codec list onto the device path (raises UnsupportedChainError otherwise).
    `chunk_shape` (the array's chunk shape) is needed to resolve reshape codecs."""
    validate_pipeline(codecs)
    ab = [c for c in codecs if c.kind == "ab"][0]
    if isinstance(ab, ShardingIndexedCodec):
        if len(codecs) != 1:
            # array-level codecs next to sharding disable partial decode
            # (CodecPipeline.supportsPartialDecode :82-84)
            raise UnsupportedChainError("sharding_indexed must be the only array-level codec")
        ic = _index_chain(ab)
        nested = None
        validate_pipeline(ab.codecs)
        inner_ab = [c for c in ab.codecs if c.kind == "ab"][0]
        if isinstance(inner_ab, ShardingIndexedCodec):
            # nested sharding (ZarrPythonTests.java:177-179): the inner pipeline is exactly
            # [sharding_indexed{...}] whose own inner pipeline is [transpose?, bytes]
            if len(ab.codecs) != 1:
                raise UnsupportedChainError("nested sharding must be the only inner codec")
            nested = inner_ab
            order, endian, inner_bb = _split_inner(nested.codecs, ndim, dsize, nested.chunk_shape)
            inner_bb, crc = _take_crc(inner_bb)
            if inner_bb:
                raise UnsupportedChainError("nested sharding with byte-to-byte leaf codecs")
        else:
            order, endian, inner_bb = _split_inner(ab.codecs, ndim, dsize, ab.chunk_shape)
            inner_bb, crc = _take_crc(inner_bb)
        chain = dict(sharded=True, inner_chunk_shape=ab.chunk_shape, transpose_order=order,
                     endian=endian, inner_crc32c=crc, index_endian=ic[0].byte_order(8),
                     index_crc32c=len(ic) == 2,
                     index_location=A.ZH_INDEX_START if ab.index_location == "start"
                     else A.ZH_INDEX_END)
        if nested is not None:
            nic = _index_chain(nested)
            chain.update(nested_chunk_shape=nested.chunk_shape,
                         nested_index_endian=nic[0].byte_order(8),
                         nested_index_crc32c=len(nic) == 2,
                         nested_index_location=A.ZH_INDEX_START
                         if nested.index_location == "start" else A.ZH_INDEX_END)
        return DeviceChain(chain, [], inner_bb, ic)
    order, endian, bb = _split_inner(codecs, ndim, dsize, chunk_shape)
    bb, crc = _take_crc(bb)
    chain = dict(sharded=False, transpose_order=order, endian=endian, inner_crc32c=crc)
    return DeviceChain(chain, bb, [])


def host_bb_decode(bb_codecs, b):
    for c in reversed(bb_codecs):
        b = c.decode(b)
    return b


def host_bb_encode(bb_codecs, b):
    for c in bb_codecs:
        b = c.encode(b)
    return b
