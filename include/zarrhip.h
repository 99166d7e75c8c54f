/*
 * zarrhip.h — C-ABI of the MI355X-native Zarr v3 chunk codec path.
 *
 * This is the drop-in boundary that zarr-java's JNI shim binds.
 * Every entry point is `extern "C"`, takes plain pointers and sizes, and returns an
 * `int` status (ZH_OK = 0).  No torch / HIP types appear in any signature: streams
 * and device buffers travel as `void*`.
 *
 * Reference interfaces replaced (zarr-java snapshot 2026-08-07,
 * M/ = src/main/java/dev/zarr/zarrjava/):
 *   zh_array_read               core.Array.read(long[],long[],boolean)       M/core/Array.java:378-441
 *   zh_plan_* (prepared read)   same, split into plan (host) + execute (device)
 *   zh_sharding_decode          ShardingIndexedCodec.decode(ByteBuffer)      M/v3/codec/core/ShardingIndexedCodec.java:98-103
 *   zh_sharding_decode_partial  ShardingIndexedCodec.decodePartial(...)      M/v3/codec/core/ShardingIndexedCodec.java:245-255
 *   zh_shard_ranges             StoreHandleDataProvider reads of decodeInternal ShardingIndexedCodec.java:190-230, 333-357
 *   zh_array_read_pieces        core.Array.read with sub-shard parts         M/core/Array.java:378-441 + the above
 *   zh_sharding_decode_pieces   ShardingIndexedCodec.decodePartial(StoreHandle, ...) ShardingIndexedCodec.java:245-255
 *   zh_shard_index_check        Crc32cCodec.decode of a shard index (host)    M/v3/codec/core/Crc32cCodec.java:24-48
 *   zh_array_read_files(_multi) core.Array.read over a FilesystemStore        M/core/Array.java:378-441 +
 *                               (exists / get(keys,start,end) per chunk)     M/store/FilesystemStore.java:43-102
 *   zh_array_write(_files)      core.Array.write + writeChunk + ShardingIndexedCodec.encode
 *                                                                            M/core/Array.java:83-156, ShardingIndexedCodec.java:105-168
 *   zh_shard_index_size         ShardingIndexedCodec.getShardIndexSize       ShardingIndexedCodec.java:176-181
 *   zh_crc32c                   utils.CRC32C.update/getValue                 M/utils/CRC32C.java:119-125,137-139
 *   zh_compute_chunk_coords     IndexingUtils.computeChunkCoords             M/utils/IndexingUtils.java:16-51
 *   zh_compute_projection       IndexingUtils.computeProjection (5-arg)      M/utils/IndexingUtils.java:65-117
 *   zh_is_permutation           Utils.isPermutation                          M/utils/Utils.java:91-100
 *   zh_inverse_permutation      Utils.inversePermutation                     M/utils/Utils.java:102-109
 *
 * Status → Java exception mapping used by the JNI shim:
 *   ZH_EINVAL  → IllegalArgumentException      (rank mismatches, Array.java:380-385)
 *   ZH_EDATA   → dev.zarr.zarrjava.ZarrException (message text reproduces the reference's)
 *   ZH_EUNSUPPORTED → caller falls back to the Java codec (chain not device-supported)
 *   ZH_EARITH  → ArithmeticException            (IndexingUtils overflow checks)
 *   ZH_EIO     → dev.zarr.zarrjava.store.StoreException (a RuntimeException; zh_array_read_files)
 *   ZH_EHIP / ZH_ENOMEM → RuntimeException
 */
#ifndef ZARRHIP_H
#define ZARRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZH_MAX_DIMS 8

enum zh_status {
  ZH_OK = 0,
  ZH_EINVAL = 1,
  ZH_EDATA = 2,
  ZH_EUNSUPPORTED = 3,
  ZH_EHIP = 4,
  ZH_ENOMEM = 5,
  ZH_EARITH = 6,
  ZH_EIO = 7 /* a store file could not be read (StoreException.readFailed) */
};

enum zh_endian { ZH_ENDIAN_LITTLE = 0, ZH_ENDIAN_BIG = 1 };
enum zh_index_location { ZH_INDEX_END = 0, ZH_INDEX_START = 1 };

/* call flags */
#define ZH_SRC_DEVICE 0x1u /* chunk/shard byte sources are device pointers            */
#define ZH_OUT_DEVICE 0x2u /* output buffer is a device pointer                      */

/*
 * Codec chain the device path executes.  Mirrors the JSON `codecs` list of a v3 array
 * (v3/ArrayMetadata.java) restricted to the device-supported chains:
 *   sharded = 0 :  [transpose?, bytes]                          (BASELINE config 2)
 *   sharded = 1 :  [sharding_indexed{ codecs=[transpose?, bytes, crc32c?],
 *                                     index_codecs=[bytes, crc32c?],
 *                                     index_location }]          (configs 3, 4, 5)
 *   plus one nested sharding_indexed level as the sole inner codec (nested* fields) and a
 *   trailing chunk crc32c (inner_crc32c).  Anything else (blosc/gzip/zstd inside the chain,
 *   array-level codecs next to sharding) is rejected with ZH_EUNSUPPORTED so the caller
 *   keeps the Java path (host byte-to-byte stages: INTEGRATION.md §3).
 */
typedef struct zh_codec_chain {
  int32_t sharded;                          /* 1: outer codec is sharding_indexed              */
  int32_t inner_chunk_shape[ZH_MAX_DIMS];   /* sharding configuration.chunk_shape              */
  int32_t has_transpose;                    /* transpose codec present in the (inner) chain    */
  int32_t transpose_order[ZH_MAX_DIMS];     /* TransposeCodec.Configuration.order              */
  int32_t endian;                           /* bytes codec endian (ignored for 1-byte types)   */
  int32_t index_endian;                     /* index_codecs bytes endian                       */
  int32_t index_has_crc32c;                 /* index_codecs contains crc32c                    */
  int32_t index_location;                   /* ZH_INDEX_END (default) / ZH_INDEX_START          */
  /* Nested sharding (ZarrPythonTests.java:177-179, ZarrV3Test.java:197-200): the sharding
   * codec's inner codecs are [sharding_indexed{nested_chunk_shape, codecs [transpose?,
   * bytes], index_codecs [bytes(nested_index_endian), crc32c?], nested_index_location}].
   * Each inner chunk is then itself a shard; transpose/endian above apply to its leaves. */
  int32_t nested;
  int32_t nested_chunk_shape[ZH_MAX_DIMS];
  int32_t nested_index_endian;
  int32_t nested_index_has_crc32c;
  int32_t nested_index_location;
  /* The chunk codecs end with crc32c ([transpose?, bytes, crc32c]; ZarrPythonTests "crc32c",
   * ZarrPythonTests.java:180-182): each stored (inner/leaf) chunk is its payload followed by
   * the payload's CRC-32C, little-endian (Crc32cCodec.java:24-60), verified on the device. */
  int32_t inner_crc32c;
} zh_codec_chain;

/* CoreArrayMetadata (M/core/ArrayMetadata.java:154-187) + the codec chain. */
typedef struct zh_array_meta {
  int32_t ndim;
  int32_t dtype_size;                 /* DataType.getByteCount(): 1, 2, 4 or 8             */
  int32_t dtype_is_bool;              /* bool decodes as b != 0 (core BytesCodec.java:24-33) */
  int32_t dtype_is_float;             /* float32 / float64: the write path's all-fill test
                                       * compares as Java's == (MultiArrayUtils.allValuesEqual,
                                       * MultiArrayUtils.java:69-80), so a ±0 fill matches
                                       * both zeros; other types compare bits */
  int64_t shape[ZH_MAX_DIMS];         /* array shape                                       */
  int32_t chunk_shape[ZH_MAX_DIMS];   /* regular chunk grid shape (= shard shape)          */
  uint8_t fill_value[8];              /* parsed fill value, element bytes little-endian     */
  zh_codec_chain chain;
} zh_array_meta;

/* One stored chunk (or shard) object.  data == NULL means the key does not exist in the
 * store (StoreHandle.exists() == false, M/core/Array.java:419-421). */
typedef struct zh_chunk_src {
  const void* data;
  int64_t nbytes;
} zh_chunk_src;

/* Destination of one encoded chunk object for zh_array_write. */
typedef struct zh_chunk_dst {
  void* data;          /* device buffer for the encoded bytes                         */
  int64_t capacity;    /* bytes available                                            */
  int64_t nbytes;      /* out: encoded size; 0 = chunk is all fill → delete key      */
} zh_chunk_dst;

typedef struct zh_ctx zh_ctx;
typedef struct zh_plan zh_plan;

/* ---- context -------------------------------------------------------------------- */
int zh_ctx_create(int device, zh_ctx** out);
void zh_ctx_destroy(zh_ctx* ctx);
int zh_ctx_device(const zh_ctx* ctx);
/* The context's default stream (a hipStream_t).  Calls with stream == NULL use it. */
void* zh_ctx_stream(zh_ctx* ctx);
/* Device blocks of finished plans are kept by the context (at most 8 GiB, blocks up to
 * 4 GiB) and reused by later plans: fresh device memory pays for its first touch.  Returns
 * them to the runtime; returns the bytes released.  No reference counterpart. */
int64_t zh_ctx_release_cache(zh_ctx* ctx);
const char* zh_version(void);

/* ---- host-side metadata helpers (no device needed) ------------------------------- */
/* Validates the chain against the reference rules (CodecPipeline ctor, sharding
 * divisibility ArrayMetadata.java:285-306, TransposeCodec.decode :35-41,
 * v3 BytesCodec.getByteOrder :43-48).  Returns ZH_EUNSUPPORTED for valid-but-not-
 * device-supported chains. */
int zh_validate_meta(const zh_array_meta* meta, char* err, size_t errlen);
/* 16 * prod(chunks per shard) (+4 with crc32c).  -1 for unsharded metas. */
int64_t zh_shard_index_size(const zh_array_meta* meta);
/* CRC32C.update over n bytes starting from a previous getValue() (0 for a fresh CRC32C). */
uint32_t zh_crc32c(uint32_t crc, const void* data, size_t n);
/* IndexingUtils.computeChunkCoords: writes up to max_coords rows of ndim int64 into
 * coords_out (may be NULL) in C order; returns the number of chunks, or -1 (ZH_EARITH
 * condition: more than Integer.MAX_VALUE chunks). */
int64_t zh_compute_chunk_coords(int ndim, const int64_t* array_shape, const int32_t* chunk_shape,
                                const int64_t* sel_offset, const int64_t* sel_shape,
                                int64_t* coords_out, int64_t max_coords);
/* IndexingUtils.computeProjection (5-arg).  Returns ZH_OK or ZH_EARITH. */
int zh_compute_projection(int ndim, const int64_t* chunk_coords, const int64_t* array_shape,
                          const int32_t* chunk_shape, const int64_t* sel_offset,
                          const int64_t* sel_shape, int32_t* chunk_offset_out,
                          int32_t* out_offset_out, int32_t* shape_out);
int zh_is_permutation(int n, const int32_t* order);
int zh_inverse_permutation(int n, const int32_t* order, int32_t* inverse_out);

/* ---- decode (the hot path) ------------------------------------------------------ */
/*
 * Prepared region read: the host half of core.Array.read (domain check, chunk
 * enumeration, projection, per-shard inner-chunk boxes) runs once in zh_plan_create;
 * zh_plan_execute only enqueues device work on `stream` (no allocation, no sync:
 * hipGraph-capturable); zh_plan_wait synchronises and reports deferred device errors
 * (CRC mismatch, corrupt index) with the reference's messages.
 *   chunks[i] belongs to the i-th chunk coordinate of
 *   computeChunkCoords(meta->shape, meta->chunk_shape, offset, shape) (C order).
 *   out = C-order buffer of prod(shape) elements.
 */
int zh_plan_create(zh_ctx* ctx, const zh_array_meta* meta, const zh_chunk_src* chunks,
                   int64_t nchunks, const int64_t* offset, const int64_t* shape, uint32_t flags,
                   zh_plan** out, char* err, size_t errlen);
int zh_plan_execute(zh_plan* plan, void* out, void* stream);
int zh_plan_wait(zh_plan* plan, char* err, size_t errlen);
/* Where the data error (ZH_EDATA) that the last read call on this thread reported sits in the
 * reference's sequential order: the failing chunk's grid coordinates (ndim
 * values into coords[0..cap)) and *key, its place inside that chunk (larger = earlier: the
 * index crc32c is ~0, else the failing inner chunk's C-order rank, complemented).  Returns
 * ndim, or 0 when that call placed no data error; the position is cleared once reported.
 * Multi-rank callers order the ranks' errors
 * by (coords, -key) so every rank reports the one a sequential read would have
 * (zarrhip.parallel.pick_error; the reference throws from its parallel chunk loop,
 * M/core/Array.java:403-407, 436-438). */
int zh_last_data_error(int64_t* coords, int cap, uint64_t* key);
void zh_plan_destroy(zh_plan* plan);
/* Plan statistics: bytes of encoded input read, output bytes written, number of
 * inner-chunk work items, shards touched. */
int zh_plan_stats(const zh_plan* plan, int64_t* in_bytes, int64_t* out_bytes,
                  int64_t* items, int64_t* nshards);
/* Diagnostic: the fast-path selection of the last decode scatter launch in this process
 * (encode = 0: aligned windows * 10^9 + fast_mode * 1000000 + kernel variant * 1000 +
 *  row group * 4 + (pieces ? 1 : 0))
 * or of the last write's encode view (encode = 1: fast_mode * 1000000 + chunk group * 1000 +
 * kernel form), or -1.  Tests use it to check that a switch reached the kernel it names. */
int64_t zh_debug_last_fast_path(int encode);
/* Per-kernel timing (HIP events around the scatter kernel on the launch stream).
 * enable=1 starts recording; zh_plan_kernel_time synchronises and returns the summed
 * scatter-kernel milliseconds and launch count since the last call. */
/* Bytes the plan copies host→device per execute (0 for device sources).  With host sources a
 * sub-shard part stages only its index + referenced inner chunks (StoreHandleDataProvider
 * semantics, ShardingIndexedCodec.java:333-357). */
int64_t zh_plan_staged_bytes(const zh_plan* plan);
int zh_plan_set_timing(zh_plan* plan, int enable);
/* enable=1: zh_plan_execute replays the plan as one hipGraph (captured on the first execute
 * for a given (out, stream); device sources and device output only, timing off).  For small
 * repeated reads this replaces ~8 enqueues with one graph launch. */
int zh_plan_set_graph(zh_plan* plan, int enable);
int zh_plan_kernel_time(zh_plan* plan, double* scatter_ms, int64_t* launches,
                        double* index_ms);

/* One-shot synchronous region read: plan + execute + wait. */
int zh_array_read(zh_ctx* ctx, const zh_array_meta* meta, const zh_chunk_src* chunks,
                  int64_t nchunks, const int64_t* offset, const int64_t* shape, void* out,
                  uint32_t flags, void* stream, char* err, size_t errlen);
/*
 * Multi-GPU region read in ONE process: the single-JVM form of SURVEY §8(b)'s
 * zh_decode_region_multi (one zarr-java Array.read spread over the GPUs of a node).
 *   The region splits into `ndev` contiguous C-order slabs along its first axis of extent
 *   >= ndev (all earlier axes must have extent 1; otherwise ctxs[root] decodes it whole),
 *   with boundaries on inner-chunk multiples (zh_slab_partition).  Slab r is planned on
 *   ctxs[r] over the chunks it touches and decoded there; all devices work concurrently,
 *   one host thread each.  chunks[] follows computeChunkCoords of the WHOLE region, as in
 *   zh_array_read; flags as there:
 *     no ZH_OUT_DEVICE : host-terminated — slab r is copied D2H straight into its slice of
 *                        the host buffer `out`, each device over its own PCIe link (pin
 *                        `out` with zh_host_register for the full rate);
 *     ZH_OUT_DEVICE    : `out` is a buffer on ctxs[root]'s device; the other devices decode
 *                        into their own HBM and copy their slab to the root's slice over
 *                        xGMI (hipMemcpyPeerAsync), or through pinned host memory when the
 *                        pair has no peer access (see zh_array_read_multi_routed).
 *   Errors: zh_array_read's messages; when the slabs' failures are all data errors the
 *   device placed (checksums, index entries), the first of them in zh_array_read's order (the
 *   chunk first in C order, then the error within it; slabs may cut a shard), else the first
 *   failing slab in C order.
 * zh_slab_partition writes nslabs rows of ndim int64 offsets / shapes (ZH_EINVAL when the
 * region cannot be split into nslabs contiguous slabs).
 */
int zh_array_read_multi(zh_ctx* const* ctxs, int ndev, int root, const zh_array_meta* meta,
                        const zh_chunk_src* chunks, int64_t nchunks, const int64_t* offset,
                        const int64_t* shape, void* out, uint32_t flags, char* err,
                        size_t errlen);
/*
 * zh_array_read_multi with a per-slab route report (slab_route: ndev int32, may be NULL):
 *   output  ZH_ROUTE_DIRECT  decoded straight into its destination (root slab / host slice)
 *           ZH_ROUTE_PEER    device-to-device copy to the root over xGMI (peer access on)
 *           ZH_ROUTE_STAGED  no peer access: D2H into pinned host memory, then H2D on a fresh
 *                            stream of the root device
 *           ZH_ROUTE_SAME    two contexts on one device: a device-local copy
 *   sources (ZH_SRC_DEVICE chunks on another device than the slab's), OR-ed in:
 *           ZH_ROUTE_SRC_PEER    the kernels read them over xGMI (peer access on)
 *           ZH_ROUTE_SRC_STAGED  copied to the slab's device first (no peer access)
 *   ZH_MULTI_FORCE_STAGED=1 stages every non-root slab even on one device (tests).
 */
#define ZH_ROUTE_DIRECT 0
#define ZH_ROUTE_PEER 1
#define ZH_ROUTE_STAGED 2
#define ZH_ROUTE_SAME 3
#define ZH_ROUTE_SRC_PEER 4
#define ZH_ROUTE_SRC_STAGED 8
int zh_array_read_multi_routed(zh_ctx* const* ctxs, int ndev, int root,
                               const zh_array_meta* meta, const zh_chunk_src* chunks,
                               int64_t nchunks, const int64_t* offset, const int64_t* shape,
                               void* out, uint32_t flags, int32_t* slab_route, char* err,
                               size_t errlen);
int zh_slab_partition(int ndim, const int64_t* offset, const int64_t* shape, int nslabs,
                      int64_t align, int64_t* slab_off, int64_t* slab_shape);
/* Number of visible HIP devices (0 when none). */
int zh_device_count(void);

/* ---- sub-shard reads from the index and the referenced pieces ------------------------
 * core.Array.read of a region that covers part of a shard goes through
 * ShardingIndexedCodec.decodePartial → StoreHandleDataProvider (ShardingIndexedCodec.java:
 * 245-255, 333-357): one prefix/suffix read of the shard's index, then one range read per
 * referenced inner chunk.  The Java side does exactly that I/O and nothing else; the stored
 * index goes to the device unchanged, where its crc32c is verified (Crc32cCodec.decode,
 * Crc32cCodec.java:24-48) and its entries are parsed and mapped onto the pieces.  A shard is
 * never assembled on the host, so a part whose referenced payload exceeds 2^31 bytes (a Java
 * array) reads like any other.
 *
 * zh_shard_ranges: the byte ranges of one stored shard a part needs.  index = the
 * index_nbytes bytes the prefix/suffix read returned (16 per inner chunk [+ 4 crc32c]);
 * shard_nbytes = StoreHandle.getSize() or -1 when the store cannot tell; [part_lo, part_hi) =
 * shard-local element box.  Entries of the part's inner-chunk box (nested sharding: its
 * level-1 cells, read whole), missing ones (-1) dropped, are sorted by offset.  max_run > 0:
 * overlapping entries are united and adjacent ranges merged while a run stays <= max_run
 * bytes; no range ever exceeds 2^31 - 1 bytes (a union that would continues as a new range).
 * max_run == 0 (chains whose host stages decode each inner chunk on its own): one range per
 * entry, overlapping or not, exact duplicates once.  Entries that cannot be read (negative,
 * beyond a known shard_nbytes, longer than 2^31 - 1) are left out: the device then reports
 * them with the reference's "Could not load byte data for chunk [...]" unless the index
 * crc32c fails first.  The index crc32c is NOT checked here (zh_shard_index_check).  Writes up to `cap` (offset, nbytes) pairs to
 * `ranges` (may be NULL) and returns the number of ranges; a negative return is -zh_status
 * (EINVAL: not a sharded meta, index_nbytes below the index size, bad part box). */
int64_t zh_shard_ranges(const zh_array_meta* meta, const void* index, int64_t index_nbytes,
                        int64_t shard_nbytes, const int64_t* part_lo, const int64_t* part_hi,
                        int64_t max_run, int64_t* ranges, int64_t cap);

/* Crc32cCodec.decode of a stored shard index on the host (Crc32cCodec.java:24-48): ZH_OK when
 * the chain's index has no crc32c or it matches, ZH_EDATA with the reference's message
 * ("The checksum of the sharding index is invalid. Stored: <int> Computed: <int>") when it does
 * not.  A sub-shard read normally leaves the check to the device; a binding calls this first
 * when the index decides host work before the device sees it: inner chains with host stages
 * (each referenced range is decoded on the host) or a store that cannot tell the shard size
 * (a corrupt entry could ask for a 2^31-byte range read).  The reference checks the index
 * before any range read (ShardingIndexedCodec.java:205). */
int zh_shard_index_check(const zh_array_meta* meta, const void* index, int64_t index_nbytes,
                         char* err, size_t errlen);

/* One byte range of a stored shard as the store returned it.  Pieces are sorted by offset and
 * disjoint, except host-decoded pieces (data_nbytes != nbytes), which may overlap one another
 * at distinct offsets: each serves exactly the entry (offset, nbytes) it was read for. */
typedef struct zh_shard_piece {
  int64_t offset;      /* shard byte offset of the range                                       */
  int64_t nbytes;      /* stored bytes in the range (one inner chunk or a run of adjacent ones) */
  const void* data;    /* the bytes: host memory, or device memory with ZH_SRC_DEVICE          */
  int64_t data_nbytes; /* == nbytes: the stored bytes.  Otherwise the range is exactly one
                          inner chunk whose host byte-to-byte stages (zstd, gzip, blosc) were
                          undone: data holds its raw `bytes` payload (+ crc32c)               */
} zh_shard_piece;

/* One stored shard of a region read (computeChunkCoords order).
 *   missing key (StoreHandle.exists() false): index = NULL, npieces = 0 → fill_value;
 *   whole shard as one object: index = NULL, one piece at offset 0 holding all its bytes;
 *   sub-shard part: index = the stored index bytes, pieces = the ranges zh_shard_ranges
 *     named (in any grouping: a piece must cover each entry it serves; sorted by offset,
 *     not overlapping).  An entry no piece covers reads as "Could not load byte data". */
typedef struct zh_shard_src {
  const void* index;
  int64_t index_nbytes;
  int64_t shard_nbytes;           /* StoreHandle.getSize(), -1 when unknown                   */
  const zh_shard_piece* pieces;
  int64_t npieces;
} zh_shard_src;

/* zh_array_read over shards given as index + pieces (HipArray.read's sub-shard form).
 * Sharded chains only (ZH_EINVAL otherwise).  Host pieces are staged into the device (page-
 * locked sources by direct DMA, pageable ones through the context's pinned ring); the device
 * checks each stored index's crc32c and resolves every entry against the pieces.  Large host
 * reads run pipelined (H2D | decode | D2H) as zh_array_read does. */
int zh_array_read_pieces(zh_ctx* ctx, const zh_array_meta* meta, const zh_shard_src* shards,
                         int64_t nshards, const int64_t* offset, const int64_t* shape, void* out,
                         uint32_t flags, void* stream, char* err, size_t errlen);
/* zh_array_read_multi_routed over shards given as index + pieces (one JVM, several GPUs). */
int zh_array_read_pieces_multi(zh_ctx* const* ctxs, int ndev, int root,
                               const zh_array_meta* meta, const zh_shard_src* shards,
                               int64_t nshards, const int64_t* offset, const int64_t* shape,
                               void* out, uint32_t flags, int32_t* slab_route, char* err,
                               size_t errlen);
/* ShardingIndexedCodec.decodePartial(StoreHandle, offset, shape) over one shard given as
 * index + pieces (HipShardingIndexedCodec's form): shard-local offset/shape → shape elements. */
int zh_sharding_decode_pieces(zh_ctx* ctx, const zh_array_meta* meta, const zh_shard_src* shard,
                              const int64_t* offset, const int32_t* shape, void* out,
                              uint32_t flags, void* stream, char* err, size_t errlen);
/* Page-locked host staging owned by the context, for bindings that copy their sources out of
 * a managed heap before a read (the JNI shim does not: it hands the library its arrays in
 * bounded critical sections): at least `bytes`, valid until the next call on
 * this context or zh_ctx_destroy; grown on demand, kept across calls up to ZH_STAGING_MAX_MB
 * (default 8192; larger requests get a one-off buffer that the next call frees).  Takes the
 * context's lock, so it never replaces the staging under a read in flight on another thread;
 * the caller must not use the previous pointer once it calls again. */
int zh_host_staging(zh_ctx* ctx, size_t bytes, void** out);

/* ---- region reads straight from a FilesystemStore ---------------------------------------
 * core.Array.read when every chunk key resolves to a file (StoreHandle.toPath(),
 * M/store/StoreHandle.java:96-101): the library does the store I/O itself.
 *
 * The store: root = FilesystemStore's directory, name = FilesystemStore.toString() (its file:
 * URI without the trailing '/', FilesystemStore.java:194-197; NULL → "file://" + root).  A
 * NULL store means the filesystem root ("/", named "file://").  Errors name the store and the
 * key as StoreException does (StoreException.java:17-35): "Failed to read from store '<name>'
 * at key '<key>': <reason>", the key being the path below root ('/'-joined keys).
 *
 * paths[i] is the file of the i-th chunk of computeChunkCoords(meta->shape, meta->chunk_shape,
 * offset, shape); NULL, or a path that is not a regular file, is a missing key
 * (FilesystemStore.exists, FilesystemStore.java:42-45) → fill_value.  Per file the reads are
 * the reference's:
 *   unsharded:           the whole object (get(keys), :47-57);
 *   sharded, whole shard (the part is the full chunk: decodePartial → chunkHandle.read(),
 *                        ShardingIndexedCodec.java:246-251): the index and the referenced
 *                        ranges of the file as it is; an index or entry beyond the file is an
 *                        error (ZH_EDATA; the reference's ByteBuffer slicing throws);
 *   sharded, part        (StoreHandleDataProvider, ShardingIndexedCodec.java:333-357): the
 *                        index by a prefix (index_location start, get(keys, 0, n)) or suffix
 *                        (get(keys, -n)) read, then the referenced inner-chunk ranges
 *                        (get(keys, off, off + n), adjacent ranges merged).  As in
 *                        get(keys, start, end) (:84-102), bytes past the end of the file read as
 *                        zeros: a truncated file decodes with zeros where its bytes are missing,
 *                        and a prefix index read of a file shorter than the index is zero-padded
 *                        (its crc32c then fails).  A suffix read of a file shorter than the
 *                        index is an error (ZH_EDATA; the reference's position(< 0) throws).
 * The index crc32c and every entry are checked on the device, as with zh_array_read_pieces.
 * The range reads (pread) write straight into the page-locked ring of the pipelined read, so
 * the file bytes are copied once on the host and the reads overlap the H2D copies, the decode
 * and the D2H of earlier slabs.  At most 64 files are open at once whatever the region's
 * chunk count (a closed one is reopened by path for its next range).  `out`: host memory
 * (flags 0) or device memory (ZH_OUT_DEVICE); ZH_SRC_DEVICE is not allowed.  A file that cannot
 * be opened or read (other than missing) → ZH_EIO with the readFailed text.  The chain must be
 * device-supported (zh_validate_meta); chains with host byte-to-byte stages keep their store
 * reads on the binding side (zh_array_read_pieces). */
typedef struct zh_file_store {
  const char* root; /* FilesystemStore's directory                                          */
  const char* name; /* FilesystemStore.toString(); NULL: "file://" + root                     */
} zh_file_store;
int zh_array_read_files(zh_ctx* ctx, const zh_array_meta* meta, const zh_file_store* store,
                        const char* const* paths, int64_t npaths, const int64_t* offset,
                        const int64_t* shape, void* out, uint32_t flags, char* err,
                        size_t errlen);
/* zh_array_read_files spread over several GPUs in one process (zh_array_read_multi_routed's
 * slabs and routes; HipArray.read with ZH_DEVICES): every device reads the files of its slab
 * and decodes it, a host-terminated read copying each slab straight into its slice of `out`
 * (each device over its own PCIe link). */
int zh_array_read_files_multi(zh_ctx* const* ctxs, int ndev, int root, const zh_array_meta* meta,
                              const zh_file_store* store, const char* const* paths,
                              int64_t npaths, const int64_t* offset, const int64_t* shape,
                              void* out, uint32_t flags, int32_t* slab_route, char* err,
                              size_t errlen);
/* core.Array.write of a region of whole chunks (clipped only by the array boundary) into a
 * FilesystemStore: the device encode of zh_array_write, then per chunk writeChunk's store call
 * (M/core/Array.java:143-156) done here — all fill_value → the file deleted (FilesystemStore.delete,
 * a missing file is fine), otherwise the parent directories created and the chunk's bytes
 * stored at its path (FilesystemStore.set, M/store/FilesystemStore.java:105-128).  The encoded
 * bytes go D2H through the page-locked ring in windows that several lanes pwrite into a
 * temporary file beside the chunk's, renamed over it once complete: a failure leaves every
 * chunk it did not complete as it was (the reference truncates a file before writing it), and
 * at most 3 files per lane are open at once.  paths[i]: the i-th chunk of computeChunkCoords;
 * src: the region in C order on the host, or on the device with ZH_SRC_DEVICE; nbytes (may be
 * NULL): per chunk the bytes written (0: deleted).  A region that cuts chunks → ZH_EUNSUPPORTED
 * (the binding's read-modify-write); a store failure → ZH_EIO with StoreException's text
 * (writeFailed: "... Failed to write <n> bytes to file: <path>" or "... Failed to create parent
 * directories for path: <dir>"; deleteFailed: "... Failed to delete file: <path>"). */
int zh_array_write_files(zh_ctx* ctx, const zh_array_meta* meta, const void* src,
                         const int64_t* offset, const int64_t* shape, const zh_file_store* store,
                         const char* const* paths, int64_t npaths, uint32_t flags,
                         int64_t* nbytes, char* err, size_t errlen);
/* Diagnostic (no device needed): the store reads zh_array_read_files would make for these
 * paths, as (chunk index, file offset, bytes) triples in order — a whole object, or a shard's
 * index read followed by its merged range reads; missing keys make none.  Writes up to `cap`
 * triples to `reads` (may be NULL) and returns their number, or -zh_status with err set (the
 * same checks and messages as the read).  Tests use it to check the read plan on the host. */
int64_t zh_debug_file_reads(const zh_array_meta* meta, const zh_file_store* store,
                            const char* const* paths, int64_t npaths, const int64_t* offset,
                            const int64_t* shape, int64_t* reads, int64_t cap, char* err,
                            size_t errlen);
/* Diagnostic (no device needed): the process-wide file table of the file reads —
 * out[0] = slots in use, out[1] = descriptors open, out[2] = entries in the queue of opens
 * (bounded: stale entries are dropped as files are given back).  Returns ZH_OK. */
int zh_debug_file_table(int64_t* out);

/* ShardingIndexedCodec.decode: whole shard → chunk_shape elements. */
int zh_sharding_decode(zh_ctx* ctx, const zh_array_meta* meta, const void* shard, int64_t nbytes,
                       void* out, uint32_t flags, void* stream, char* err, size_t errlen);
/* ShardingIndexedCodec.decodePartial: shard-local offset/shape → shape elements. */
int zh_sharding_decode_partial(zh_ctx* ctx, const zh_array_meta* meta, const void* shard,
                               int64_t nbytes, const int64_t* offset, const int32_t* shape,
                               void* out, uint32_t flags, void* stream, char* err,
                               size_t errlen);

/* ---- encode (write path) ---------------------------------------------------------- */
/*
 * Device encode of every chunk intersecting [offset, offset+shape), which must cover
 * whole chunks (clipped only by the array boundary); src is that region in C order on
 * the device.  Inner chunks that are all fill_value become (-1,-1) index entries and
 * are laid out in C order (deterministic; the reference's order is not — SURVEY Q7).
 * A chunk that is entirely fill reports nbytes = 0 (writeChunk deletes it).
 * dsts[i] follows computeChunkCoords order.  zh_array_encoded_bound gives the worst-
 * case encoded size of one chunk.
 */
int64_t zh_array_encoded_bound(const zh_array_meta* meta);
int zh_array_write(zh_ctx* ctx, const zh_array_meta* meta, const void* src,
                   const int64_t* offset, const int64_t* shape, zh_chunk_dst* dsts,
                   int64_t nchunks, void* stream, char* err, size_t errlen);
/* zh_array_write for host buffers (the JNI write path: the region is a Java array, the
 * encoded chunks become byte[]s): src_host holds the region in C order; the encoded chunk i
 * is copied to outs[i] (capacities[i] bytes available) and its size stored in nbytes[i]
 * (0 = chunk is all fill → delete the key).  A capacity below the encoded size → ZH_EINVAL
 * naming the size needed; zh_array_encoded_bound always suffices.  Staging goes through the
 * context's block cache. */
int zh_array_write_host(zh_ctx* ctx, const zh_array_meta* meta, const void* src_host,
                        const int64_t* offset, const int64_t* shape, void* const* outs,
                        const int64_t* capacities, int64_t* nbytes, int64_t nchunks, char* err,
                        size_t errlen);

/* ---- device memory / stream / event plumbing for callers without their own ---------- */
/* sizeof of the public structs, for binding-side layout checks (ctypes / JNI mirrors):
 * out[0..3] = zh_codec_chain, zh_array_meta, zh_chunk_src, zh_chunk_dst.  Returns 4. */
int zh_abi_sizes(int64_t* out, int n);
/* Device memory for regions and shards, the library's default kind (zh_device_malloc_ex with
 * flags 0): a buffer of at least 1 GiB is built from 1 GiB physical chunks (ZH_MALLOC_SCATTER,
 * falling back to hipMalloc), a smaller one is hipMalloc'd.  Round 6 timed the full c4 decode
 * into 3 fresh outputs of each kind on three boxes (DESIGN.md §4 "Placement"): 1 GiB chunks had
 * the highest floor on each (2871 / 2869 / 2927 GiB/s against hipMalloc's 2841 / 2844 / 2913
 * and 16 MiB chunks' 2803 / 2830 / 2900). */
int zh_device_malloc(zh_ctx* ctx, size_t bytes, void** out);
/* Allocation flags for zh_device_malloc_ex.  The write bandwidth a large buffer gets depends
 * on where its physical memory lands (DESIGN.md §4 "Placement": writes only, any access
 * pattern, not TLB or L2-channel balance).  ZH_MALLOC_CONTIGUOUS asks for physically
 * contiguous HBM (hipDeviceMallocContiguous).  Falls back to hipMalloc unless
 * ZH_MALLOC_REQUIRE. */
#define ZH_MALLOC_CONTIGUOUS 0x1u
#define ZH_MALLOC_REQUIRE 0x2u
/* Physical chunks (hipMemCreate, ZH_SCATTER_MB MiB each, default 1024) mapped into one virtual
 * range in a coprime-stride order, so that virtually adjacent chunks are not physically
 * adjacent: the decode's output arena in bench.py (DESIGN.md §4 "Placement": mean +5.6 % over
 * hipMalloc on 18 buffers, 3 boxes).  The rest beyond the last whole chunk gets one smaller
 * chunk (rounded up to the allocation granularity), mapped last.  Freed by zh_device_free. */
#define ZH_MALLOC_SCATTER 0x4u
/* With ZH_MALLOC_SCATTER: allocate two candidate arenas (the first held while the second is
 * allocated, so each gets other physical chunks), time a contiguous
 * store probe over each (zh_device_write_rate pattern 0) and keep the fastest.  A large
 * arena's write rate is set by its physical chunks (not their order or its address) and the
 * probe predicts the decode's rate into it (DESIGN.md §4 "Placement").  Needs the memory of
 * two arenas while it runs; a candidate that does not fit ends the search.  The buffer's
 * contents are undefined.  zh_device_alloc_probes reports the probes. */
#define ZH_MALLOC_CALIBRATE 0x8u
/* hipMalloc whatever the size (the default kind's small-buffer form for every size). */
#define ZH_MALLOC_PLAIN 0x10u
int zh_device_malloc_ex(zh_ctx* ctx, size_t bytes, unsigned flags, void** out);
/* Map a ZH_MALLOC_SCATTER allocation's physical chunks a second time, at a fresh virtual
 * range, in chunk order `order` (0 = the allocation's order: slot i <- chunk (i*m) mod n;
 * k > 0: another coprime stride and a rotation).  The view aliases the allocation's memory;
 * free it with zh_device_free before the allocation.  ZH_EINVAL for a pointer that is not a
 * scatter allocation.  (Re-mapping a live range in place is not offered: on ROCm 7.2 the
 * device kept translations of the old mapping, DESIGN.md §4 "Placement".) */
/* Probe rates (GB/s) of the candidates ZH_MALLOC_CALIBRATE tried for `ptr`, in allocation
 * order; *chosen = the index of `ptr` among them.  Returns the number of candidates (0 for an
 * allocation that was not calibrated), or -ZH_EINVAL. */
int zh_device_alloc_probes(zh_ctx* ctx, void* ptr, double* gbps, int cap, int* chosen);
int zh_device_scatter_view(zh_ctx* ctx, void* ptr, uint64_t order, void** out);
/* Write bandwidth of [ptr, ptr+bytes): one untimed and `reps` timed launches of a store-only
 * probe on the context stream (pattern 0: contiguous 16-B stores; 1: the decode kernels' store
 * pattern, 128-B lines 6 KiB apart).  *gbps = bytes / median time, in 1e9 B/s.  Overwrites
 * the buffer. */
int zh_device_write_rate(zh_ctx* ctx, void* ptr, size_t bytes, int pattern, int reps,
                         double* gbps);
/* Copy ceiling of a buffer pair: one untimed and `reps` timed launches of a streaming
 * byte-swapping copy src -> dst over the first bytes rounded down to 128 KiB (non-temporal
 * 16-B loads and stores, 128 KiB per workgroup step: the fastest stream of
 * tools/copy_lab.hip).  *gbps = (bytes read + bytes written) / median time, in 1e9 B/s, the
 * decode's own traffic count.  Overwrites dst.  ZH_EINVAL below 128 KiB. */
int zh_device_copy_rate(zh_ctx* ctx, void* dst, const void* src, size_t bytes, int reps,
                        double* gbps);
int zh_device_free(zh_ctx* ctx, void* ptr);
int zh_host_malloc_pinned(zh_ctx* ctx, size_t bytes, void** out);
int zh_host_free_pinned(zh_ctx* ctx, void* ptr);
/* Page-lock caller-owned host memory (hipHostRegister), e.g. one rank's slice of a region
 * buffer shared by the processes of a multi-GPU read, so that its D2H runs at pinned rate. */
int zh_host_register(zh_ctx* ctx, void* ptr, size_t bytes);
int zh_host_unregister(zh_ctx* ctx, void* ptr);
/* kind: 0 H2D, 1 D2H, 2 D2D; asynchronous on stream */
int zh_memcpy_async(zh_ctx* ctx, void* dst, const void* src, size_t bytes, int kind, void* stream);
int zh_memset_async(zh_ctx* ctx, void* dst, int value, size_t bytes, void* stream);
int zh_stream_synchronize(zh_ctx* ctx, void* stream);
int zh_stream_create(zh_ctx* ctx, void** stream);
int zh_stream_destroy(zh_ctx* ctx, void* stream);
/* make `stream` wait for `ev` (recorded on another stream) */
int zh_stream_wait_event(zh_ctx* ctx, void* stream, void* ev);
/* pitched copy of `height` rows of `width` bytes; kind as zh_memcpy_async */
int zh_memcpy2d_async(zh_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width, size_t height, int kind, void* stream);
int zh_event_create(zh_ctx* ctx, void** ev);
int zh_event_destroy(zh_ctx* ctx, void* ev);
int zh_event_record(zh_ctx* ctx, void* ev, void* stream);
int zh_event_elapsed_ms(zh_ctx* ctx, void* start, void* stop, float* ms);
int zh_device_info(zh_ctx* ctx, char* name, size_t namelen, int64_t* total_mem,
                   int* cu_count, char* arch, size_t archlen);

/* ---- host byte-to-byte stage: blosc1 frames ----------------------------------------
 * Replaces the blosc-java call inside BloscCodec.decode (M/v3/codec/core/BloscCodec.java,
 * M/v2/codec/core/BloscCodec.java) for hosts without the blosc library: BloscLZ, LZ4/LZ4HC,
 * zlib and zstd payloads, byte and bit shuffle, split and unsplit blocks, memcpyed frames.
 * dst == NULL only reports the decompressed size in *nbytes_out.  Snappy payloads
 * → ZH_EUNSUPPORTED. */
int zh_blosc_decompress(const void* src, size_t srclen, void* dst, size_t dstcap,
                        size_t* nbytes_out, char* err, size_t errlen);

/* ---- blosc1 frames decoded on the device, a batch at a time ---------------------------
 * Frames whose streams are LZ4, BloscLZ or stored raw are independent blocks of independent
 * streams: the compressed bytes cross PCIe and one kernel decodes every stream of the batch
 * (one workgroup per block, one wavefront per stream) and undoes the byte / bit shuffle.
 * Memcpyed frames are one copy; zlib and zstd payloads are decoded by zh_blosc_decompress on
 * the host and copied, unless the _ex calls below are given the flag that sends them to the
 * device.  The decoded frames lie in one device buffer at dst_off. */
typedef struct zh_blosc_frame {
  const void* src;   /* the stored frame, host memory                               */
  int64_t srclen;
  int64_t dst_off;   /* out (plan): offset in the batch destination, 256-B aligned  */
  int64_t nbytes;    /* out (plan): decoded size                                    */
  int32_t where;     /* out (plan): 0 device streams, 1 host fallback (zlib / zstd
                        payload: zh_blosc_decompress into pinned staging, then H2D),
                        2 memcpyed                                                  */
  int32_t status;    /* out: ZH_OK or this frame's error                            */
} zh_blosc_frame;

/* No device needed: validates headers with the checks and texts of zh_blosc_decompress's
 * size query, fills dst_off / nbytes / where, returns the destination bytes or -zh_status
 * (the first bad frame in batch order; its status field is set). */
int64_t zh_blosc_batch_plan(zh_blosc_frame* frames, int64_t n, char* err, size_t errlen);

/* Plans as above, stages the compressed bytes H2D through the context's pinned ring, decodes
 * on `stream` (NULL: the context's), waits, and reports the first failing frame in batch order
 * with the host decoder's text ("corrupt blosc block", ...) and status.  dst is device memory
 * of dstcap >= the plan's bytes.  After a failed call dst is undefined; the context stays
 * usable. */
int zh_blosc_decode_batch(zh_ctx* ctx, zh_blosc_frame* frames, int64_t n, void* dst,
                          int64_t dstcap, void* stream, char* err, size_t errlen);

/* Diagnostic: milliseconds the decode kernel of the last successful zh_blosc_decode_batch in
 * this process took, by device events around its launch (-1: none yet, or no device frame). */
double zh_debug_blosc_kernel_ms(void);

/* Diagnostic, no device: the block / stream table of one device-decoded frame, as rows of 6
 * int64 — per block (0, offset in the decoded frame, size, typesize, shuffle kind: 0 none,
 * 1 byte, 2 bit with the format-2 leftover rule, 3 bit with the format-3 rule, streams)
 * followed by its streams (1, payload offset in the frame, csize, offset in the shuffled
 * block, raw size, method: 0 raw copy, 1 LZ4, 2 BloscLZ).  Writes up to `cap` rows to `rows`
 * (may be NULL) and returns their number, or -zh_status with err set (header and chain errors
 * as zh_blosc_decompress words them; ZH_EUNSUPPORTED for memcpyed and host-decoded frames). */
int64_t zh_debug_blosc_streams(const void* src, size_t srclen, int64_t* rows, int64_t cap,
                               char* err, size_t errlen);

/* The three calls above with flags; flags = 0 is exactly those calls, any unknown bit is
 * ZH_EINVAL.  ZH_BLOSC_ZSTD_DEVICE: a frame with compressor code 4 (zstd) is planned where = 0
 * when its block / stream chain is sound and every stream is stored raw or ONE zstd frame that
 * ends at the stream's last byte, has no dictionary and no checksum, and whose content size is
 * the stream's raw size (what ZSTD_compress, which c-blosc calls, writes).  Such streams are
 * decoded one wavefront each by the library's zstd frame decoder into the block's window before
 * the kernel above undoes the shuffle; the diagnostic reports them with method 3.  Any other
 * zstd frame (a stream with a checksum, without or with another content size, concatenated or
 * skippable frames) stays where = 1.
 * ZH_BLOSC_ZLIB_DEVICE: a frame with compressor code 3 (zlib) is planned where = 0 when its
 * chain is sound and every stream is stored raw or begins with a zlib header that inflate
 * accepts (CM 8, valid check bits, no preset dictionary) and that declares the 32 KiB window
 * (CINFO 7: what compress2, which c-blosc calls, writes).  Such streams are decoded one wavefront
 * each by the library's DEFLATE decoder, which also computes the Adler-32 of what it wrote; a
 * stream is good when exactly its raw size came out and the Adler-32 is the stored one (bytes
 * behind the trailer are ignored, as uncompress ignores them).  The diagnostic reports them with
 * method 4.  A frame with any other stream stays where = 1.  Without its flag a compressor's
 * payloads stay on the host.  The value is 4: 2 is not a flag.
 * The device memory of one launch is bounded: at most 128 MiB of decoded zstd and zlib frames go
 * into one slab (a larger frame is its own), and a slab's literal scratch and shuffle temporary
 * are each at most its decoded bytes.  zh_debug_blosc_kernel_ms covers all kernels of every
 * slab. */
#define ZH_BLOSC_ZSTD_DEVICE 1u
#define ZH_BLOSC_ZLIB_DEVICE 4u
int64_t zh_blosc_batch_plan_ex(zh_blosc_frame* frames, int64_t n, unsigned flags, char* err,
                               size_t errlen);
int zh_blosc_decode_batch_ex(zh_ctx* ctx, zh_blosc_frame* frames, int64_t n, unsigned flags,
                             void* dst, int64_t dstcap, void* stream, char* err, size_t errlen);
int64_t zh_debug_blosc_streams_ex(const void* src, size_t srclen, unsigned flags, int64_t* rows,
                                  int64_t cap, char* err, size_t errlen);

/* ---- blosc1 LZ4 frames written on the host and on the device ---------------------------
 * The writer of the frames the decoders above read: version 2, compressor code 1 (LZ4), byte
 * or bit shuffle (format-2 rule), blocks of at most 64 KiB (a larger configured block size is
 * clamped), split into typesize streams when the shuffle is the byte shuffle, typesize <= 16
 * and blocksize / typesize >= 128.  A stream LZ4 would not shrink is stored raw; a frame that
 * would pass nbytes + 16 is written MEMCPYED, so cbytes <= nbytes + 16 always.  The bytes are
 * a pure function of (input, typesize, shuffle, block size): the host call and the batch call
 * give the same frame. */
typedef struct zh_blosc_enc_params {
  int32_t typesize;   /* 1..255                                */
  int32_t shuffle;    /* 0 none, 1 byte, 2 bit                 */
  int32_t blocksize;  /* 0: default (16 KiB); above 64 KiB: 64 KiB */
} zh_blosc_enc_params;

typedef struct zh_blosc_enc_frame {
  const void* src;   /* raw bytes: device memory for the batch call            */
  int64_t nbytes;
  int64_t dst_off;   /* out: place of the frame in dst, 16-byte aligned        */
  int64_t cbytes;    /* out: size of the frame                                 */
  int32_t status;    /* out: ZH_OK or this frame's error                       */
} zh_blosc_enc_frame;

/* Host, no device: one frame.  dst == NULL: *cbytes = the bound nbytes + 16 (cap must reach
 * it otherwise).  typesize outside 1..255 (or another bad parameter) → ZH_EINVAL. */
int zh_blosc_compress(const void* src, size_t n, const zh_blosc_enc_params* params, void* dst,
                      size_t cap, size_t* cbytes, char* err, size_t errlen);

/* Host memory a batch needs for its frames: the sum of nbytes + 16, each rounded up to 16
 * bytes; or -zh_status. */
int64_t zh_blosc_encode_bound(const zh_blosc_enc_frame* frames, int64_t n,
                              const zh_blosc_enc_params* params);

/* Sources in device memory; the frames arrive in host memory dst (dstcap >= the bound) at
 * dst_off, cbytes long, compressed by one kernel (one workgroup per block, one wavefront per
 * stream), laid out by a second, and copied back through the context's page-locked ring: only
 * the compressed bytes and the size tables cross PCIe.  Runs on `stream` (NULL: the
 * context's) and waits.  Batches are worked off in slabs of at most 128 MiB of raw bytes (a
 * larger frame is its own slab), which bounds the device memory of a call. */
int zh_blosc_encode_batch(zh_ctx* ctx, zh_blosc_enc_frame* frames, int64_t n,
                          const zh_blosc_enc_params* params, void* dst, int64_t dstcap,
                          void* stream, char* err, size_t errlen);

/* Diagnostic: milliseconds the kernels of the last successful zh_blosc_encode_batch or
 * zh_blosc_encode_batch_ex took, by device events around their launches, summed over its slabs
 * (-1: none yet). */
double zh_debug_blosc_encode_kernel_ms(void);

/* The same writer with flags.  flags = 0: exactly the two calls above.  ZH_BLOSC_ENC_ZSTD: the
 * frame carries compressor code 4 and its streams are zstd frames: same block size rule,
 * shuffle flags, split rule and block starts; a stream's payload is, byte for byte, what
 * zh_zstd_compress writes for the stream's shuffled bytes with checksum 0 and blocksize 64 KiB
 * (one frame of one compressed block behind the 13-byte header with the 8-byte content size)
 * when that is shorter than the stream, else the raw bytes.  A frame that would pass
 * nbytes + 16 is written MEMCPYED; zh_blosc_encode_bound holds for every flag.  The batch call
 * runs three kernels per slab (match finder: one workgroup per block, one wavefront per
 * stream; sequence coder: one thread per stream; raw streams) before the layout kernel; a slab's
 * device memory is its raw bytes three and a half times over (scratch: the raw size and 16
 * bytes per stream; records: 1.5 x; the compact frames) and the small tables.  Any other bit →
 * ZH_EINVAL.  zh_blosc_decompress, libzstd on the streams, and zh_blosc_decode_batch_ex with
 * ZH_BLOSC_ZSTD_DEVICE read these frames.
 * ZH_BLOSC_ENC_ZLIB: the frame carries compressor code 3 and every stream is one RFC 1950 zlib
 * stream of its shuffled bytes: 78 01, then what zh_gzip_compress with blocksize 16 KiB puts
 * between its 10 header bytes and its 8 trailer bytes (one byte-aligned stored or fixed segment
 * per 16 KiB piece, each with its sync marker, and the final empty fixed block 03 00), then the
 * Adler-32 of the shuffled bytes, big-endian; a stream whose payload would reach its raw size is
 * stored raw.  ZH_BLOSC_ENC_DYNAMIC, valid only together with ZH_BLOSC_ENC_ZLIB: a segment may
 * take the dynamic form, as zh_gzip_enc_params::dynamic = 1 allows.  The batch call writes the
 * slab's shuffled blocks to device memory once (shuffle kernel, with the Adler-32 of every
 * stream behind it), runs the gzip writer's match and coding kernels over the 16 KiB pieces
 * and lays the frames out with the layout kernel; a slab's device memory is its raw bytes four
 * and a half times over.  zh_blosc_decompress, zlib on the streams, and zh_blosc_decode_batch_ex
 * with ZH_BLOSC_ZLIB_DEVICE read these frames.  The valid flag words are 0, 1, 4 and 12; the
 * value of the zlib bit is 4 because 2 and 3 are refused by every release. */
#define ZH_BLOSC_ENC_ZSTD 1u
#define ZH_BLOSC_ENC_ZLIB 4u
#define ZH_BLOSC_ENC_DYNAMIC 8u
/* Diagnostic: zh_debug_blosc_encode_kernel_ms of the last successful batch with
 * ZH_BLOSC_ENC_ZLIB, apart: out[0] the shuffle kernel (with the Adler-32), out[1] the match and
 * coding kernels, out[2] the layout kernel (-1: none yet). */
void zh_debug_blosc_zlib_encode_parts_ms(double out[3]);
int zh_blosc_compress_ex(const void* src, size_t n, const zh_blosc_enc_params* params,
                         unsigned flags, void* dst, size_t cap, size_t* cbytes, char* err,
                         size_t errlen);
int zh_blosc_encode_batch_ex(zh_ctx* ctx, zh_blosc_enc_frame* frames, int64_t n,
                             const zh_blosc_enc_params* params, unsigned flags, void* dst,
                             int64_t dstcap, void* stream, char* err, size_t errlen);

/* ---- host byte-to-byte stage: zstd frames (RFC 8878) ------------------------------
 * Replaces zstd-jni inside ZstdCodec.decode (M/core/codec/core/ZstdCodec.java:14-22) and the
 * zstd compressor of blosc frames (BloscCodec.java; CodecBuilder.withBlosc() defaults to
 * cname "zstd", M/v3/codec/CodecBuilder.java:58-60).  One or more frames (skippable frames
 * skipped); the XXH64 content checksum is verified when a frame carries one; frames that need
 * a dictionary → ZH_EUNSUPPORTED.  dst == NULL: *dstlen = the decoded size (the declared content
 * sizes, or a pass that stores nothing for a frame that declares none).  A frame is decoded by
 * the decoder the device batch below runs (csrc/zh_zstd_dec.h), here on one lane; this call adds
 * the loop over frames, the checksum comparison and the status and text of each reason.  After
 * a failure *dstlen says nothing.
 * zh_zstd_compress_raw writes a valid frame of raw (stored) blocks with the content size and,
 * if asked, the checksum (the write path's encoder; no compression); dst == NULL: the size.
 * zh_xxh64: XXH64 of a buffer (the checksum's hash). */
int zh_zstd_decompress(const void* src, size_t srclen, void* dst, size_t dstcap, size_t* dstlen,
                       char* err, size_t errlen);
int zh_zstd_compress_raw(const void* src, size_t srclen, int checksum, void* dst, size_t dstcap,
                         size_t* dstlen);
uint64_t zh_xxh64(const void* data, size_t len, uint64_t seed);

/* ---- zstd frames written by the library, on the host or on the device ---------------
 * One frame per call / per source, never concatenated frames.  The content is cut into blocks
 * of `blocksize` bytes, each compressed on its own (greedy LZ over a 1024-slot table, raw
 * literals, sequences FSE-coded with the predefined tables, no repeat offsets); a block that
 * would not shrink is a raw block, neighbouring raw blocks are merged up to 128 KiB, and a frame
 * that would reach the size of zh_zstd_compress_raw's is written as that frame, byte for byte.
 * The bytes are a pure function of (input, block size, checksum): the host call and the batch
 * call give the same frame.  The codec's `level` is not honoured. */
typedef struct zh_zstd_enc_params {
  int32_t checksum;   /* 0 / 1: the XXH64 content checksum                              */
  int32_t blocksize;  /* 0: default (16 KiB); below 1 KiB: 1 KiB; above 64 KiB: 64 KiB  */
} zh_zstd_enc_params;

typedef struct zh_zstd_enc_frame {
  const void* src;   /* raw bytes: device memory                               */
  int64_t nbytes;
  int64_t dst_off;   /* out: place of the frame in dst, 16-byte aligned        */
  int64_t cbytes;    /* out: size of the frame                                 */
  int32_t status;    /* out: ZH_OK or this frame's error                       */
} zh_zstd_enc_frame;

/* Host, no device: one frame.  dst == NULL: *len = the bound, the size of the raw-block frame
 * (cap must reach it otherwise). */
int zh_zstd_compress(const void* src, size_t n, const zh_zstd_enc_params* params, void* dst,
                     size_t cap, size_t* len, char* err, size_t errlen);

/* Host memory a batch needs for its frames: the sum of the bounds, each rounded up to 16
 * bytes; or -zh_status. */
int64_t zh_zstd_encode_bound(const zh_zstd_enc_frame* frames, int64_t n,
                             const zh_zstd_enc_params* params);

/* Sources in device memory; the frames arrive in host memory dst (dstcap >= the bound) at
 * dst_off, cbytes long.  One kernel matches (one wavefront per block), a second codes the
 * sequences (one thread per block), a third hashes the content (one wavefront per frame), a
 * fourth lays the frames out; they leave through the context's page-locked ring.  Runs on
 * `stream` (NULL: the context's) and waits.  Slabs of at most 128 MiB of raw bytes (a larger
 * frame is its own slab) bound the device memory of a call. */
int zh_zstd_encode_batch(zh_ctx* ctx, zh_zstd_enc_frame* frames, int64_t n,
                         const zh_zstd_enc_params* params, void* dst, int64_t dstcap,
                         void* stream, char* err, size_t errlen);

/* Diagnostics: milliseconds the kernels of the last successful zh_zstd_encode_batch took, by
 * device events, summed over its slabs (-1: none yet); XXH64 (seed 0) of n device buffers by
 * the batch's hash kernel into out[n] (host). */
double zh_debug_zstd_encode_kernel_ms(void);
int zh_debug_zstd_xxh64(zh_ctx* ctx, const zh_zstd_enc_frame* frames, int64_t n, uint64_t* out);

/* ---- gzip members written by the library, on the host or on the device ---------------
 * One member per call / per source, never concatenated members (RFC 1952; header
 * 1f 8b 08 00 00 00 00 00 00 ff: no name, mtime 0, OS 255).  The content is cut into blocks of
 * `blocksize` bytes, each compressed on its own (greedy LZ over a 1024-slot table, no match
 * reaching before the block) into one byte-aligned segment: a fixed-Huffman DEFLATE block
 * followed by an empty stored block, or, when that is not smaller, a stored block (5 bytes over
 * raw).  The member ends with the final empty fixed block 03 00, the CRC-32 and the size.  With
 * `dynamic` 0 there are no dynamic-Huffman blocks: bytes that LZ alone does not shrink are
 * stored.  With `dynamic` 1 a dynamic-Huffman block (its own length-limited Huffman codes over
 * the block's literals, lengths and distances, followed by the same empty stored block) is the
 * block's segment when it is strictly smaller than both other forms.  No member is larger
 * than 20 + n + 5 * ceil(n / blocksize): the bound, with either value.  The bytes are a pure
 * function of (input, block size, dynamic): the host call and the batch call give the same
 * member.  The codec's `level` is not honoured.  Callers zero the struct before they set a
 * field: a field added later then keeps the behaviour of before. */
typedef struct zh_gzip_enc_params {
  int32_t blocksize;  /* 0: default (16 KiB); below 1 KiB: 1 KiB; above 32 KiB: 32 KiB  */
  int32_t dynamic;    /* 0: stored and fixed segments; 1: dynamic ones too; else ZH_EINVAL */
} zh_gzip_enc_params;

typedef struct zh_gzip_enc_frame {
  const void* src;   /* raw bytes: device memory                               */
  int64_t nbytes;
  int64_t dst_off;   /* out: place of the member in dst, 16-byte aligned       */
  int64_t cbytes;    /* out: size of the member                                */
  int32_t status;    /* out: ZH_OK or this member's error                      */
} zh_gzip_enc_frame;

/* Host, no device: one member.  dst == NULL: *len = the bound (cap must reach it otherwise). */
int zh_gzip_compress(const void* src, size_t n, const zh_gzip_enc_params* params, void* dst,
                     size_t cap, size_t* len, char* err, size_t errlen);

/* CRC-32 (IEEE, the gzip trailer's) with zlib's chaining: zh_crc32(zh_crc32(0, a), b) is the
 * CRC of a || b; data == NULL: 0. */
uint32_t zh_crc32(uint32_t crc, const void* data, size_t len);

/* Host memory a batch needs for its members: the sum of the bounds, each rounded up to 16
 * bytes; or -zh_status. */
int64_t zh_gzip_encode_bound(const zh_gzip_enc_frame* frames, int64_t n,
                             const zh_gzip_enc_params* params);

/* Sources in device memory, at any byte alignment; the members arrive in host memory dst
 * (dstcap >= the bound) at dst_off, cbytes long.  One kernel hashes the whole batch (one
 * workgroup per 64 KiB span; the spans' CRCs are combined on the host), then per slab one
 * kernel matches (one wavefront per block), a second codes literals and matches (one wavefront
 * per block), a third lays the members out; they leave through the context's page-locked ring.
 * Runs on `stream` (NULL: the context's) and waits.  Slabs of at most 128 MiB of raw bytes (a
 * larger source is its own slab) bound the device memory of a call. */
int zh_gzip_encode_batch(zh_ctx* ctx, zh_gzip_enc_frame* frames, int64_t n,
                         const zh_gzip_enc_params* params, void* dst, int64_t dstcap,
                         void* stream, char* err, size_t errlen);

/* Diagnostics: milliseconds the kernels of the last successful zh_gzip_encode_batch took, by
 * device events, summed over its slabs (-1: none yet), and the same per kernel into out[4]:
 * match, coder (with `dynamic` 1: histogram, code construction and coding), CRC-32, gather;
 * CRC-32 of n device buffers by the batch's hash kernel and the host combination into out[n]
 * (host); the code lengths the dynamic form gives `rows` histograms of `nsym` counts each
 * (nsym <= 286, counts <= 2^22, limit 1..15) into lens[rows * nsym]: on the host when ctx is
 * NULL, else one wavefront per row on the device (counts and lens are host memory). */
double zh_debug_gzip_encode_kernel_ms(void);
void zh_debug_gzip_encode_kernel_parts_ms(double out[4]);
int zh_debug_gzip_crc32(zh_ctx* ctx, const zh_gzip_enc_frame* frames, int64_t n, uint32_t* out);
int zh_debug_gzip_code_lengths(zh_ctx* ctx, const uint32_t* counts, int32_t nsym, int32_t limit,
                               int64_t rows, uint8_t* lens);

/* ---- zstd frames decoded on the device, a batch at a time -----------------------------
 * The read side of the batch above, in the shape of zh_blosc_decode_batch.  A stored chunk that
 * is exactly one zstd frame with a Frame_Content_Size, no dictionary and a block chain that ends
 * at its last byte (its checksum included) is decoded on the device: one wavefront per frame
 * runs the block decoder (raw / RLE / compressed blocks; raw, RLE, Huffman and treeless
 * literals; predefined, RLE, FSE and repeat sequence tables) with its tables in LDS, and the
 * content checksum is verified by the hash kernel of zh_zstd_encode_batch.  Everything else
 * (concatenated or skippable frames, no content size, a content size the block headers cannot
 * produce, a header walk that fails) is decoded by zh_zstd_decompress on the host inside the
 * call and copied up.  The decoded frames lie in one device buffer at dst_off. */
typedef struct zh_zstd_frame {
  const void* src;   /* the stored frame, host memory                               */
  int64_t srclen;
  int64_t dst_off;   /* out (plan): offset in the batch destination, 256-B aligned  */
  int64_t nbytes;    /* out (plan): decoded size                                    */
  int32_t where;     /* out (plan): 0 device, 1 host fallback (zh_zstd_decompress into
                        pinned staging, then H2D).  zh_zstd_decode_batch also sets 1 on a
                        frame its kernel refused and zh_zstd_decompress then accepted  */
  int32_t status;    /* out: ZH_OK or this frame's error                            */
} zh_zstd_frame;

/* No device needed: runs zh_zstd_decompress's size query on every frame (its status and text
 * for the first bad frame in batch order; that frame's status field is set), walks the frame
 * and block headers (no entropy decoding), fills dst_off / nbytes / where, and returns the
 * destination bytes or -zh_status. */
int64_t zh_zstd_batch_plan(zh_zstd_frame* frames, int64_t n, char* err, size_t errlen);

/* Plans as above, stages the compressed bytes H2D through the context's pinned ring, decodes on
 * `stream` (NULL: the context's) in slabs of at most 128 MiB of decoded bytes (a larger frame is
 * its own slab), waits, and reports the first failing frame in batch order with
 * zh_zstd_decompress's status and text: the kernel runs the decoder zh_zstd_decompress runs and
 * leaves its reason in the frame's flag; a flagged frame (or a checksum mismatch) goes through
 * zh_zstd_decompress once more, which names the error or, if it accepts the frame, supplies the
 * bytes. dst is device memory of dstcap >= the plan's bytes.  After a
 * failed call dst is undefined; the context stays usable. */
int zh_zstd_decode_batch(zh_ctx* ctx, zh_zstd_frame* frames, int64_t n, void* dst,
                         int64_t dstcap, void* stream, char* err, size_t errlen);

/* Diagnostic: milliseconds the decode and checksum kernels of the last successful
 * zh_zstd_decode_batch in this process took, by device events, summed over its slabs (-1: none
 * yet). */
double zh_debug_zstd_decode_kernel_ms(void);

/* Diagnostic, no device: the blocks of one device-decoded frame as rows of 10 int64: block
 * type (0 raw, 1 RLE, 2 compressed), stored size, decoded size (-1: a compressed block does not
 * say), and for a compressed block the literals type (0 raw, 1 RLE, 2 Huffman, 3 treeless), the
 * number of Huffman streams (0, 1 or 4), the regenerated literals size, the sequence count and
 * the LL / OF / ML table modes (0 predefined, 1 RLE, 2 FSE, 3 repeat); -1 where a field does not
 * apply.  Writes up to `cap` rows to `rows` (may be NULL) and returns their number, or
 * -ZH_EUNSUPPORTED for a frame the plan sends to the host. */
int64_t zh_debug_zstd_blocks(const void* src, size_t srclen, int64_t* rows, int64_t cap,
                             char* err, size_t errlen);

/* ---- gzip members decoded on the host or on the device, a batch at a time ----------------
 * The read side of zh_gzip_encode_batch, in the shape of the zstd batch above.  The decoder
 * (csrc/zh_gzip_dec.h, RFC 1951 / RFC 1952) reads the FIRST member of a buffer and ignores what
 * follows it, as zlib.decompress(b, 31) does: stored, fixed and dynamic blocks; FEXTRA, FNAME,
 * FCOMMENT and FHCRC headers; it accepts and rejects what zlib's inflate accepts and rejects.
 *
 * zh_gzip_decompress: host, no device.  dst == NULL: the size query, a decoding pass that stores
 * nothing (never ISIZE alone).  Otherwise dstcap must hold the content; the CRC-32 and ISIZE are
 * verified.  Errors are ZH_EDATA with zlib's wording behind "gzip: " (e.g. "gzip: invalid
 * distance too far back", "gzip: incorrect data check"); content larger than dstcap is
 * ZH_EINVAL. */
int zh_gzip_decompress(const void* src, size_t srclen, void* dst, size_t dstcap, size_t* dstlen,
                       char* err, size_t errlen);

typedef struct zh_gzip_frame {
  const void* src;   /* the stored member, host memory                              */
  int64_t srclen;
  int64_t dst_off;   /* out (plan): offset in the batch destination, 256-B aligned  */
  int64_t nbytes;    /* out (plan): decoded size                                    */
  int32_t where;     /* out (plan): 0 device, 1 host (zh_gzip_decompress, then H2D).
                        zh_gzip_decode_batch also sets 1 on a member its kernel refused
                        and zh_gzip_decompress then accepted                        */
  int32_t status;    /* out: ZH_OK or this frame's error                            */
  int32_t host_only; /* in: non-zero plans the frame for the host                   */
} zh_gzip_frame;

/* No device needed: walks the gzip header of every frame, no block.  A header error is reported
 * for the first bad frame in batch order with zh_gzip_decompress's status and text (that frame's
 * status field is set).  where = 0 takes nbytes from the frame's last four bytes and requires
 * host_only == 0, at least 2 + 8 bytes behind the header and nbytes <= 1032 x (srclen - header
 * - 8), DEFLATE's largest expansion; every other frame is where = 1 with nbytes from the size
 * query (whose failure is reported the same way).  Returns the destination bytes or
 * -zh_status. */
int64_t zh_gzip_batch_plan(zh_gzip_frame* frames, int64_t n, char* err, size_t errlen);

/* Plans as above, stages the compressed bytes H2D through the context's pinned ring, decodes on
 * `stream` (NULL: the context's) one wavefront per member, in slabs of at most 128 MiB of decoded
 * bytes (a larger member is its own slab), hashes the decoded members with the CRC-32 kernel of
 * zh_gzip_encode_batch, compares with the stored CRC-32 on the host, and waits.  A member the
 * kernel flagged (it also requires the planned nbytes and that the member ends with the frame),
 * or whose CRC-32 differs, goes through zh_gzip_decompress in batch order: a failure is the
 * call's status and text; a success that fits the frame's slot (nbytes rounded up to 256) is
 * copied up, nbytes is corrected and where becomes 1; a success larger than its slot (trailing
 * bytes, or a member over 4 GiB, hid the real ISIZE) sets that frame's status to
 * ZH_EUNSUPPORTED and, unless an error comes first, the call returns ZH_EUNSUPPORTED with
 * "gzip: decoded size exceeds the planned size": plan such frames again with host_only set.
 * dst is device memory of dstcap >= the plan's bytes.  After a failed call dst is undefined;
 * the context stays usable. */
int zh_gzip_decode_batch(zh_ctx* ctx, zh_gzip_frame* frames, int64_t n, void* dst,
                         int64_t dstcap, void* stream, char* err, size_t errlen);

/* Diagnostic: milliseconds the decode and CRC-32 kernels of the last successful
 * zh_gzip_decode_batch in this process took, by device events, summed over its slabs (-1: none
 * yet). */
double zh_debug_gzip_decode_kernel_ms(void);

/* Diagnostic, no device: the DEFLATE blocks of the first member as rows of 9 int64: block type
 * (0 stored, 1 fixed, 2 dynamic), stored bits (header bits included), decoded bytes, the number
 * of literal/length and of distance codes (HLIT + 257 and HDIST + 1; 288 and 32 for a fixed
 * block, -1 for a stored one), the largest literal/length code length, the largest distance
 * code length, the number of distance codes in use, and the largest match distance of the
 * block (0: no match).  Writes up to `cap` rows to `rows` (may be NULL) and returns their
 * number, or -zh_status for a member the decoder rejects. */
int64_t zh_debug_gzip_blocks(const void* src, size_t srclen, int64_t* rows, int64_t cap,
                             char* err, size_t errlen);

/* dst block b ← src block src_block[b] (device buffers, blocks of block_bytes, a multiple of
 * 16; 16-byte aligned; src_block on the host), synchronous: re-lays out encoded shards, e.g.
 * the bench's shuffled inner-chunk order. */
int zh_gather_blocks(zh_ctx* ctx, void* dst, const void* src, int64_t block_bytes,
                     const int64_t* src_block, int64_t n);

/* ---- synthetic data (bench / property tests) -------------------------------------- */
/* dst[i] = low dtype_size bytes of splitmix64((first + i) ^ seed), i in [0, n). */
int zh_synth_fill(zh_ctx* ctx, void* dst, int64_t n, int dtype_size, int64_t first,
                  uint64_t seed, void* stream);
/* Counts elements of the C-order region [offset, offset+shape) of an array of
 * array_shape whose value differs from the synth value at their global index. */
int zh_synth_verify(zh_ctx* ctx, const void* region, int ndim, const int64_t* array_shape,
                    const int64_t* offset, const int64_t* shape, int dtype_size,
                    uint64_t seed, uint64_t* mismatches, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ZARRHIP_H */
