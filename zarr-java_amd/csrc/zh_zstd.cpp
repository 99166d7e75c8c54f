// zh_zstd.cpp — the host side of Zstandard frames (RFC 8878).  zh_zstd_decompress backs the host
// decompression hand-off of the device pipeline: ZstdCodec.decode
// (M/core/codec/core/ZstdCodec.java:14-22, zstd-jni 1.5.x in the reference) and blosc frames whose
// compressor is zstd (BloscCodec.java; withBlosc() defaults to cname "zstd",
// M/v3/codec/CodecBuilder.java:58-60).  The decoded bytes then go to the device `bytes` /
// transpose / scatter stages.
//
// The decoder of a frame is zh_zstd_dec.h, the one the device kernel runs; it is run here on one
// lane.  This file has what surrounds a frame: the loop over concatenated and skippable frames,
// the size query (the declared content sizes, or a pass that stores nothing for a frame that
// declares none), the comparison of the XXH64 content checksum, and the status and text of every
// reason the decoder gives.  Dictionaries are not supported (zarr's zstd codec has none): a frame
// naming one is rejected as unsupported.  The encoder side: zh_zstd_compress is the host form of
// the block writer of zh_zstd_enc.h, whose encoding tables are derived here from the decoder's
// fse_build; zh_zstd_compress_raw writes frames of raw blocks.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "../../include/zarrhip.h"
#include "zh_zstd_dec.h"
#include "zh_zstd_enc.h"

namespace {

void set_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) snprintf(err, errlen, "%s", msg);
}

struct Fail {  // a predefined table that does not invert: the encoder cannot start
  int status;
  const char* msg;
};

[[noreturn]] void fail(const char* msg, int status = ZH_EDATA) { throw Fail{status, msg}; }

uint64_t rd_le64(const uint8_t* p, int n) {
  uint64_t v = 0;
  for (int i = n - 1; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}

// ---- XXH64 (content checksum: low 32 bits of XXH64(content, seed 0)) -----------------
constexpr uint64_t P1 = 11400714785074694791ull, P2 = 14029467366897019727ull,
                   P3 = 1609587929392839161ull, P4 = 9650029242287828579ull,
                   P5 = 2870177450012600261ull;
inline uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t xround(uint64_t acc, uint64_t in) {
  acc += in * P2;
  acc = rotl(acc, 31);
  return acc * P1;
}
inline uint64_t xmerge(uint64_t acc, uint64_t v) {
  acc ^= xround(0, v);
  return acc * P1 + P4;
}

}  // namespace

extern "C" uint64_t zh_xxh64(const void* data, size_t len, uint64_t seed) {
  const uint8_t* p = (const uint8_t*)data;
  const uint8_t* end = p + len;
  uint64_t h;
  if (len >= 32) {
    uint64_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
    const uint8_t* lim = end - 32;
    do {
      v1 = xround(v1, rd_le64(p, 8));
      v2 = xround(v2, rd_le64(p + 8, 8));
      v3 = xround(v3, rd_le64(p + 16, 8));
      v4 = xround(v4, rd_le64(p + 24, 8));
      p += 32;
    } while (p <= lim);
    h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    h = xmerge(h, v1);
    h = xmerge(h, v2);
    h = xmerge(h, v3);
    h = xmerge(h, v4);
  } else {
    h = seed + P5;
  }
  h += (uint64_t)len;
  while (p + 8 <= end) {
    h ^= xround(0, rd_le64(p, 8));
    h = rotl(h, 27) * P1 + P4;
    p += 8;
  }
  if (p + 4 <= end) {
    h ^= rd_le64(p, 4) * P1;
    h = rotl(h, 23) * P2 + P3;
    p += 4;
  }
  while (p < end) {
    h ^= (*p++) * P5;
    h = rotl(h, 11) * P1;
  }
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

namespace {

// ---- the encoder's view of the predefined tables ---------------------------------------
// For a symbol s, the decode-table states carrying s partition the next-state range: state S
// covers [base[S], base[S] + 2^nbits[S]).  So (s, next state) names one state.
template <int NSYM, int SIZE>
void fill_enc(const int16_t* dflt, int log, uint8_t (*state)[SIZE], uint8_t* first, uint8_t* nb,
              uint16_t* base) {
  int16_t norm[NSYM];
  uint32_t tab[SIZE];  // the decoder's table: symbol | nbits << 8 | base << 16
  for (int s = 0; s < NSYM; s++) norm[s] = dflt[s];
  if (zh_zd::fse_build(tab, norm, NSYM, log)) fail("zstd: FSE table spread does not close");
  for (int s = 0; s < NSYM; s++) {
    first[s] = 0xFF;
    for (int n = 0; n < SIZE; n++) state[s][n] = 0xFF;
  }
  for (int S = 0; S < SIZE; S++) {
    const int s = tab[S] & 0xFF;
    nb[S] = (uint8_t)(tab[S] >> 8);
    base[S] = (uint16_t)(tab[S] >> 16);
    if (first[s] == 0xFF) first[s] = (uint8_t)S;
    for (int n = base[S]; n < base[S] + (1 << nb[S]); n++) {
      if (state[s][n] != 0xFF) fail("zstd: predefined table states overlap");
      state[s][n] = (uint8_t)S;
    }
  }
  for (int s = 0; s < NSYM; s++)
    for (int n = 0; n < SIZE; n++)
      if (state[s][n] == 0xFF) fail("zstd: predefined table leaves a next state uncovered");
}

zh_ze::Tables make_enc_tables() {
  zh_ze::Tables T;
  memset(&T, 0, sizeof T);
  using namespace zh_zd;
  fill_enc<36, 64>(kLLDefault, 6, T.ll_state, T.ll_first, T.ll_nb, T.ll_base);
  fill_enc<53, 64>(kMLDefault, 6, T.ml_state, T.ml_first, T.ml_nb, T.ml_base);
  fill_enc<29, 32>(kOFDefault, 5, T.of_state, T.of_first, T.of_nb, T.of_base);
  for (int c = 0; c < 36; c++) T.ll_cbase[c] = kLLBase[c], T.ll_cbits[c] = kLLBits[c];
  for (int c = 0; c < 53; c++) T.ml_cbase[c] = kMLBase[c], T.ml_cbits[c] = kMLBits[c];
  for (uint32_t v = 0, c = 0; v < 64; v++) {
    while (c + 1 < 36 && kLLBase[c + 1] <= v) c++;
    T.ll_code[v] = (uint8_t)c;
  }
  for (uint32_t v = 0, c = 0; v < 128; v++) {  // v = match length - 3
    while (c + 1 < 53 && kMLBase[c + 1] <= v + 3) c++;
    T.ml_code[v] = (uint8_t)c;
  }
  return T;
}

// ---- frames --------------------------------------------------------------------------------
// The status and text of every reason zh_zstd_dec.h rejects a frame for.
struct Text {
  zh_zd::Verdict why;
  int status;
  const char* msg;
};
const Text& text_of(zh_zd::Verdict v) {
  using namespace zh_zd;
  static const Text T[] = {
    {kBadMagic, ZH_EDATA, "zstd: unknown frame magic"},
    {kHeaderTruncated, ZH_EDATA, "zstd: frame header truncated"},
    {kReservedHeaderBit, ZH_EDATA, "zstd: reserved frame header bit set"},
    {kDictionary, ZH_EUNSUPPORTED, "zstd: frames that need a dictionary are not supported"},
    {kBlockHeaderTruncated, ZH_EDATA, "zstd: block header truncated"},
    {kReservedBlockType, ZH_EDATA, "zstd: reserved block type"},
    {kBlockTruncated, ZH_EDATA, "zstd: block truncated"},
    {kBlockTooLarge, ZH_EDATA, "zstd: block larger than 128 KiB"},
    {kNoRoom, ZH_EINVAL, "zstd: decoded data exceeds the output buffer"},
    {kSizeMismatch, ZH_EDATA, "zstd: frame content size mismatch"},
    {kChecksumTruncated, ZH_EDATA, "zstd: content checksum truncated"},
    {kTrailingBytes, ZH_EDATA, "zstd: trailing bytes after the last frame"},
    {kSkippableTruncated, ZH_EDATA, "zstd: skippable frame truncated"},
    {kNoFrame, ZH_EDATA, "zstd: no frame"},
    {kChecksumMismatch, ZH_EDATA, "zstd: content checksum mismatch"},
    {kEmptyBlock, ZH_EDATA, "zstd: empty compressed block"},
    {kLitHeaderTruncated, ZH_EDATA, "zstd: literals header truncated"},
    {kRawLitTruncated, ZH_EDATA, "zstd: raw literals truncated"},
    {kRleLitTruncated, ZH_EDATA, "zstd: RLE literals truncated"},
    {kLitTruncated, ZH_EDATA, "zstd: compressed literals truncated"},
    {kNoHufTable, ZH_EDATA, "zstd: treeless literals without a previous Huffman table"},
    {kNoMemory, ZH_ENOMEM, "zstd: out of memory"},
    {kJumpTruncated, ZH_EDATA, "zstd: literals jump table truncated"},
    {kStreamsTruncated, ZH_EDATA, "zstd: literals streams truncated"},
    {kFourStreamsShort, ZH_EDATA, "zstd: literals too short for four streams"},
    {kEmptyBitstream, ZH_EDATA, "zstd: empty bitstream"},
    {kNoEndMarker, ZH_EDATA, "zstd: bitstream without its end marker"},
    {kHufStreamInexact, ZH_EDATA, "zstd: Huffman stream not consumed exactly"},
    {kNoTree, ZH_EDATA, "zstd: missing Huffman tree description"},
    {kWeightsTruncated, ZH_EDATA, "zstd: Huffman weights truncated"},
    {kWeightStreamEmpty, ZH_EDATA, "zstd: Huffman weight stream empty"},
    {kTooManyWeights, ZH_EDATA, "zstd: too many Huffman weights"},
    {kTooManySymbols, ZH_EDATA, "zstd: too many Huffman symbols"},
    {kWeightTooLarge, ZH_EDATA, "zstd: Huffman weight too large"},
    {kWeightsZero, ZH_EDATA, "zstd: Huffman weights all zero"},
    {kTreeIncomplete, ZH_EDATA, "zstd: Huffman weights do not complete a tree"},
    {kTreeTooDeep, ZH_EDATA, "zstd: Huffman tree too deep"},
    {kCodeSpace, ZH_EDATA, "zstd: Huffman code space not filled"},
    {kTableOverrun, ZH_EDATA, "zstd: table description overruns its section"},
    {kAccuracyLog, ZH_EDATA, "zstd: FSE accuracy log too large"},
    {kFseSum, ZH_EDATA, "zstd: FSE probabilities do not sum to the table size"},
    {kFseSpread, ZH_EDATA, "zstd: FSE table spread does not close"},
    {kNoSequences, ZH_EDATA, "zstd: sequences section missing"},
    {kCountTruncated, ZH_EDATA, "zstd: sequence count truncated"},
    {kNoModes, ZH_EDATA, "zstd: sequence modes missing"},
    {kReservedModes, ZH_EDATA, "zstd: reserved bits set in the sequence modes"},
    {kRleTableTruncated, ZH_EDATA, "zstd: RLE sequence table truncated"},
    {kRleCode, ZH_EDATA, "zstd: RLE sequence code out of range"},
    {kNoRepeatTable, ZH_EDATA, "zstd: repeat sequence table without a previous table"},
    {kSequenceCode, ZH_EDATA, "zstd: sequence code out of range"},
    {kPastLiterals, ZH_EDATA, "zstd: sequence reads past the literals"},
    {kOffset, ZH_EDATA, "zstd: match offset before the frame"},
    {kSeqStreamInexact, ZH_EDATA, "zstd: sequence bitstream not consumed exactly"},
  };
  static_assert(sizeof T / sizeof T[0] == kVerdicts - 1, "a reason without a text");
  for (const Text& t : T)
    if (t.why == v) return t;
  return T[0];  // not reached: every reason has its row
}

// The size of a frame that declares it (the size query): the block headers alone.
zh_zd::Verdict skip_frame(const uint8_t* src, size_t len, const zh_zd::Header& h, size_t* used) {
  size_t p = h.size;
  for (;;) {
    if (len - p < 3) return zh_zd::kBlockHeaderTruncated;
    const uint32_t bh = zh_zd::rd_le(src + p, 3);
    p += 3;
    if (((bh >> 1) & 3) == 3) return zh_zd::kReservedBlockType;
    const size_t stored = ((bh >> 1) & 3) == 1 ? 1 : bh >> 3;
    if (stored > len - p) return zh_zd::kBlockTruncated;
    p += stored;
    if (bh & 1) break;
  }
  if (h.csum) {
    if (len - p < 4) return zh_zd::kChecksumTruncated;
    p += 4;
  }
  *used = p;
  return zh_zd::kOk;
}

// Working memory of one zh_zstd_decompress call: the tables and the Huffman literals of a block.
struct Scratch {
  zh_zd::Work work;
  uint8_t lit[zh_zd::kMaxRegen];
};

// Frame after frame of [s, s+n) into dst (null: count only); *total: the bytes of the frames
// that were accepted.
zh_zd::Verdict run(const uint8_t* s, size_t n, uint8_t* dst, size_t cap, size_t* total) {
  using namespace zh_zd;
  std::unique_ptr<Scratch> sc;
  size_t p = 0;
  int frames = 0;
  *total = 0;
  while (p < n) {
    if (n - p < 4) return kTrailingBytes;
    const uint32_t magic = rd_le(s + p, 4);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {  // skippable frame
      if (n - p < 8 || rd_le(s + p + 4, 4) > n - p - 8) return kSkippableTruncated;
      p += 8 + (size_t)rd_le(s + p + 4, 4);
      continue;
    }
    if (magic != kMagic) return kBadMagic;
    Header h;
    size_t used = 0;
    uint64_t made = 0;
    Verdict v = frame_header(s + p, n - p, &h);
    if (v) return v;
    if (!dst && h.fcs >= 0) {  // size query: the header says it all
      v = skip_frame(s + p, n - p, h, &used);
      made = (uint64_t)h.fcs;
    } else {
      if (!sc) sc.reset(new (std::nothrow) Scratch);
      if (!sc) return kNoMemory;
      if (dst) {
        SerialLanes lanes;
        v = decode_frame(s + p, n - p, dst + *total, cap - *total, sc->lit, sizeof sc->lit,
                         sc->work, lanes, &made, &used, &h);
        if (!v && h.csum &&
            rd_le(s + p + used - 4, 4) != (uint32_t)zh_xxh64(dst + *total, (size_t)made, 0))
          v = kChecksumMismatch;
      } else {
        CountLanes lanes;
        uint8_t nowhere;
        v = decode_frame(s + p, n - p, &nowhere, SIZE_MAX - *total, sc->lit, sizeof sc->lit,
                         sc->work, lanes, &made, &used, &h);
      }
    }
    if (v) return v;
    *total += (size_t)made;
    p += used;
    frames++;
  }
  return frames ? kOk : kNoFrame;
}

}  // namespace

const zh_ze::Tables& zh_ze::tables() {
  static const zh_ze::Tables T = make_enc_tables();
  return T;
}

extern "C" {

// One compressed frame on the host (zh_zstd_enc.h over HostLanes): the device batch's oracle.
int zh_zstd_compress(const void* src, size_t n, const zh_zstd_enc_params* params, void* dst,
                     size_t cap, size_t* len, char* err, size_t errlen) {
  const char* msg = "";
  try {
    const int st = zh_ze::compress_frame(zh_ze::tables(), (const uint8_t*)src, n, params,
                                         (uint8_t*)dst, cap, len, &msg);
    if (st != ZH_OK) set_err(err, errlen, msg);
    return st;
  } catch (const Fail& f) {
    set_err(err, errlen, f.msg);
    return f.status;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, "zstd: out of memory");
    return ZH_ENOMEM;
  }
}

// Size query (dst == NULL): the sum of the frames' declared content sizes, or, when a frame
// omits its size, a full decode pass without output.  Decode: dstcap must hold the content.
int zh_zstd_decompress(const void* src, size_t srclen, void* dst, size_t dstcap, size_t* dstlen,
                       char* err, size_t errlen) {
  if (!src || !dstlen) return ZH_EINVAL;
  const zh_zd::Verdict v = run((const uint8_t*)src, srclen, (uint8_t*)dst, dstcap, dstlen);
  if (v) set_err(err, errlen, text_of(v).msg);
  return v ? text_of(v).status : ZH_OK;
}

// A frame of raw blocks (no compression): content size in the header, XXH64 checksum when
// `checksum` is set.  dst NULL: returns the frame size in *dstlen.
int zh_zstd_compress_raw(const void* src, size_t srclen, int checksum, void* dst, size_t dstcap,
                         size_t* dstlen) {
  if (!dstlen || (!src && srclen)) return ZH_EINVAL;
  const size_t maxb = (size_t)128 << 10;
  const size_t nblk = srclen == 0 ? 1 : (srclen + maxb - 1) / maxb;
  const size_t need = 4 + 1 + 8 + nblk * 3 + srclen + (checksum ? 4 : 0);
  *dstlen = need;
  if (!dst) return ZH_OK;
  if (dstcap < need) return ZH_EINVAL;
  uint8_t* d = (uint8_t*)dst;
  size_t p = 0;
  auto put = [&](uint64_t v, int n) {
    for (int i = 0; i < n; i++) d[p++] = (uint8_t)(v >> (8 * i));
  };
  put(zh_zd::kMagic, 4);
  put((3u << 6) | (1u << 5) | (checksum ? 4u : 0u), 1);  // 8-byte FCS, single segment
  put(srclen, 8);
  for (size_t k = 0; k < nblk; k++) {
    const size_t o = k * maxb, b = srclen - o < maxb ? srclen - o : maxb;
    put(((uint32_t)b << 3) | (k + 1 == nblk ? 1u : 0u), 3);  // raw block
    if (b) memcpy(d + p, (const uint8_t*)src + o, b);
    p += b;
  }
  if (checksum) put((uint32_t)zh_xxh64(src, srclen, 0), 4);
  return ZH_OK;
}

}  // extern "C"
