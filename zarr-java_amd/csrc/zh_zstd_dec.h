// zh_zstd_dec.h — the zstd frame decoder (RFC 8878), written from the format specification: the
// only one in the library.  zh_zstd_decompress (zh_zstd.cpp) runs it on the host, one lane, frame
// after frame; the batched device read (zh_zstd_dec_kernels.hip) runs it with a wave per frame.
// It decodes ONE frame without a dictionary: raw, RLE and compressed blocks; raw / RLE / Huffman
// (1 or 4 streams, direct or FSE-compressed weights) / treeless literals; sequence counts of 1, 2
// and 3 bytes; predefined / RLE / FSE / repeat tables; repeat offsets; matches that reach back
// anywhere in the frame (the window descriptor is ignored).  A frame without a
// Frame_Content_Size decodes into whatever room the caller has.  Skippable and concatenated
// frames, the comparison of the checksum and the text of an error are the caller's.
//
// Every step returns a Verdict: kOk, or the reason for rejecting the frame.  Where a frame has
// two faults the order of the checks decides which is reported; zh_zstd_decompress's callers
// and tests/golden/zstd_verdicts.txt depend on that order.
//
// The templates are parameterised on a lane policy P:
//     static const uint32_t W        lanes that share the frame (1 on the host, 64 in a wave)
//     uint32_t lane()                this lane, < W
//     bool     first()               lane() == 0: runs the serial steps
//     void     order()               what this wave stored before is visible to its later loads
//     bool     all(bool)             true when true in every lane
//     void     copy(d, s, n)         d[k] = s[k]                  (across the lanes)
//     void     fill(d, byte, n)      d[k] = byte
//     void     match(d, o, off, n)   d[o+k] = d[o-off + k % off]  (off <= o; only bytes below o
//                                    are read: the argument of zh_blosc_kernels.hip's WaveCopy)
// Control flow is uniform over the lanes except where a loop starts at lane().  A serial step
// (table descriptions, FSE spreading) runs on the first lane, leaves its result and its verdict
// in Work (LDS on the device) and is followed by order(); parallel steps (Huffman table fill,
// the four literal streams on four lanes, every copy) stride by W.
//
// The frames are untrusted.  Every loop is bounded by a count from a checked header (nseq,
// regen, a table size, csize) or consumes input bits each turn; every read is checked against
// the block / section it belongs to and every write against the room in the destination or the
// literal scratch.  Reading a backwards bitstream past its start yields zero bits; the streams'
// exact-consumption checks then reject the block.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZH_ZD_HD __host__ __device__ inline
#else
#define ZH_ZD_HD inline
#endif

namespace zh_zd {

constexpr uint32_t kMagic = 0xFD2FB528u;
constexpr uint32_t kMaxBlock = 128u << 10;
constexpr int kMaxHufBits = 11;
constexpr uint32_t kMaxRegen = 1u << 18;  // Huffman literals of one block: an 18-bit field

// Why a frame is rejected.  zh_zstd.cpp has the status and text of each.
enum Verdict : int32_t {
  kOk = 0,
  kBadMagic, kHeaderTruncated, kReservedHeaderBit, kDictionary,
  kBlockHeaderTruncated, kReservedBlockType, kBlockTruncated, kBlockTooLarge, kNoRoom,
  kSizeMismatch, kChecksumTruncated,
  kEmptyBlock, kLitHeaderTruncated, kRawLitTruncated, kRleLitTruncated, kLitTruncated,
  kNoHufTable, kNoMemory, kJumpTruncated, kStreamsTruncated, kFourStreamsShort,
  kEmptyBitstream, kNoEndMarker, kHufStreamInexact,
  kNoTree, kWeightsTruncated, kWeightStreamEmpty, kTooManyWeights, kTooManySymbols,
  kWeightTooLarge, kWeightsZero, kTreeIncomplete, kTreeTooDeep, kCodeSpace,
  kTableOverrun, kAccuracyLog, kFseSum, kFseSpread,
  kNoSequences, kCountTruncated, kNoModes, kReservedModes, kRleTableTruncated, kRleCode,
  kNoRepeatTable, kSequenceCode, kPastLiterals, kOffset, kSeqStreamInexact,
  // the callers': what surrounds a frame, and its checksum
  kTrailingBytes, kSkippableTruncated, kNoFrame, kChecksumMismatch,
  kVerdicts
};

constexpr uint32_t kLLBase[36] = {0,  1,  2,   3,   4,   5,    6,    7,    8,    9,     10,    11,
                                  12, 13, 14,  15,  16,  18,   20,   22,   24,   28,    32,    40,
                                  48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
constexpr uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,  0,  0,  1,  1,
                                 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr uint32_t kMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10,  11,  12,   13,   14,   15,   16,
                                  17, 18, 19, 20, 21, 22, 23, 24,  25,  26,   27,   28,   29,   30,
                                  31, 32, 33, 34, 35, 37, 39, 41,  43,  47,   51,   59,   67,   83,
                                  99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
constexpr uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1,
                                 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr int16_t kLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                    2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int16_t kMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
constexpr int16_t kOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

// Per-frame working memory: the tables a later block may reuse, and what the serial steps hand
// to the other lanes.  FSE entry: symbol | nbits << 8 | base << 16; Huffman: symbol | nbits << 8.
struct Work {
  union {
    uint16_t huf[1 << kMaxHufBits];
    struct {  // while a tree description is read the previous table is dead
      int16_t norm[256];
      uint32_t tab[64];
    } wt;
  };
  uint32_t ll[512], ml[512], of[256];
  uint8_t w[256];      // Huffman weights, then code lengths
  uint8_t order[256];  // symbols sorted by (code length descending, symbol)
  int16_t norm[64];    // probabilities of a sequence table
  uint32_t cnt[16];    // symbols per code length
  uint32_t start[16];  // first rank of each length, longest codes first
  int32_t huf_bits, ll_log, ml_log, of_log;  // 0 / -1: no table yet
  uint32_t used;                             // bytes the last description took
  int32_t verdict;                           // of the last serial step
};

ZH_ZD_HD int highbit(uint64_t v) {  // index of the highest set bit (v > 0)
  int r = 0;
  while (v >>= 1) r++;
  return r;
}
ZH_ZD_HD uint32_t rd_le(const uint8_t* p, int n) {  // n <= 4
  uint32_t v = 0;
  for (int i = n - 1; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}

// ---- frame header ------------------------------------------------------------------------------
struct Header {
  uint32_t size;    // bytes up to the first block header
  int64_t fcs;      // -1: none
  int csum;         // checksum flag
};
// A content size of 2^63 or more reads as none.
ZH_ZD_HD Verdict frame_header(const uint8_t* src, size_t len, Header* h) {
  if (len < 5) return kHeaderTruncated;
  if (rd_le(src, 4) != kMagic) return kBadMagic;
  const uint32_t fhd = src[4];
  const int fcs_flag = (int)(fhd >> 6), single = (fhd >> 5) & 1, did_flag = fhd & 3;
  if (fhd & 0x08) return kReservedHeaderBit;
  size_t p = 5 + (single ? 0 : 1);
  const int did = did_flag == 3 ? 4 : did_flag;
  if (p + (size_t)did > len) return kHeaderTruncated;
  if (did && rd_le(src + p, did) != 0) return kDictionary;
  p += (size_t)did;
  const int fs = fcs_flag == 0 ? single : (fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8);
  if (p + (size_t)fs > len) return kHeaderTruncated;
  h->fcs = -1;
  if (fs) {
    uint64_t v = rd_le(src + p, fs > 4 ? 4 : fs);
    if (fs == 8) v |= (uint64_t)rd_le(src + p + 4, 4) << 32;
    if (fs == 2) v += 256;
    h->fcs = (int64_t)v < 0 ? -1 : (int64_t)v;
  }
  h->csum = (fhd >> 2) & 1;
  h->size = (uint32_t)(p + (size_t)fs);
  return kOk;
}

// Literals header of a compressed block.
struct LitHeader {
  uint32_t type, streams, regen, csize, hsz;
};
ZH_ZD_HD Verdict literals_header(const uint8_t* src, uint32_t len, LitHeader* l) {
  if (len < 1) return kEmptyBlock;
  l->type = src[0] & 3;
  const uint32_t sf = (src[0] >> 2) & 3;
  l->streams = 0;
  l->csize = 0;
  if (l->type <= 1) {
    l->hsz = sf == 1 ? 2 : sf == 3 ? 3 : 1;
    if (len < l->hsz) return kLitHeaderTruncated;
    l->regen = l->hsz == 1 ? (uint32_t)src[0] >> 3 : rd_le(src, (int)l->hsz) >> 4;
    return kOk;
  }
  l->streams = sf == 0 ? 1 : 4;
  l->hsz = sf <= 1 ? 3 : sf + 2;
  if (len < l->hsz) return kLitHeaderTruncated;
  const uint64_t h = (uint64_t)rd_le(src, 4 < l->hsz ? 4 : (int)l->hsz) |
                     (l->hsz == 5 ? (uint64_t)src[4] << 32 : 0);
  const int nb = sf <= 1 ? 10 : sf == 2 ? 14 : 18;
  l->regen = (uint32_t)(h >> 4) & ((1u << nb) - 1);
  l->csize = (uint32_t)(h >> (4 + nb)) & ((1u << nb) - 1);
  return kOk;
}

// ---- bit streams -------------------------------------------------------------------------------
// Forward, LSB first (FSE table descriptions); `bad` once a read ran past the section.
struct FwdBits {
  const uint8_t* p;
  size_t len, bit;
  bool bad;
  ZH_ZD_HD uint32_t read(int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; i++, bit++) {
      if (bit / 8 >= len) {
        bad = true;
        return 0;
      }
      v |= (uint32_t)((p[bit / 8] >> (bit % 8)) & 1) << i;
    }
    return v;
  }
};

// Backward: read from the end, below the end marker (the last byte's highest set bit).  Bytes
// below the stream's start read as zero.  A 64-bit container is refilled from at most 8 bytes.
struct BackBits {
  const uint8_t* p;
  int64_t len, off, cbase;  // off: bits left above position 0; container = bits [cbase, cbase+64)
  uint64_t cont;
  ZH_ZD_HD Verdict init(const uint8_t* src, size_t n) {
    p = src;
    len = (int64_t)n;
    if (n == 0) return kEmptyBitstream;
    if (src[n - 1] == 0) return kNoEndMarker;
    off = (int64_t)n * 8 - (8 - highbit(src[n - 1]));
    cbase = off + 1;  // forces the first refill
    cont = 0;
    return kOk;
  }
  // Always inline: left to itself the host compiler calls it, six times a sequence, with the
  // container in memory.
  __attribute__((always_inline)) ZH_ZD_HD uint64_t read(int n) {  // n <= 32
    if (n == 0) return 0;
    off -= n;
    if (off < cbase) {
      cbase = ((off + n + 7) & ~(int64_t)7) - 64;  // cbase + 39 <= off + n + 7 - 25: holds n bits
      const int64_t b0 = cbase >> 3;               // arithmetic shift: cbase is a multiple of 8
      if (b0 >= 0 && b0 + 8 <= len) {  // inside the stream: one load (little-endian on both sides)
        __builtin_memcpy(&cont, p + b0, 8);
      } else {
        cont = 0;
        for (int i = 0; i < 8; i++) {
          const int64_t b = b0 + i;
          if (b >= 0 && b < len) cont |= (uint64_t)p[b] << (8 * i);
        }
      }
    }
    return (cont >> (off - cbase)) & ((1ull << n) - 1);
  }
};

// ---- FSE ---------------------------------------------------------------------------------------
// Serial.  norm[0..nsym) is consumed (it becomes the per-symbol state counter).
ZH_ZD_HD Verdict fse_build(uint32_t* tab, int16_t* norm, int nsym, int acc) {
  const int size = 1 << acc;
  int high = size;
  for (int s = 0; s < nsym; s++)
    if (norm[s] == -1) {
      tab[--high] = (uint32_t)s;
      norm[s] = 1;
    } else if (norm[s] > 0) {
      norm[s] = (int16_t)-norm[s];  // still to be spread
    }
  const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
  int pos = 0;
  for (int s = 0; s < nsym; s++) {
    if (norm[s] >= 0) continue;
    const int cnt = -norm[s];
    norm[s] = (int16_t)cnt;
    for (int i = 0; i < cnt; i++) {
      tab[pos] = (uint32_t)s;
      do pos = (pos + step) & mask;
      while (pos >= high);
    }
  }
  if (pos != 0) return kFseSpread;
  for (int i = 0; i < size; i++) {
    const uint32_t s = tab[i];
    const uint32_t d = (uint32_t)(uint16_t)norm[s]++;
    const uint32_t nb = (uint32_t)(acc - highbit(d));
    tab[i] = s | (nb << 8) | ((((d << nb) - (uint32_t)size) & 0xFFFFu) << 16);
  }
  return kOk;
}

// Serial.  A table description into norm / tab; *used: the bytes it took.
ZH_ZD_HD Verdict fse_read(const uint8_t* src, size_t len, int max_log, int max_sym, int16_t* norm,
                          uint32_t* tab, int* log, size_t* used) {
  FwdBits in{src, len, 0, false};
  const int acc = 5 + (int)in.read(4);
  if (in.bad) return kTableOverrun;
  if (acc > max_log) return kAccuracyLog;
  int remaining = 1 << acc, s = 0;
  while (remaining > 0 && s < max_sym) {
    const int bits = highbit((uint64_t)remaining + 1) + 1;
    uint32_t val = in.read(bits);
    if (in.bad) return kTableOverrun;
    const uint32_t lower = (1u << (bits - 1)) - 1;
    const uint32_t threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
    if ((val & lower) < threshold) {
      in.bit -= 1;
      val &= lower;
    } else if (val > lower) {
      val -= threshold;
    }
    const int proba = (int)val - 1;
    remaining -= proba < 0 ? -proba : proba;
    norm[s++] = (int16_t)proba;
    if (proba == 0) {
      int rep = (int)in.read(2);
      for (;;) {  // two input bits per turn
        if (in.bad) return kTableOverrun;
        for (int i = 0; i < rep && s < max_sym; i++) norm[s++] = 0;
        if (rep != 3) break;
        rep = (int)in.read(2);
      }
    }
  }
  if (remaining != 0) return kFseSum;
  if (fse_build(tab, norm, s, acc)) return kFseSpread;
  *log = acc;
  *used = (in.bit + 7) / 8;
  return kOk;
}

// ---- Huffman -----------------------------------------------------------------------------------
// Serial.  The tree description at src: weights -> code lengths (W.w), symbols per length
// (W.cnt), symbols in table order (W.order), W.huf_bits, W.used.
ZH_ZD_HD Verdict huf_read_tree(const uint8_t* src, size_t len, Work& W) {
  W.huf_bits = 0;
  if (len < 1) return kNoTree;
  const uint32_t hb = src[0];
  int n = 0;
  if (hb >= 128) {  // direct 4-bit weights
    n = (int)hb - 127;
    const size_t nb = ((size_t)n + 1) / 2;
    if (1 + nb > len) return kWeightsTruncated;
    for (int i = 0; i < n; i++)
      W.w[i] = (uint8_t)(i % 2 == 0 ? src[1 + i / 2] >> 4 : src[1 + i / 2] & 15);
    W.used = (uint32_t)(1 + nb);
  } else {  // FSE-compressed weights: two interleaved states
    const size_t cs = hb;
    if (1 + cs > len || cs == 0) return kWeightsTruncated;
    int log = 0;
    size_t hl = 0;
    Verdict v = fse_read(src + 1, cs, 6, 256, W.wt.norm, W.wt.tab, &log, &hl);
    if (v) return v;
    if (hl >= cs) return kWeightStreamEmpty;
    BackBits b;
    v = b.init(src + 1 + hl, cs - hl);
    if (v) return v;
    uint32_t s1 = (uint32_t)b.read(log), s2 = (uint32_t)b.read(log);
    for (;;) {  // every turn stores a weight: at most 255
      if (n >= 255) return kTooManyWeights;
      W.w[n++] = (uint8_t)W.wt.tab[s1];
      s1 = (W.wt.tab[s1] >> 16) + (uint32_t)b.read((int)((W.wt.tab[s1] >> 8) & 0xFF));
      if (b.off < 0) {
        W.w[n++] = (uint8_t)W.wt.tab[s2];
        break;
      }
      if (n >= 255) return kTooManyWeights;
      W.w[n++] = (uint8_t)W.wt.tab[s2];
      s2 = (W.wt.tab[s2] >> 16) + (uint32_t)b.read((int)((W.wt.tab[s2] >> 8) & 0xFF));
      if (b.off < 0) {
        if (n >= 255) return kTooManyWeights;
        W.w[n++] = (uint8_t)W.wt.tab[s1];
        break;
      }
    }
    W.used = (uint32_t)(1 + cs);
  }
  // n transmitted weights; the last is implied
  if (n + 1 > 256) return kTooManySymbols;
  uint64_t sum = 0;
  for (int i = 0; i < n; i++) {
    if (W.w[i] > kMaxHufBits) return kWeightTooLarge;
    sum += W.w[i] ? (1ull << (W.w[i] - 1)) : 0;
  }
  if (sum == 0) return kWeightsZero;
  const int mb = highbit(sum) + 1;
  const uint64_t left = (1ull << mb) - sum;
  if (left & (left - 1)) return kTreeIncomplete;
  if (mb > kMaxHufBits) return kTreeTooDeep;
  for (int i = 0; i < n; i++) W.w[i] = W.w[i] ? (uint8_t)(mb + 1 - W.w[i]) : 0;
  W.w[n] = (uint8_t)(mb + 1 - (highbit(left) + 1));
  const int ns = n + 1;
  int max_bits = 0;
  for (int i = 0; i < 16; i++) W.cnt[i] = 0;
  for (int i = 0; i < ns; i++) {
    max_bits = W.w[i] > max_bits ? W.w[i] : max_bits;
    W.cnt[W.w[i]]++;
  }
  uint32_t cells = 0, rank = 0;
  for (int i = max_bits; i >= 1; i--) {
    W.start[i] = rank;
    rank += W.cnt[i];
    cells += W.cnt[i] << (max_bits - i);
  }
  if (cells != (1u << max_bits)) return kCodeSpace;
  for (int i = 0; i < ns; i++)
    if (W.w[i]) W.order[W.start[W.w[i]]++] = (uint8_t)i;
  W.huf_bits = max_bits;
  return kOk;
}

// Parallel: the decoding table from cnt / order.
template <class P>
ZH_ZD_HD void huf_fill(Work& W, P& p) {
  const int mb = W.huf_bits;
  uint32_t cell = 0, rank = 0;
  for (int i = mb; i >= 1; i--) {
    const uint32_t c = W.cnt[i], sh = (uint32_t)(mb - i), n = c << sh;
    for (uint32_t k = p.lane(); k < n; k += P::W)
      W.huf[cell + k] = (uint16_t)(W.order[rank + (k >> sh)] | ((uint32_t)i << 8));
    cell += n;
    rank += c;
  }
}

// One lane: a stream of nout literals.
ZH_ZD_HD Verdict huf_stream(const Work& W, const uint8_t* src, size_t len, uint8_t* out,
                            size_t nout) {
  BackBits b;
  const Verdict v = b.init(src, len);
  if (v) return v;
  const int mb = W.huf_bits;
  uint32_t st = (uint32_t)b.read(mb);
  const uint32_t mask = (1u << mb) - 1;
  for (size_t i = 0; i < nout; i++) {
    const uint32_t e = W.huf[st];
    out[i] = (uint8_t)e;
    const int nb = (int)(e >> 8);
    st = ((st << nb) + (uint32_t)b.read(nb)) & mask;
  }
  return b.off == -(int64_t)mb ? kOk : kHufStreamInexact;
}

// ---- sequences ---------------------------------------------------------------------------------
// Serial.  One of the three tables by its mode; W.used: the bytes the mode took.
ZH_ZD_HD Verdict seq_table(uint32_t* tab, int32_t* log, int mode, const uint8_t* p, size_t len,
                           const int16_t* dflt, int ndflt, int dlog, int max_log, int max_sym,
                           Work& W) {
  W.used = 0;
  if (mode == 0) {
    for (int i = 0; i < ndflt; i++) W.norm[i] = dflt[i];
    *log = dlog;
    return fse_build(tab, W.norm, ndflt, dlog);
  }
  if (mode == 1) {
    if (len < 1) return kRleTableTruncated;
    if (p[0] >= max_sym) return kRleCode;
    tab[0] = p[0];
    *log = 0;
    W.used = 1;
    return kOk;
  }
  if (mode == 2) {
    int lg = -1;
    *log = -1;  // a failed description leaves no table
    size_t u = 0;
    const Verdict v = fse_read(p, len, max_log, max_sym, W.norm, tab, &lg, &u);
    if (v) return v;
    *log = lg;
    W.used = (uint32_t)u;
    return kOk;
  }
  return *log >= 0 ? kOk : kNoRepeatTable;
}

struct Reps {
  uint64_t r0, r1, r2;
};

// A compressed block.  dst / cap / *outp: the frame's content, the room for it and how much of
// it there is; rep: the repeat offsets.
template <class P>
ZH_ZD_HD Verdict decode_block(const uint8_t* src, uint32_t len, uint8_t* dst, uint64_t cap,
                              uint64_t* outp, uint8_t* lit, uint64_t litcap, Work& W, Reps& rep,
                              P& p) {
  // -- literals section
  LitHeader lh;
  const Verdict hv = literals_header(src, len, &lh);
  if (hv) return hv;
  const uint32_t regen = lh.regen;
  const uint8_t* lits = nullptr;  // null: RLE literals of lbyte
  uint32_t lbyte = 0, lsec;
  if (lh.type == 0) {
    if (lh.hsz + regen > len) return kRawLitTruncated;
    lits = src + lh.hsz;
    lsec = lh.hsz + regen;
  } else if (lh.type == 1) {
    if (lh.hsz + 1 > len) return kRleLitTruncated;
    lbyte = src[lh.hsz];
    lsec = lh.hsz + 1;
  } else {
    if (lh.hsz + lh.csize > len) return kLitTruncated;
    const uint8_t* q = src + lh.hsz;
    uint32_t rem = lh.csize;
    if (lh.type == 2) {
      if (p.first()) W.verdict = huf_read_tree(q, rem, W);
      p.order();
      if (W.verdict) return (Verdict)W.verdict;
      huf_fill(W, p);
      p.order();
      q += W.used;
      rem -= W.used;
    } else if (W.huf_bits == 0) {
      return kNoHufTable;
    }
    if (regen > litcap) return kNoMemory;
    uint32_t s1 = 0, s2 = 0, s3 = 0, per = regen;
    if (lh.streams == 4) {
      if (rem < 6) return kJumpTruncated;
      s1 = rd_le(q, 2), s2 = rd_le(q + 2, 2), s3 = rd_le(q + 4, 2);
      if (6 + s1 + s2 + s3 > rem) return kStreamsTruncated;
      per = (regen + 3) / 4;
      if (3 * per > regen) return kFourStreamsShort;
    }
    Verdict sv = kOk;  // this lane's: of the first of its streams that fails
    for (uint32_t s = p.lane(); s < lh.streams; s += P::W) {
      if (lh.streams == 1) {
        sv = huf_stream(W, q, rem, lit, regen);
      } else {
        const uint32_t o = 6 + (s > 0 ? s1 : 0) + (s > 1 ? s2 : 0) + (s > 2 ? s3 : 0);
        const uint32_t n = s == 0 ? s1 : s == 1 ? s2 : s == 2 ? s3 : rem - 6 - s1 - s2 - s3;
        const Verdict vs =
            huf_stream(W, q + o, n, lit + (size_t)s * per, s < 3 ? per : regen - 3 * per);
        sv = sv ? sv : vs;
      }
    }
    const bool ok = p.all(sv == kOk);
    p.order();
    // a lane whose own stream decoded names the commonest reason for another lane's
    if (!ok) return sv ? sv : kHufStreamInexact;
    lits = lit;
    lsec = lh.hsz + lh.csize;
  }
  // -- sequences section
  const uint8_t* q = src + lsec;
  uint32_t rem = len - lsec;
  if (rem < 1) return kNoSequences;
  uint32_t nseq;
  if (q[0] < 128) {
    nseq = q[0];
    q += 1, rem -= 1;
  } else if (q[0] < 255) {
    if (rem < 2) return kCountTruncated;
    nseq = ((uint32_t)(q[0] - 128) << 8) + q[1];
    q += 2, rem -= 2;
  } else {
    if (rem < 3) return kCountTruncated;
    nseq = rd_le(q + 1, 2) + 0x7F00;
    q += 3, rem -= 3;
  }
  uint64_t out = *outp;
  uint32_t lpos = 0;
  if (nseq > 0) {
    if (rem < 1) return kNoModes;
    const uint32_t modes = q[0];
    if (modes & 3) return kReservedModes;
    q += 1, rem -= 1;
    for (int t = 0; t < 3; t++) {  // LL, OF, ML in stream order
      if (p.first()) {
        const int mode = (int)(modes >> (6 - 2 * t)) & 3;
        W.verdict =
            t == 0   ? seq_table(W.ll, &W.ll_log, mode, q, rem, kLLDefault, 36, 6, 9, 36, W)
            : t == 1 ? seq_table(W.of, &W.of_log, mode, q, rem, kOFDefault, 29, 5, 8, 32, W)
                     : seq_table(W.ml, &W.ml_log, mode, q, rem, kMLDefault, 53, 6, 9, 53, W);
      }
      p.order();
      if (W.verdict) return (Verdict)W.verdict;
      q += W.used;  // <= rem: the description was read inside it
      rem -= W.used;
    }
    BackBits b;
    const Verdict bv = b.init(q, rem);
    if (bv) return bv;
    const int lll = W.ll_log, ofl = W.of_log, mll = W.ml_log;
    uint32_t sll = (uint32_t)b.read(lll), sof = (uint32_t)b.read(ofl), sml = (uint32_t)b.read(mll);
    for (uint32_t k = 0; k < nseq; k++) {
      const uint32_t el = W.ll[sll], eo = W.of[sof], em = W.ml[sml];
      const uint32_t llc = el & 0xFF, ofc = eo & 0xFF, mlc = em & 0xFF;
      if (llc > 35 || mlc > 52 || ofc > 31) return kSequenceCode;
      const uint64_t ofv = (1ull << ofc) + b.read((int)ofc);
      const uint32_t ml = kMLBase[mlc] + (uint32_t)b.read(kMLBits[mlc]);
      const uint32_t ll = kLLBase[llc] + (uint32_t)b.read(kLLBits[llc]);
      if (k + 1 < nseq) {
        sll = (el >> 16) + (uint32_t)b.read((int)((el >> 8) & 0xFF));
        sml = (em >> 16) + (uint32_t)b.read((int)((em >> 8) & 0xFF));
        sof = (eo >> 16) + (uint32_t)b.read((int)((eo >> 8) & 0xFF));
      }
      uint64_t offset;  // repeat offsets (RFC 8878 3.1.2.5)
      if (ofv > 3) {
        offset = ofv - 3;
        rep.r2 = rep.r1, rep.r1 = rep.r0, rep.r0 = offset;
      } else {
        const unsigned idx = (unsigned)ofv - 1 + (ll == 0 ? 1u : 0u);
        if (idx == 0) {
          offset = rep.r0;
        } else {
          offset = idx == 1 ? rep.r1 : idx == 2 ? rep.r2 : rep.r0 - 1;
          if (idx > 1) rep.r2 = rep.r1;
          rep.r1 = rep.r0, rep.r0 = offset;
        }
      }
      if (ll > regen - lpos) return kPastLiterals;
      if ((uint64_t)ll + ml > cap - out) return kNoRoom;
      if (ll) {
        if (lits) p.copy(dst + out, lits + lpos, ll);
        else p.fill(dst + out, lbyte, ll);
      }
      lpos += ll;
      out += ll;
      if (offset == 0 || offset > out) return kOffset;
      p.match(dst, out, offset, ml);
      out += ml;
    }
    if (b.off != 0) return kSeqStreamInexact;
  }
  const uint32_t tail = regen - lpos;
  if (tail > cap - out) return kNoRoom;
  if (tail) {
    if (lits) p.copy(dst + out, lits + lpos, tail);
    else p.fill(dst + out, lbyte, tail);
  }
  *outp = out + tail;
  return kOk;
}

// One frame at src (it need not end at len): its content goes to dst, which has room for `cap`
// bytes.  `lit`: scratch for Huffman literals (kMaxRegen bytes hold any block's; Walk::max_regen
// this frame's).  *produced: the content's bytes, which equal the header's content size where it
// has one; *used: the frame's bytes, the checksum field included.  The checksum is not compared
// here, and whether the frame should fill dst or end at len is the caller's to say.
template <class P>
ZH_ZD_HD Verdict decode_frame(const uint8_t* src, size_t len, uint8_t* dst, uint64_t cap,
                              uint8_t* lit, uint64_t litcap, Work& W, P& p, uint64_t* produced,
                              size_t* used, Header* hdr) {
  Header& h = *hdr;
  const Verdict hv = frame_header(src, len, &h);
  if (hv) return hv;
  if (p.first()) {
    W.huf_bits = 0;
    W.ll_log = W.of_log = W.ml_log = -1;
    W.verdict = kOk;
    W.used = 0;
  }
  p.order();
  Reps rep{1, 4, 8};
  size_t pos = h.size;
  uint64_t out = 0;
  for (;;) {  // three input bytes per turn at least
    if (len - pos < 3) return kBlockHeaderTruncated;
    const uint32_t bh = rd_le(src + pos, 3);
    pos += 3;
    const uint32_t last = bh & 1, type = (bh >> 1) & 3, bsz = bh >> 3;
    if (type == 3) return kReservedBlockType;
    if (type == 1) {
      if (len - pos < 1) return kBlockTruncated;
      if (bsz > cap - out) return kNoRoom;
      p.fill(dst + out, src[pos], bsz);
      out += bsz;
      pos += 1;
    } else {
      if (bsz > len - pos) return kBlockTruncated;
      if (bsz > kMaxBlock) return kBlockTooLarge;
      if (type == 0) {
        if (bsz > cap - out) return kNoRoom;
        p.copy(dst + out, src + pos, bsz);
        out += bsz;
      } else {
        const Verdict v = decode_block(src + pos, bsz, dst, cap, &out, lit, litcap, W, rep, p);
        if (v) return v;
      }
      pos += bsz;
    }
    if (last) break;
  }
  if (h.fcs >= 0 && (uint64_t)h.fcs != out) return kSizeMismatch;
  if (h.csum) {
    if (len - pos < 4) return kChecksumTruncated;
    pos += 4;
  }
  *produced = out;
  *used = pos;
  return kOk;
}

// The host's lanes: one.
struct SerialLanes {
  static constexpr uint32_t W = 1;
  uint32_t lane() const { return 0; }
  bool first() const { return true; }
  void order() {}
  bool all(bool v) { return v; }
  void copy(uint8_t* d, const uint8_t* s, uint64_t n) {
    if (n) __builtin_memcpy(d, s, n);
  }
  void fill(uint8_t* d, uint32_t v, uint64_t n) {
    if (n) __builtin_memset(d, (int)v, n);
  }
  void match(uint8_t* d, uint64_t o, uint64_t off, uint64_t n) {
    uint8_t* t = d + o;
    if (n < 64) {  // short: byte after byte, the source may run into what this match stores
      const uint8_t* s = t - off;
      for (uint64_t k = 0; k < n; k++) t[k] = s[k];
      return;
    }
    // The off bytes below o repeat.  Every copy reads only bytes that are stored already, [o - off,
    // o + done), where done is a multiple of off: so what can be copied at once doubles.
    for (uint64_t done = 0; done < n;) {
      const uint64_t m = off + done < n - done ? off + done : n - done;
      __builtin_memcpy(t + done, t - off, m);
      done += m;
    }
  }
};

// One lane that stores nothing: the size of a frame whose header does not say it.  Every check
// of the decoder still applies; the destination is never dereferenced.
struct CountLanes : SerialLanes {
  void copy(uint8_t*, const uint8_t*, uint64_t) {}
  void fill(uint8_t*, uint32_t, uint64_t) {}
  void match(uint8_t*, uint64_t, uint64_t, uint64_t) {}
};

// ---- host: the walk over a frame's headers (no entropy decoding) -----------------------------
struct BlockInfo {  // a row of zh_debug_zstd_blocks
  int64_t type, stored, decoded;  // decoded: -1 when the header does not say (compressed)
  int64_t lit_type, streams, regen, nseq, ll_mode, of_mode, ml_mode;  // -1: not a compressed block
};
struct Walk {
  bool device = false;   // one frame, content size, no dictionary, an exact block chain
  int64_t fcs = -1;
  int64_t max_regen = 0;  // the largest Huffman literals section
  bool csum = false;
  uint32_t want = 0;      // the stored checksum
};

struct NoRows {
  void push_back(const BlockInfo&) {}
};

// Walks [src, src+len) as one frame.  B: vector-like of BlockInfo, or null.  Walk::device stays
// false at the first thing the device route does not take; the rows so far stay in place.
template <class B>
inline Walk walk_frame(const uint8_t* src, size_t len, B* rows) {
  Walk w;
  Header h;
  if (frame_header(src, len, &h)) return w;
  w.fcs = h.fcs;
  w.csum = h.csum != 0;
  size_t pos = h.size;
  uint64_t exact = 0, room = 0;  // bytes of raw / RLE blocks; what compressed blocks may add
  for (;;) {
    if (len - pos < 3) return w;
    const uint32_t bh = rd_le(src + pos, 3);
    pos += 3;
    const uint32_t last = bh & 1, type = (bh >> 1) & 3, bsz = bh >> 3;
    if (type == 3) return w;
    const size_t stored = type == 1 ? 1 : bsz;
    if (stored > len - pos || (type != 1 && bsz > kMaxBlock)) return w;
    BlockInfo bi{(int64_t)type, (int64_t)stored, type == 2 ? -1 : (int64_t)bsz,
                 -1, -1, -1, -1, -1, -1, -1};
    bool ok = true;
    if (type == 2) {
      LitHeader lh;
      ok = literals_header(src + pos, bsz, &lh) == kOk;
      if (ok) {
        bi.lit_type = lh.type, bi.streams = lh.streams, bi.regen = lh.regen;
        if (lh.type >= 2 && (int64_t)lh.regen > w.max_regen) w.max_regen = lh.regen;
        const uint64_t lsec = lh.hsz + (lh.type == 0 ? lh.regen : lh.type == 1 ? 1 : lh.csize);
        const uint8_t* q = src + pos + lsec;
        const uint64_t rem = lsec < bsz ? bsz - lsec : 0;
        if (rem >= 1 && q[0] < 128) {
          bi.nseq = q[0];
          q += 1;
        } else if (rem >= 2 && q[0] < 255) {
          bi.nseq = ((int64_t)(q[0] - 128) << 8) + q[1];
          q += 2;
        } else if (rem >= 3 && q[0] == 255) {
          bi.nseq = (int64_t)rd_le(q + 1, 2) + 0x7F00;
          q += 3;
        } else {
          ok = false;
        }
        if (ok && bi.nseq > 0) {
          if (q < src + pos + bsz)
            bi.ll_mode = q[0] >> 6, bi.of_mode = (q[0] >> 4) & 3, bi.ml_mode = (q[0] >> 2) & 3;
          else
            ok = false;
        }
      }
      room += kMaxBlock;
    } else {
      exact += bsz;
    }
    if (rows) rows->push_back(bi);
    if (!ok) return w;
    pos += stored;
    if (last) break;
  }
  if (h.csum) {
    if (len - pos < 4) return w;
    w.want = rd_le(src + pos, 4);
    pos += 4;
  }
  if (pos != len || h.fcs < 0) return w;
  if ((uint64_t)h.fcs < exact || (uint64_t)h.fcs > exact + room) return w;
  if (w.max_regen > h.fcs) return w;
  w.device = true;
  return w;
}

}  // namespace zh_zd
