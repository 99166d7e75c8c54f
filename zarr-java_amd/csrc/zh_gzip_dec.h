// zh_gzip_dec.h — the gzip member reader (RFC 1952) and its DEFLATE decoder (RFC 1951), written
// from the two specifications: the only one in the library.  zh_gzip_decompress (zh_gzip.cpp)
// runs it on the host, one lane; the batched device read (zh_gzip_dec_kernels.hip) runs it with a
// wave per member.  It decodes the FIRST member of a buffer and ignores what follows it, as
// zlib.decompress(b, 31) and the reference's GzipCompressorInputStream do.
//   header   magic 1f 8b, CM 8; the reserved FLG bits (0xe0) are rejected; FEXTRA, FNAME and
//            FCOMMENT are skipped; FHCRC (the low 16 bits of the CRC-32 of the header bytes) is
//            verified.
//   blocks   stored (LEN against NLEN), fixed and dynamic.  A dynamic block: HLIT <= 286 and
//            HDIST <= 30 codes; the code-length code first; the repeats 16, 17 and 18 run over
//            the literal/length lengths into the distance lengths, and are rejected without a
//            previous length or past HLIT + HDIST; a missing end-of-block code, an
//            over-subscribed set and an incomplete set are rejected, the last by zlib's rule: a
//            set may be incomplete only when it is a single code of length 1 (and the
//            code-length code never).  A distance set without any code is accepted.
//   symbols  literal/length symbols 286 and 287 and distance symbols 30 and 31 are invalid where
//            they are used, as is the unused code of an incomplete set; a distance beyond the
//            bytes produced so far is rejected.
//   trailer  eight bytes must follow the final block; ISIZE must equal the produced size mod
//            2^32.  Comparing the CRC-32 is the caller's, as is the text of an error.
// The blocks are a function of their own (decode_blocks), shared with the reader of a zlib stream
// (RFC 1950: decode_zlib_stream, for the streams of blosc frames in zh_blosc_streams.h):
//   header   two bytes: CM 8, CINFO <= 7, (CMF << 8 | FLG) % 31 == 0, FDICT clear;
//   trailer  four bytes, big-endian: the Adler-32 of the content (adler32 computes it across
//            the lanes; comparing is the caller's).  A zlib stream carries no size: the caller
//            knows it.
//
// Every step returns a Verdict: kOk, or the reason for rejecting the member.
//
// The templates are parameterised on a lane policy P, the one of zh_zstd_dec.h with one more
// store:
//     static const uint32_t W        lanes that share the member (1 on the host, 64 in a wave)
//     uint32_t lane()                this lane, < W
//     bool     first()               lane() == 0: runs the serial steps
//     void     order()               what this wave stored before is visible to its later loads
//     bool     all(bool)             true when true in every lane
//     void     copy(d, s, n)         d[k] = s[k]                  (across the lanes)
//     void     fill(d, byte, n)      d[k] = byte
//     void     match(d, o, off, n)   d[o+k] = d[o-off + k % off]  (off <= o; only bytes below o
//                                    are read)
//     void     spread(d, v, n)       d[lane()] = v in the lanes below n (n <= W): a literal run
//     uint32_t sum(v)                the sum of v over the lanes, in every lane (the Adler-32)
// Control flow is uniform over the lanes except where a loop starts at lane().  Symbols are
// decoded uniformly: every lane reads the same bit container and the same table entries.
// Literals are not stored one by one: lane k keeps the k-th literal of a run, and a run is
// stored (spread) when it reaches W, before a match and at a block's end.  The description of a
// dynamic block (a short serial chain) is read by the first lane, which leaves the sorted
// symbols, the counts, its bit position and its verdict in Work (LDS on the device) and is
// followed by order(); the lookup tables are then filled by all lanes.
//
// The members are untrusted.  Every loop is bounded by a checked count (HLIT + HDIST, a table
// size, LEN) or consumes at least one input bit per turn; a code or field that would end past
// the member is kTruncated (the container reads zeros there, but nothing past the end is ever
// accepted); every write is checked against the room the caller gave; every table index is
// masked or bounded by the counts that built the table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZH_GD_HD __host__ __device__ inline
#else
#define ZH_GD_HD inline
#endif

namespace zh_gd {

constexpr int kLitBits = 10, kDistBits = 8;  // the lookup tables; longer codes walk the counts
constexpr uint32_t kMaxLit = 288, kMaxDist = 32, kEndOfBlock = 256;
constexpr uint32_t kMaxExpand = 1032;  // a 258-byte match from a 2-bit pair of codes

// Why a member is rejected.  zh_gzip.cpp has the status and text of each.
enum Verdict : int32_t {
  kOk = 0,
  kBadMagic, kBadMethod, kReservedFlag, kHeaderTruncated, kHeaderCrc,
  kBlockType, kStoredLen, kTooManyCodes, kCodeLengthSet, kRepeat, kNoEndOfBlock,
  kLitLenSet, kDistSet, kLitLenCode, kDistCode, kDistTooFar,
  kTruncated, kNoRoom, kTrailerTruncated, kSizeMismatch,
  // the callers': the checksum, and what the device plan adds
  kCrcMismatch, kNotToTheEnd,
  // a zlib stream (RFC 1950): its header, its trailer and its checksum
  kZlibHeader, kZlibDictionary, kZlibTrailerTruncated, kAdlerMismatch,
  kVerdicts
};

constexpr uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2,
                                   2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,
                                    33,  49,  65,  97,  129, 193,  257,  385,  513,  769,
                                    1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2,  3,  3,  4,  4,  5,  5,  6,
                                    6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// One canonical code: the symbols with a length, sorted by (length, symbol), and per length how
// many there are, where they start in `sym` and the first code.
struct Code {
  uint16_t count[16], offs[17], first[16];
};

// Per-member working memory.  Table entry: symbol << 4 | code length; 0: no code of at most the
// table's bits starts like this (a longer code, or the hole of an incomplete set).
struct Work {
  uint16_t lit[1 << kLitBits];
  uint16_t dist[1 << kDistBits];
  uint16_t lsym[kMaxLit], dsym[kMaxDist];
  Code lc, dc;
  uint8_t lens[kMaxLit + kMaxDist];
  // the serial steps' own: the code-length code, and the cursors of a sort (in Work, not on the
  // stack: the device keeps no array in scratch memory)
  Code cc;
  uint16_t csym[19], next[16];
  uint8_t cl[19];
  uint32_t nlen, ndist;  // of the block described last
  uint64_t pos;          // the bit position after the last serial step
  int32_t verdict;       // of the last serial step
};

// A row of zh_debug_gzip_blocks.
struct BlockInfo {
  int64_t type, stored_bits, decoded, hlit, hdist, max_lit_len, max_dist_len, dist_codes, max_dist;
};
struct Trace {
  BlockInfo* rows;
  int64_t cap, n;
};

ZH_GD_HD uint32_t rd_le(const uint8_t* p, int n) {  // n <= 4
  uint32_t v = 0;
  for (int i = n - 1; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}
ZH_GD_HD uint32_t crc_byte(uint32_t r, uint8_t b) {  // headers only: no table
  r ^= b;
  for (int k = 0; k < 8; k++) r = r & 1u ? (r >> 1) ^ 0xEDB88320u : r >> 1;
  return r;
}

// ---- member header -----------------------------------------------------------------------------
// *size: the bytes up to the first block.
ZH_GD_HD Verdict member_header(const uint8_t* s, size_t n, size_t* size) {
  if (n >= 2 && (s[0] != 0x1f || s[1] != 0x8b)) return kBadMagic;
  if (n >= 3 && s[2] != 8) return kBadMethod;
  if (n >= 4 && (s[3] & 0xe0)) return kReservedFlag;
  if (n < 10) return kHeaderTruncated;
  const uint32_t flg = s[3];
  size_t p = 10;
  if (flg & 4) {  // FEXTRA
    if (n - p < 2) return kHeaderTruncated;
    const size_t xlen = rd_le(s + p, 2);
    p += 2;
    if (n - p < xlen) return kHeaderTruncated;
    p += xlen;
  }
  for (uint32_t f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & f)) continue;
    while (p < n && s[p]) p++;
    if (p == n) return kHeaderTruncated;
    p++;
  }
  if (flg & 2) {  // FHCRC
    if (n - p < 2) return kHeaderTruncated;
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < p; i++) r = crc_byte(r, s[i]);
    if (((r ^ 0xFFFFFFFFu) & 0xFFFFu) != rd_le(s + p, 2)) return kHeaderCrc;
    p += 2;
  }
  *size = p;
  return kOk;
}

// ---- the bit stream: forwards, LSB first ---------------------------------------------------------
// A 64-bit container over bits [cbase, cbase + 64), refilled from at most 8 bytes; bytes past the
// end read as zero.  peek never moves; skip is the caller's after it has checked `left`.
struct Bits {
  const uint8_t* p;
  uint64_t len, nbits, pos, cbase, cont;
  ZH_GD_HD void init(const uint8_t* src, size_t n) {
    p = src;
    len = n;
    nbits = (uint64_t)n * 8;
    pos = 0;
    cbase = 0;
    cont = 0;
    refill();
  }
  ZH_GD_HD void refill() {
    cbase = pos & ~(uint64_t)7;
    const uint64_t b0 = cbase >> 3;
    if (b0 + 8 <= len) {  // inside the member: one load (little-endian on both sides)
      __builtin_memcpy(&cont, p + b0, 8);
    } else {
      cont = 0;
      for (uint64_t i = 0; i < 8 && b0 + i < len; i++) cont |= (uint64_t)p[b0 + i] << (8 * i);
    }
  }
  ZH_GD_HD void seek(uint64_t to) {
    pos = to;
    refill();
  }
  __attribute__((always_inline)) ZH_GD_HD uint32_t peek(int n) {  // n <= 32
    if (n == 0) return 0;
    if (pos + (uint64_t)n > cbase + 64) refill();  // pos - cbase < 8 afterwards: 57 bits
    return (uint32_t)(cont >> (pos - cbase)) & (uint32_t)((1ull << n) - 1);
  }
  ZH_GD_HD bool has(uint64_t n) const { return pos + n <= nbits; }
  // n <= 32 bits, or kTruncated
  __attribute__((always_inline)) ZH_GD_HD Verdict take(int n, uint32_t* v) {
    if (!has((uint64_t)n)) return kTruncated;
    *v = peek(n);
    pos += (uint64_t)n;
    return kOk;
  }
};

// ---- canonical codes -------------------------------------------------------------------------
// Serial.  Counts, zlib's completeness rule, the first codes and the sorted symbols of lens[0..n).
// `why`: the verdict of a bad set.
ZH_GD_HD Verdict code_build(const uint8_t* lens, uint32_t n, Code* c, uint16_t* sym, uint16_t* next,
                            Verdict why) {
  for (int l = 0; l < 16; l++) c->count[l] = 0;
  for (uint32_t s = 0; s < n; s++) c->count[lens[s] & 15]++;
  int left = 1, max = 0;
  for (int l = 1; l < 16; l++) {
    left = (left << 1) - (int)c->count[l];
    if (left < 0) return why;  // over-subscribed
    if (c->count[l]) max = l;
  }
  if (left > 0 && max > 1) return why;  // incomplete, and not a single code of length 1
  uint32_t code = 0, at = 0;
  for (int l = 1; l < 16; l++) {
    c->first[l] = (uint16_t)code;
    c->offs[l] = (uint16_t)at;
    code = (code + c->count[l]) << 1;
    at += c->count[l];
  }
  c->offs[16] = (uint16_t)at;
  c->first[0] = c->offs[0] = 0;
  for (int l = 1; l < 16; l++) next[l] = c->offs[l];
  for (uint32_t s = 0; s < n; s++)
    if (lens[s] & 15) sym[next[lens[s] & 15]++] = (uint16_t)s;
  return kOk;
}

// Across the lanes: the lookup table of the codes of at most `bits` bits.
template <class P>
ZH_GD_HD void table_fill(uint16_t* tab, int bits, const Code& c, const uint16_t* sym, P& p) {
  const uint32_t size = 1u << bits;
  for (uint32_t k = p.lane(); k < size; k += P::W) tab[k] = 0;
  p.order();
  const uint32_t total = c.offs[16];
  for (uint32_t i = p.lane(); i < total; i += P::W) {
    int l = 1;
    while (l < 15 && i >= c.offs[l + 1]) l++;  // offs rises to offs[16] = total > i
    if (l > bits) continue;
    const uint32_t code = (uint32_t)c.first[l] + (i - c.offs[l]);
    uint32_t rev = 0;  // the stream has a code's first bit lowest
    for (int b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
    const uint16_t e = (uint16_t)((uint32_t)sym[i] << 4 | (uint32_t)l);
    for (uint32_t k = rev; k < size; k += 1u << l) tab[k] = e;
  }
  p.order();
}

// One symbol from the 15 bits `v` (zeros past the end): through the table, or bit by bit along
// the counts.  Returns the code's length, 0 when no code starts like this.
__attribute__((always_inline)) ZH_GD_HD int symbol(uint32_t v, const uint16_t* tab, int bits,
                                                   const Code& c, const uint16_t* sym,
                                                   uint32_t* out) {
  const uint32_t e = tab[v & ((1u << bits) - 1)];
  if (e) {
    *out = e >> 4;
    return (int)(e & 15u);
  }
  uint32_t code = 0, first = 0, index = 0;
  for (int l = 1; l < 16; l++) {
    code |= (v >> (l - 1)) & 1u;
    const uint32_t cnt = c.count[l];
    if (code - first < cnt) {  // code >= first always
      *out = sym[index + (code - first)];
      return l;
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return 0;
}

// Serial: the description of a dynamic block into w.lens / w.nlen / w.ndist and the two codes.
ZH_GD_HD Verdict read_dynamic(Bits& in, Work& w) {
  uint32_t v = 0;
  if (in.take(14, &v)) return kTruncated;
  const uint32_t nlen = (v & 31u) + 257, ndist = ((v >> 5) & 31u) + 1, ncode = (v >> 10) + 4;
  if (nlen > 286 || ndist > 30) return kTooManyCodes;
  uint8_t* cl = w.cl;
  for (int i = 0; i < 19; i++) cl[i] = 0;
  for (uint32_t i = 0; i < ncode; i++) {
    if (in.take(3, &v)) return kTruncated;
    cl[kClOrder[i]] = (uint8_t)v;
  }
  // the code-length code may not be incomplete, not even as a single code; without any code
  // zlib reads a zero length from every bit and then misses the end-of-block code
  Code& cc = w.cc;
  uint16_t* csym = w.csym;
  if (code_build(cl, 19, &cc, csym, w.next, kCodeLengthSet)) return kCodeLengthSet;
  int left = 1;
  for (int l = 1; l < 16; l++) left = (left << 1) - (int)cc.count[l];
  if (left != 0) return kCodeLengthSet;
  const uint32_t total = nlen + ndist;
  uint32_t have = 0;
  while (have < total) {  // every turn takes at least one bit
    const uint32_t bits7 = in.peek(7);
    uint32_t code = 0, first = 0, index = 0, s = 19;
    int l = 1;
    for (; l <= 7; l++) {
      code |= (bits7 >> (l - 1)) & 1u;
      const uint32_t cnt = cc.count[l];
      if (code - first < cnt) {
        s = csym[index + (code - first)];
        break;
      }
      index += cnt;
      first = (first + cnt) << 1;
      code <<= 1;
    }
    if (s == 19) return kCodeLengthSet;  // not reached: the code is complete
    if (!in.has((uint64_t)l)) return kTruncated;
    in.pos += (uint64_t)l;
    if (s < 16) {
      w.lens[have++] = (uint8_t)s;
      continue;
    }
    uint32_t rep = 0, val = 0;
    if (s == 16) {
      if (have == 0) return kRepeat;
      val = w.lens[have - 1];
      if (in.take(2, &rep)) return kTruncated;
      rep += 3;
    } else if (s == 17) {
      if (in.take(3, &rep)) return kTruncated;
      rep += 3;
    } else {
      if (in.take(7, &rep)) return kTruncated;
      rep += 11;
    }
    if (have + rep > total) return kRepeat;
    while (rep--) w.lens[have++] = (uint8_t)val;
  }
  if (w.lens[kEndOfBlock] == 0) return kNoEndOfBlock;
  w.nlen = nlen;
  w.ndist = ndist;
  if (code_build(w.lens, nlen, &w.lc, w.lsym, w.next, kLitLenSet)) return kLitLenSet;
  if (code_build(w.lens + nlen, ndist, &w.dc, w.dsym, w.next, kDistSet)) return kDistSet;
  return kOk;
}

// Serial: the fixed codes of RFC 1951 §3.2.6.
ZH_GD_HD void read_fixed(Work& w) {
  for (uint32_t s = 0; s < 288; s++) w.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
  for (uint32_t s = 0; s < 32; s++) w.lens[288 + s] = 5;
  w.nlen = 288;
  w.ndist = 32;
  (void)code_build(w.lens, 288, &w.lc, w.lsym, w.next, kLitLenSet);
  (void)code_build(w.lens + 288, 32, &w.dc, w.dsym, w.next, kDistSet);
}

// ---- the blocks ----------------------------------------------------------------------------
// The DEFLATE blocks from in.pos up to and including the final block, into dst[0, room).  *made:
// the bytes produced.  What stands before the first block and behind the last one is the
// caller's: decode_member (gzip) and decode_zlib_stream (zlib) below.  kTrace (host): one
// BlockInfo per block into *tr.
template <class P, bool kTrace = false>
ZH_GD_HD Verdict decode_blocks(Bits& in, uint8_t* dst, uint64_t room, Work& w, P& p,
                               uint64_t* made, Trace* tr = nullptr) {
  uint64_t out = 0;
  uint32_t run = 0, mine = 0;  // the literal run: `mine` is this lane's
  int tables = 0;              // 1: the fixed codes are in w, 2: a dynamic block's
  for (bool last = false; !last;) {
    uint32_t v = 0;
    if (in.take(3, &v)) return kTruncated;
    last = v & 1u;
    const uint32_t type = v >> 1;
    BlockInfo bi = {(int64_t)type, 0, 0, -1, -1, 0, 0, 0, 0};
    const uint64_t pos0 = in.pos - 3, out0 = out;
    if (type == 3) return kBlockType;
    if (type == 0) {
      in.seek((in.pos + 7) & ~(uint64_t)7);
      uint32_t ln = 0;
      if (in.take(32, &ln)) return kTruncated;
      const uint32_t n = ln & 0xFFFFu;
      if (n != (~ln >> 16)) return kStoredLen;
      const uint64_t at = in.pos >> 3;
      if (n > in.len - at) return kTruncated;
      if (n > room - out) return kNoRoom;
      p.copy(dst + out, in.p + at, n);
      out += n;
      in.seek(in.pos + (uint64_t)n * 8);
    } else {
      if (type == 2 || tables != 1) {
        if (p.first()) {
          w.verdict = kOk;
          if (type == 2) {
            w.verdict = read_dynamic(in, w);
          } else {
            read_fixed(w);
          }
          w.pos = in.pos;
        }
        p.order();
        if (w.verdict) return (Verdict)w.verdict;
        in.seek(w.pos);
        table_fill(w.lit, kLitBits, w.lc, w.lsym, p);
        table_fill(w.dist, kDistBits, w.dc, w.dsym, p);
        tables = (int)type;
      }
      if (kTrace) {
        bi.hlit = w.nlen;
        bi.hdist = w.ndist;
        for (int l = 1; l < 16; l++) {
          if (w.lc.count[l]) bi.max_lit_len = l;
          if (w.dc.count[l]) bi.max_dist_len = l;
        }
        bi.dist_codes = w.dc.offs[16];
      }
      for (;;) {  // every turn takes at least one bit
        uint32_t s = 0;
        int l = symbol(in.peek(15), w.lit, kLitBits, w.lc, w.lsym, &s);
        if (l == 0) return in.has(15) ? kLitLenCode : kTruncated;
        if (!in.has((uint64_t)l)) return kTruncated;
        in.pos += (uint64_t)l;
        if (s < 256) {
          if (run == P::W) {
            p.spread(dst + out, mine, run);
            out += run;
            run = 0;
          }
          if (room - out <= run) return kNoRoom;
          if (p.lane() == run) mine = s;
          run++;
          continue;
        }
        if (run) {  // a match or the block's end: the run goes out first
          p.spread(dst + out, mine, run);
          out += run;
          run = 0;
        }
        if (s == kEndOfBlock) break;
        if (s > 285) return kLitLenCode;
        uint32_t extra = 0;
        if (in.take(kLenExtra[s - 257], &extra)) return kTruncated;
        const uint32_t mlen = kLenBase[s - 257] + extra;
        uint32_t d = 0;
        l = symbol(in.peek(15), w.dist, kDistBits, w.dc, w.dsym, &d);
        if (l == 0) return in.has(15) ? kDistCode : kTruncated;
        if (!in.has((uint64_t)l)) return kTruncated;
        in.pos += (uint64_t)l;
        if (d > 29) return kDistCode;
        if (in.take(kDistExtra[d], &extra)) return kTruncated;
        const uint64_t off = (uint64_t)kDistBase[d] + extra;
        if (off > out) return kDistTooFar;
        if (mlen > room - out) return kNoRoom;
        p.match(dst, out, off, mlen);
        out += mlen;
        if (kTrace && (int64_t)off > bi.max_dist) bi.max_dist = (int64_t)off;
      }
    }
    if (kTrace && tr) {
      bi.stored_bits = (int64_t)(in.pos - pos0);
      bi.decoded = (int64_t)(out - out0);
      if (tr->rows && tr->n < tr->cap) tr->rows[tr->n] = bi;
      tr->n++;
    }
  }
  *made = out;
  return kOk;
}

// ---- a member ------------------------------------------------------------------------------
// Decodes the first member of src[0, len) into dst[0, room).  *made: the bytes produced; *used:
// the member's bytes, its trailer included; *crc: the stored CRC-32.  kTrace (host): one
// BlockInfo per block into *tr.
template <class P, bool kTrace = false>
ZH_GD_HD Verdict decode_member(const uint8_t* src, size_t len, uint8_t* dst, uint64_t room,
                               Work& w, P& p, uint64_t* made, size_t* used, uint32_t* crc,
                               Trace* tr = nullptr) {
  size_t hsize = 0;
  Verdict hv = member_header(src, len, &hsize);
  if (hv) return hv;
  Bits in;
  in.init(src + hsize, len - hsize);
  uint64_t out = 0;
  const Verdict bv = decode_blocks<P, kTrace>(in, dst, room, w, p, &out, tr);
  if (bv) return bv;
  const uint64_t at = (in.pos + 7) >> 3;
  if (in.len - at < 8) return kTrailerTruncated;
  if (rd_le(in.p + at + 4, 4) != (uint32_t)out) return kSizeMismatch;
  *crc = rd_le(in.p + at, 4);
  *made = out;
  *used = hsize + (size_t)at + 8;
  return kOk;
}

// ---- a zlib stream (RFC 1950) --------------------------------------------------------------
// The two header bytes: CM 8, CINFO <= 7, (CMF << 8 | FLG) a multiple of 31, no preset
// dictionary.  *cinfo: the window size the writer declared (7: 32 KiB, what compress2 writes).
ZH_GD_HD Verdict zlib_header(const uint8_t* s, size_t n, uint32_t* cinfo) {
  if (n < 2) return kZlibHeader;
  const uint32_t cmf = s[0], flg = s[1];
  if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u != 0) return kZlibHeader;
  if (flg & 0x20u) return kZlibDictionary;
  *cinfo = cmf >> 4;
  return kOk;
}

// Decodes the zlib stream at src[0, len) into dst[0, room): the header above, the blocks, and
// the four bytes of the trailer.  *made: the bytes produced; *used: the stream's bytes, its
// trailer included (what follows is ignored, as zlib's uncompress ignores it); *adler: the stored
// Adler-32, big-endian in the stream.  Comparing it (adler32 below) is the caller's, as the
// CRC-32 of a member is.  A distance is checked against the bytes produced so far and not
// against the declared window, like a zlib built without strict window checking.
template <class P>
ZH_GD_HD Verdict decode_zlib_stream(const uint8_t* src, size_t len, uint8_t* dst, uint64_t room,
                                    Work& w, P& p, uint64_t* made, size_t* used,
                                    uint32_t* adler) {
  uint32_t cinfo = 0;
  const Verdict hv = zlib_header(src, len, &cinfo);
  if (hv) return hv;
  Bits in;
  in.init(src + 2, len - 2);
  uint64_t out = 0;
  const Verdict bv = decode_blocks(in, dst, room, w, p, &out);
  if (bv) return bv;
  const uint64_t at = (in.pos + 7) >> 3;
  if (in.len - at < 4) return kZlibTrailerTruncated;
  const uint8_t* t = in.p + at;
  *adler = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
  *made = out;
  *used = 2 + (size_t)at + 4;
  return kOk;
}

// Across the lanes: the Adler-32 of d[0, n), the same value in every lane.  With M = 65521,
// A = 1 + sum d[i] mod M and B = n + sum (n - i) d[i] mod M; the value is B << 16 | A.
// The bytes go in chunks of at most kAdlerChunk; a chunk of L bytes with s1 = sum d[j] and
// s2 = sum (L - j) d[j] takes (A, B) to (A + s1, B + L A + s2).  Inside a chunk lane l takes
// the four bytes at j0 = 4 (W r + l) of every round r (bytes past L count as zero), so with
// s = d0 + d1 + d2 + d3 of a round its share of s2 is
//     (L - 4 l) sum s  -  4 W sum r s  -  sum (d1 + 2 d2 + 3 d3)
// in 64-bit sums that cannot overflow: L <= 2^24 gives at most 2^16 rounds in a wave, sum s <
// 2^26, sum r s < 2^42, and the products stay below 2^51 (on one lane: 2^22 rounds, sum s < 2^32,
// sum r s < 2^54, products below 2^57).  The share is a sum of non-negative terms, so the
// differences never wrap.  A lane's two sums are reduced mod M before the lanes are added
// (P::sum, 32 bits: W values below 2^16).
// On the device the bytes are what this wave stored: the caller has order() before this.
constexpr uint32_t kAdlerMod = 65521;
constexpr uint64_t kAdlerChunk = (uint64_t)1 << 24;  // a multiple of 4 W
template <class P>
ZH_GD_HD uint32_t adler32(const uint8_t* d, uint64_t n, P& p) {
  uint64_t A = 1, B = 0;
  for (uint64_t c0 = 0; c0 < n; c0 += kAdlerChunk) {
    const uint8_t* q = d + c0;
    const uint64_t L = n - c0 < kAdlerChunk ? n - c0 : kAdlerChunk;
    const uint64_t l4 = 4 * (uint64_t)p.lane();
    uint64_t a = 0, c = 0, e = 0, r = 0;
    for (uint64_t j0 = l4; j0 < L; j0 += 4 * (uint64_t)P::W, r++) {
      uint32_t v = 0;
      if (j0 + 4 <= L) {
        __builtin_memcpy(&v, q + j0, 4);  // little-endian on both sides
      } else {
        for (uint64_t t = 0; j0 + t < L; t++) v |= (uint32_t)q[j0 + t] << (8 * t);
      }
      const uint32_t d0 = v & 255u, d1 = (v >> 8) & 255u, d2 = (v >> 16) & 255u, d3 = v >> 24;
      const uint64_t s = d0 + d1 + d2 + d3;
      a += s;
      c += r * s;
      e += d1 + 2 * d2 + 3 * d3;
    }
    // a lane without bytes in the chunk has a = c = e = 0 (and L < 4 l does no harm)
    const uint64_t mine = (L - l4) * a - 4 * (uint64_t)P::W * c - e;
    const uint64_t s1 = p.sum((uint32_t)(a % kAdlerMod));
    const uint64_t s2 = p.sum((uint32_t)(mine % kAdlerMod));
    B = (B + (L % kAdlerMod) * A + s2) % kAdlerMod;
    A = (A + s1) % kAdlerMod;
  }
  return (uint32_t)(B << 16 | A);
}

// ---- host lane policies --------------------------------------------------------------------
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
    const uint8_t* s = t - off;  // byte after byte: the source may run into what this stores
    for (uint64_t k = 0; k < n; k++) t[k] = s[k];
  }
  void spread(uint8_t* d, uint32_t v, uint32_t n) {
    if (n) d[0] = (uint8_t)v;
  }
  uint32_t sum(uint32_t v) { return v; }
};
// Stores nothing: the size query.
struct CountLanes : SerialLanes {
  void copy(uint8_t*, const uint8_t*, uint64_t) {}
  void fill(uint8_t*, uint32_t, uint64_t) {}
  void match(uint8_t*, uint64_t, uint64_t, uint64_t) {}
  void spread(uint8_t*, uint32_t, uint32_t) {}
};

}  // namespace zh_gd
