// zh_gzip_enc.h — the gzip member writer shared by the host and the device (RFC 1951 / RFC 1952;
// zlib and Python's gzip are the independent readers).
//
// Member: the 10 header bytes 1f 8b 08 00 00 00 00 00 00 ff (no name, mtime 0, XFL 0, OS 255),
// the segments, the final empty fixed block 03 00, then CRC-32 of the content and n mod 2^32,
// both little endian.  One chunk is one member.
// Segments: the content is cut into blocks of B bytes (the last one shorter); each is compressed
// on its own with the `wide` matcher of zh_lz_match.h: no match reaches before the block's first
// byte, so one wave can take one block, and B <= 32 KiB, DEFLATE's window, bounds every distance.
// A block becomes one byte-aligned segment, the smaller of two forms (stored on a tie):
//   * fixed: header bits BFINAL 0, BTYPE 01; the fixed Huffman codes of RFC 1951 §3.2.6 (codes
//     MSB first, extra bits LSB first, in an LSB-first bit stream); the end-of-block code; an
//     empty stored block as a sync marker: bits 000, zero bits up to the byte boundary,
//     00 00 ff ff;
//   * stored: 00, LEN, NLEN, the block's bytes: 5 bytes over raw.
// A third form (dynamic Huffman) would join the same choice without changing the layout.
// So no member is larger than 20 + n + 5 * ceil(n / B), the bound the interface reports.
// Two phases per block, as in the zstd writer:
//   match_block    over a lane policy W: (literal length, match length, offset) records,
//                  3 x uint16, to a list (a record covers kMinMatch bytes or more: n / 4 at the
//                  most), and the number of bytes the matches cover.  The literals stay where
//                  they are: the coder reads them from the block;
//   deflate_block  serial and forwards: every literal and every record through the fixed codes
//                  into a 64-bit accumulator flushed in whole bytes.  A match longer than 258 is
//                  split by piece_count / piece_len, the one statement of the rule.  The codes
//                  are computed (lit_bits, match_bits), not looked up: the writer has no tables.
//                  The bit position of a symbol is a prefix sum of code lengths, so the device
//                  runs the same coding a wave per block (zh_gzip_enc_kernels.hip); the segment
//                  is stored exactly when the fixed form would pass n + 4 bytes, in both.
// The CRC-32 is linear, so a content is hashed in spans that are combined with x^(8 len) mod P
// (mulmod, xpow8, crc_finish): the device hashes spans in parallel, the host folds them.
// The output is a pure function of (input bytes, B).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "zh_lz_match.h"

namespace zh_gz {

constexpr uint32_t kMaxBlock = 32u << 10;  // DEFLATE's window
constexpr uint32_t kMinBlock = 1u << 10;
constexpr uint32_t kDefaultBlock = 16u << 10;  // DESIGN.md "Gzip members encoded on the device"
constexpr uint32_t kMaxMatch = 258, kMinPiece = 3;
constexpr size_t kHeader = 10, kEnding = 2, kTrailer = 8;
constexpr uint32_t kStoredOver = 5;  // a stored segment: 00 LEN NLEN
constexpr uint32_t kMinSegment = 6;  // an empty fixed block and its sync marker
constexpr uint32_t kPoly = 0xEDB88320u;
static_assert(kMaxBlock <= zh_lz::kMaxBlock, "positions and lengths fit 16 bits");

ZH_BS_HD uint32_t highbit32(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

ZH_BS_HD uint32_t block_bytes(int32_t configured) {
  if (configured <= 0) return kDefaultBlock;
  return (uint32_t)configured < kMinBlock   ? kMinBlock
         : (uint32_t)configured > kMaxBlock ? kMaxBlock
                                            : (uint32_t)configured;
}

// ---- CRC-32 (IEEE, reflected) -------------------------------------------------------------
// a * b mod P; bit 31 is x^0.
ZH_BS_HD uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = b & 1u ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}
// x^(8 n) mod P
ZH_BS_HD uint32_t xpow8(uint64_t n) {
  uint32_t p = 1u << 31, sq = 1u << 23;
  for (; n; n >>= 1) {
    if (n & 1u) p = mulmod(sq, p);
    sq = mulmod(sq, sq);
  }
  return p;
}
ZH_BS_HD uint32_t crc_table_entry(uint32_t c) {
  for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ kPoly : c >> 1;
  return c;
}
// The register after `len` more bytes, without the inversions (`raw`: started at 0, the
// content's polynomial times x^32 mod P).
inline uint32_t crc_raw(uint32_t r, const uint8_t* p, size_t len) {
  static const struct Tab {
    uint32_t t[256];
    Tab() {
      for (uint32_t i = 0; i < 256; i++) t[i] = crc_table_entry(i);
    }
  } T;
  for (size_t i = 0; i < len; i++) r = T.t[(r ^ p[i]) & 255u] ^ (r >> 8);
  return r;
}
// raw(A || B) from raw(A), raw(B) and x^(8 |B|)
ZH_BS_HD uint32_t crc_append(uint32_t raw_a, uint32_t raw_b, uint32_t xlen_b) {
  return mulmod(raw_a, xlen_b) ^ raw_b;
}
// zlib's crc32 of n bytes from their raw register: the initial ones, moved n bytes, and the
// final inversion.
ZH_BS_HD uint32_t crc_finish(uint32_t raw, uint64_t n) {
  return raw ^ mulmod(0xFFFFFFFFu, xpow8(n)) ^ 0xFFFFFFFFu;
}

// ---- phase 1 ------------------------------------------------------------------------------
// s: the block (n <= kMaxBlock bytes); seq: room for 3 * (n / 4) + 3 uint16; table: kHashSize
// slots.  Returns the number of records; *covered: the bytes their matches cover.
template <class W>
ZH_BS_HD uint32_t match_block(const uint8_t* s, uint32_t n, uint16_t* seq, uint32_t* table, W& w,
                              uint32_t* covered) {
  *covered = 0;
  if (n < 8 || n > kMaxBlock) return 0;
  w.clear(table);
  const uint32_t lim = n - 4;  // the last position 4 bytes can be read at
  uint32_t p = 0, a = 0, ns = 0, cov = 0;
  while (p <= lim) {
    uint32_t ref = 0;
    const uint32_t lane = w.find(s, p, lim, table, &ref);
    if (lane == 64) {
      w.insert(p, lim + 1, table);
      p += 64;
      continue;
    }
    const uint32_t m = p + lane;
    const uint32_t ml = 4 + w.extend(s, ref + 4, m + 4, n - (m + 4));
    w.put16(seq + 3 * ns, m - a);
    w.put16(seq + 3 * ns + 1, ml);  // m >= 1: ml < n
    w.put16(seq + 3 * ns + 2, m - ref);
    ns++;
    cov += ml;
    w.insert(p, m + ml < lim + 1 ? m + ml : lim + 1, table);
    p = a = m + ml;
  }
  *covered = cov;
  return ns;
}

// ---- phase 2 ------------------------------------------------------------------------------
// The pieces of a match of ml bytes: none longer than 258, none shorter than 3.  Pieces of 258
// while what is left stays above 258; a rest of 259 or 260 is cut into 256 or 257 and 3.
ZH_BS_HD uint32_t piece_count(uint32_t ml) {
  return ml <= kMaxMatch ? 1 : (ml + kMaxMatch - 1) / kMaxMatch;
}
ZH_BS_HD uint32_t piece_len(uint32_t ml, uint32_t j) {
  if (ml <= kMaxMatch) return ml;
  const uint32_t q = ml / kMaxMatch, r = ml % kMaxMatch;
  if (r == 0 || r >= kMinPiece) return j < q ? kMaxMatch : r;
  if (j + 1 < q) return kMaxMatch;
  return j + 1 == q ? kMaxMatch + r - kMinPiece : kMinPiece;
}

ZH_BS_HD uint32_t rev16(uint32_t v) {
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
  return ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
}
// A Huffman code of nb bits as the LSB-first stream takes it.
ZH_BS_HD uint32_t huff(uint32_t code, uint32_t nb) { return rev16(code) >> (16 - nb); }

// (bits, count) of a literal: 0..143 are 8 bits from 0x30, 144..255 are 9 bits from 0x190.
ZH_BS_HD uint32_t lit_bits(uint32_t v, uint32_t* nb) {
  *nb = v < 144 ? 8u : 9u;
  return v < 144 ? huff(0x30 + v, 8) : huff(0x190 + (v - 144), 9);
}
// (bits, count) of a match of 3..258 bytes at a distance of 1..32768: the length code
// (257..279: 7 bits from 0; 280..287: 8 bits from 0xC0), its extra bits, the 5-bit distance code,
// its extra bits: 31 bits at the most.
ZH_BS_HD uint32_t match_bits(uint32_t len, uint32_t dist, uint32_t* nb) {
  const uint32_t l = len - 3;
  uint32_t le = l < 8 ? 0 : highbit32(l) - 2;
  uint32_t lc = 4 * le + (l >> le);  // the code - 257
  uint32_t lx = l & ((1u << le) - 1);
  if (len == kMaxMatch) lc = 28, le = 0, lx = 0;  // code 285
  const uint32_t d = dist - 1;
  const uint32_t de = d < 4 ? 0 : highbit32(d) - 1;
  const uint32_t dc = 2 * de + (d >> de);
  const uint32_t dx = d & ((1u << de) - 1);
  uint32_t v, k;
  if (lc < 23) {
    v = huff(lc + 1, 7), k = 7;
  } else {
    v = huff(0xC0 + (lc - 23), 8), k = 8;
  }
  v |= lx << k, k += le;
  v |= huff(dc, 5) << k, k += 5;
  v |= dx << k, k += de;
  *nb = k;
  return v;
}

// LSB-first bit writer; stops at cap.
struct BitOut {
  uint8_t* d;
  uint32_t o, cap;
  uint64_t acc = 0;
  uint32_t cnt = 0;
  bool over = false;
  ZH_BS_HD void add(uint32_t v, uint32_t nb) {  // nb <= 32, cnt < 8
    acc |= (uint64_t)v << cnt;
    cnt += nb;
    while (cnt >= 8) {
      if (o >= cap) {
        over = true;
        acc = 0, cnt = 0;
        return;
      }
      d[o++] = (uint8_t)acc;
      acc >>= 8;
      cnt -= 8;
    }
  }
};

// s: the block; seq, ns, covered: what match_block left; out: room for n + 4 bytes.  Returns the
// size of the block's segment: that of the fixed form written to out, or n + kStoredOver when the
// fixed form would reach that (the segment is stored; out holds nothing of use).
ZH_BS_HD uint32_t deflate_block(const uint8_t* s, uint32_t n, const uint16_t* seq, uint32_t ns,
                                uint32_t covered, uint8_t* out) {
  const uint32_t stored = n + kStoredOver;
  if (covered > n) return stored;
  // at least 8 bits a literal and 12 a record, 13 bits of header, end and marker, 4 bytes
  if ((8 * (n - covered) + 12 * ns + 13 + 7) / 8 + 4 >= stored) return stored;
  BitOut b{out, 0, stored - 1};
  b.add(2, 3);  // BFINAL 0, BTYPE 01
  uint32_t pos = 0;
  for (uint32_t k = 0; k <= ns; k++) {
    const uint32_t lit = k < ns ? seq[3 * k] : n - pos;
    if (lit > n - pos) return stored;  // never: the records partition the block
    for (uint32_t i = 0; i < lit; i++) {
      uint32_t nb;
      const uint32_t v = lit_bits(s[pos + i], &nb);
      b.add(v, nb);
    }
    pos += lit;
    if (k == ns) break;
    const uint32_t ml = seq[3 * k + 1], off = seq[3 * k + 2];
    if (ml > n - pos || off == 0 || off > pos) return stored;  // never
    for (uint32_t j = 0, np = piece_count(ml); j < np; j++) {
      uint32_t nb;
      const uint32_t v = match_bits(piece_len(ml, j), off, &nb);
      b.add(v, nb);
    }
    pos += ml;
    if (b.over) return stored;
  }
  b.add(0, 7);  // end of block
  b.add(0, 3);  // the marker: BFINAL 0, BTYPE 00
  if (b.cnt) b.add(0, 8 - b.cnt);
  b.add(0xFFFF0000u, 32);  // LEN 0, NLEN ffff
  return b.over ? stored : b.o;
}

// ---- member layout --------------------------------------------------------------------------
inline size_t block_count(size_t n, uint32_t B) { return (n + B - 1) / B; }
inline uint32_t block_size(size_t n, uint32_t B, size_t k) {
  const size_t rest = n - k * B;
  return rest < B ? (uint32_t)rest : B;
}
inline size_t member_bound(size_t n, uint32_t B) {
  return kHeader + kEnding + kTrailer + n + (size_t)kStoredOver * block_count(n, B);
}
inline void put_header(uint8_t* d) {
  const uint8_t h[kHeader] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
  for (size_t i = 0; i < kHeader; i++) d[i] = h[i];
}
// 03 00, CRC-32, ISIZE: kEnding + kTrailer bytes
inline void put_ending(uint8_t* d, uint32_t crc, size_t n) {
  d[0] = 3, d[1] = 0;
  for (int i = 0; i < 4; i++) d[2 + i] = (uint8_t)(crc >> (8 * i));
  for (int i = 0; i < 4; i++) d[6 + i] = (uint8_t)((uint64_t)n >> (8 * i));
}
// LEN, NLEN of a stored segment as one little-endian word
inline uint32_t stored_word(uint32_t len) { return len | ((~len & 0xFFFFu) << 16); }

struct Params {
  uint32_t B = kDefaultBlock;
};
inline bool read_params(const zh_gzip_enc_params* p, Params* out) {
  if (!p || p->blocksize < 0) return false;
  out->B = block_bytes(p->blocksize);
  return true;
}

// One member on the host with HostLanes.  dst == nullptr: *len = the bound.
inline int compress_member(const uint8_t* src, size_t n, const zh_gzip_enc_params* prm,
                           uint8_t* dst, size_t cap, size_t* len, const char** msg) {
  Params P;
  if (!read_params(prm, &P) || (n > 0 && !src) || !len) {
    *msg = "zh_gzip_compress: blocksize >= 0";
    return ZH_EINVAL;
  }
  const size_t bound = member_bound(n, P.B);
  if (!dst) {
    *len = bound;
    return ZH_OK;
  }
  if (cap < bound) {
    *msg = "zh_gzip_compress: destination smaller than the bound";
    return ZH_EINVAL;
  }
  const size_t nb = block_count(n, P.B);
  uint8_t* seg = new uint8_t[P.B + kStoredOver];
  uint16_t* seq = new uint16_t[3 * (size_t)(P.B / 4) + 3];
  uint32_t* table = new uint32_t[zh_lz::kHashSize];
  zh_lz::HostLanes w;
  w.wide = true;
  put_header(dst);
  size_t p = kHeader;
  for (size_t k = 0; k < nb; k++) {
    const uint32_t bsz = block_size(n, P.B, k);
    const uint8_t* s = src + k * P.B;
    uint32_t covered = 0;
    const uint32_t ns = match_block(s, bsz, seq, table, w, &covered);
    const uint32_t size = deflate_block(s, bsz, seq, ns, covered, seg);
    if (size == bsz + kStoredOver) {
      const uint32_t word = stored_word(bsz);
      dst[p++] = 0;
      for (int i = 0; i < 4; i++) dst[p++] = (uint8_t)(word >> (8 * i));
      for (uint32_t q = 0; q < bsz; q++) dst[p + q] = s[q];
      p += bsz;
    } else {
      for (uint32_t q = 0; q < size; q++) dst[p + q] = seg[q];
      p += size;
    }
  }
  put_ending(dst + p, crc_finish(crc_raw(0, src, n), n), n);
  p += kEnding + kTrailer;
  delete[] table;
  delete[] seq;
  delete[] seg;
  if (p > bound) {
    *msg = "zh_gzip_compress: layout and bound disagree";
    return ZH_EINVAL;
  }
  *len = p;
  return ZH_OK;
}

}  // namespace zh_gz
