// zh_gzip_enc.h — the gzip member writer shared by the host and the device (RFC 1951 / RFC 1952;
// zlib and Python's gzip are the independent readers).
//
// Member: the 10 header bytes 1f 8b 08 00 00 00 00 00 00 ff (no name, mtime 0, XFL 0, OS 255),
// the segments, the final empty fixed block 03 00, then CRC-32 of the content and n mod 2^32,
// both little endian.  One chunk is one member.
// Segments: the content is cut into blocks of B bytes (the last one shorter); each is compressed
// on its own with the `wide` matcher of zh_lz_match.h: no match reaches before the block's first
// byte, so one wave can take one block, and B <= 32 KiB, DEFLATE's window, bounds every distance.
// A block becomes one byte-aligned segment, the smallest of two forms, or of three when the
// caller asks for it (zh_gzip_enc_params::dynamic = 1); stored wins a tie, fixed one against
// dynamic:
//   * fixed: header bits BFINAL 0, BTYPE 01; the fixed Huffman codes of RFC 1951 §3.2.6 (codes
//     MSB first, extra bits LSB first, in an LSB-first bit stream); the end-of-block code; an
//     empty stored block as a sync marker: bits 000, zero bits up to the byte boundary,
//     00 00 ff ff;
//   * stored: 00, LEN, NLEN, the block's bytes: 5 bytes over raw;
//   * dynamic: header bits BFINAL 0, BTYPE 10; the block's own length-limited Huffman codes
//     (code_lengths, plan_dynamic below), the symbols, the end-of-block code and the same sync
//     marker.  It is chosen only when strictly smaller than both other forms.
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
//   deflate_block_dynamic  the same walk with the dynamic form in the choice: the block's
//                  histogram first, then the exact sizes, then one table walk for either form.
// The output is a pure function of (input bytes, B, dynamic).  Callers zero zh_gzip_enc_params
// before they set a field: dynamic = 0 gives the two forms of before, byte for byte.
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
// The length code of 3..258 bytes less 257 (0..28), the number of its extra bits and their value;
// the distance code of 1..32768 (0..29) likewise.  The fixed coder, the histogram and the dynamic
// coder share them.
ZH_BS_HD uint32_t len_code(uint32_t len, uint32_t* eb, uint32_t* ex) {
  const uint32_t l = len - 3;
  uint32_t le = l < 8 ? 0 : highbit32(l) - 2;
  uint32_t lc = 4 * le + (l >> le);
  uint32_t lx = l & ((1u << le) - 1);
  if (len == kMaxMatch) lc = 28, le = 0, lx = 0;  // code 285
  *eb = le, *ex = lx;
  return lc;
}
ZH_BS_HD uint32_t dist_code(uint32_t dist, uint32_t* eb, uint32_t* ex) {
  const uint32_t d = dist - 1;
  const uint32_t de = d < 4 ? 0 : highbit32(d) - 1;
  *eb = de, *ex = d & ((1u << de) - 1);
  return 2 * de + (d >> de);
}
// (bits, count) of a match of 3..258 bytes at a distance of 1..32768: the length code
// (257..279: 7 bits from 0; 280..287: 8 bits from 0xC0), its extra bits, the 5-bit distance code,
// its extra bits: 31 bits at the most.
ZH_BS_HD uint32_t match_bits(uint32_t len, uint32_t dist, uint32_t* nb) {
  uint32_t le, lx, de, dx;
  const uint32_t lc = len_code(len, &le, &lx);
  const uint32_t dc = dist_code(dist, &de, &dx);
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

// ---- phase 2, the dynamic form ----------------------------------------------------------------
// Every rule of the dynamic form is stated here once, over a lane policy W (lane, W::n lanes,
// order(), sum()): the host runs it on OneLane, the device on a wave.  The steps marked "first
// lane" are short serial chains; the rest is spread over the lanes.
constexpr uint32_t kLitLen = 286, kDist = 30, kSyms = kLitLen + kDist, kClSyms = 19;
constexpr uint32_t kEob = 256;
constexpr uint32_t kMaxCount = 1u << 22;  // code_lengths sorts keys of count << 9 | symbol

// What one block's dynamic form needs: 7 244 bytes, in the wave's LDS on the device.
struct DynWork {
  uint32_t hist[kSyms];  // literal/length symbols 0..285, then the distance codes 0..29
  uint32_t tab[kSyms];   // per symbol: the code as the stream takes it | its length << 16
  uint32_t a[kLitLen];   // code_lengths: the keys of the used symbols, then the nodes' weights
  uint32_t b[kLitLen];   // code_lengths: the keys in ascending order
  uint32_t clhist[kClSyms], cltab[kClSyms];
  uint32_t cnt[16], next[16];  // codes per length, first code per length
  uint16_t par[2 * kLitLen];   // code_lengths: a node's parent, then its depth
  uint16_t items[kSyms];       // the header's code-length symbols: symbol | extra value << 5
  uint8_t lens[kSyms], cllens[kClSyms + 1];
  uint32_t used, ok, nitems, hlit, hdist, hclen, fixed_bits, dyn_bits, offered;
};
static_assert(sizeof(DynWork) == 7244, "the LDS budget of gzip_deflate_dyn_kernel");

struct OneLane {
  uint32_t lane = 0;
  static constexpr uint32_t n = 1;
  ZH_BS_HD void order() {}
  ZH_BS_HD uint32_t sum(uint32_t v) { return v; }
};

ZH_BS_HD uint32_t len_extra(uint32_t lc) { return lc < 8 || lc == 28 ? 0 : (lc >> 2) - 1; }
ZH_BS_HD uint32_t dist_extra(uint32_t dc) { return dc < 4 ? 0 : (dc >> 1) - 1; }
// the extra bits behind symbol s of DynWork::hist
ZH_BS_HD uint32_t sym_extra(uint32_t s) {
  return s <= kEob ? 0 : s < kLitLen ? len_extra(s - 257) : dist_extra(s - kLitLen);
}
ZH_BS_HD uint32_t cl_extra(uint32_t s) { return s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0; }
// the order the code-length code's lengths are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2
// 14 1 15, five bits each
ZH_BS_HD uint32_t cl_order(uint32_t i) {
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 |
                          9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 |
                          4ull << 55;
  constexpr uint64_t hi =
      12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}
// the table entry of symbol s under the fixed codes of RFC 1951 §3.2.6
ZH_BS_HD uint32_t fixed_entry(uint32_t s) {
  if (s < 144) return huff(0x30 + s, 8) | 8u << 16;
  if (s < 256) return huff(0x190 + (s - 144), 9) | 9u << 16;
  if (s < 280) return huff(s - 256, 7) | 7u << 16;
  if (s < kLitLen) return huff(0xC0 + (s - 280), 8) | 8u << 16;
  return huff(s - kLitLen, 5) | 5u << 16;
}
// (bits, count) of a symbol with table entry t followed by eb extra bits of value ex: 28 at most
ZH_BS_HD uint32_t entry_bits(uint32_t t, uint32_t ex, uint32_t eb, uint32_t* nb) {
  *nb = (t >> 16) + eb;
  return (t & 0xFFFFu) | ex << (t >> 16);
}

// The code lengths of a Huffman code over the symbols with counts[s] > 0 (counts <= kMaxCount,
// nsym <= 286, limit <= 15), none longer than `limit`: a pure function of the counts.
//   * no symbol used: all lengths 0; one used: that symbol gets length 1;
//   * the used symbols in ascending order of (count, symbol); Huffman's merge with two queues,
//     the leaves and the nodes made so far, a leaf before a node of equal weight: an optimal code;
//   * only the number of leaves at each depth is kept.  Depths past `limit` are folded into
//     `limit`; while the Kraft sum is above 1, the deepest leaf above row `limit` moves down one
//     row and a leaf of row `limit` moves up beside it, which takes 2^-limit off the sum;
//   * the lengths go out in the sorted order, the longest to the rarest: no symbol has a longer
//     code than a rarer one, and of two equally frequent symbols the lower has the longer code.
// False when no such code exists or an argument is out of range (never, from the callers here).
template <class W>
ZH_BS_HD bool code_lengths(const uint32_t* counts, uint32_t nsym, uint32_t limit, uint8_t* lens,
                           DynWork& d, W& w) {
  if (nsym > kLitLen || limit < 1 || limit > 15) return false;
  for (uint32_t s = w.lane; s < nsym; s += W::n) lens[s] = 0;
  if (w.lane == 0) {  // first lane: the keys of the used symbols
    uint32_t u = 0;
    bool ok = true;
    for (uint32_t s = 0; s < nsym; s++) {
      const uint32_t c = counts[s];
      if (c > kMaxCount) ok = false;
      if (c && ok) d.a[u++] = c << 9 | s;
    }
    d.used = u;
    d.ok = ok;
  }
  w.order();
  const uint32_t u = d.used;
  if (!d.ok || u > (1u << limit)) return false;
  if (u == 0) return true;
  if (u == 1) {
    if (w.lane == 0) lens[d.a[0] & 511u] = 1;
    w.order();
    return true;
  }
  for (uint32_t i = w.lane; i < u; i += W::n) {  // the keys differ: a key's rank is its place
    const uint32_t key = d.a[i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < u; j++) r += d.a[j] < key ? 1u : 0u;
    d.b[r] = key;
  }
  w.order();
  if (w.lane == 0) {  // first lane: leaves 0..u-1 in sorted order, node m is u + m, weight a[m]
    uint32_t li = 0, ii = 0;
    for (uint32_t m = 0; m + 1 < u; m++) {
      uint32_t sum = 0;
      for (int t = 0; t < 2; t++) {
        if (li < u && (ii >= m || (d.b[li] >> 9) <= d.a[ii])) {
          sum += d.b[li] >> 9;
          d.par[li++] = (uint16_t)(u + m);
        } else {
          sum += d.a[ii];
          d.par[u + ii++] = (uint16_t)(u + m);
        }
      }
      d.a[m] = sum;
    }
    for (uint32_t bl = 0; bl < 16; bl++) d.cnt[bl] = 0;
    d.par[2 * u - 2] = 0;  // the root; a parent comes after its children
    uint32_t kraft = 0;    // in units of 2^-limit
    for (uint32_t v = 2 * u - 2; v-- > 0;) {
      const uint32_t dep = d.par[d.par[v]] + 1u;
      d.par[v] = (uint16_t)dep;
      if (v < u) {
        const uint32_t bl = dep < limit ? dep : limit;
        d.cnt[bl]++;
        kraft += 1u << (limit - bl);
      }
    }
    bool ok = true;
    while (ok && kraft > (1u << limit)) {
      uint32_t bl = limit - 1;
      while (bl > 0 && d.cnt[bl] == 0) bl--;
      if (bl == 0 || d.cnt[limit] == 0) {
        ok = false;  // never: u <= 2^limit
        break;
      }
      d.cnt[bl]--, d.cnt[bl + 1] += 2, d.cnt[limit]--, kraft--;
    }
    uint32_t i = 0;
    for (uint32_t bl = limit; ok && bl >= 1; bl--)
      for (uint32_t c = d.cnt[bl]; c > 0 && i < u; c--) lens[d.b[i++] & 511u] = (uint8_t)bl;
    d.ok = ok && i == u && kraft == (1u << limit);
  }
  w.order();
  return d.ok != 0;
}

// First lane: the canonical codes (RFC 1951 §3.2.2) of nsym lengths into tab.
ZH_BS_HD void make_codes(const uint8_t* lens, uint32_t nsym, uint32_t* tab, DynWork& d) {
  for (uint32_t bl = 0; bl < 16; bl++) d.cnt[bl] = 0;
  for (uint32_t s = 0; s < nsym; s++) d.cnt[lens[s]]++;
  d.cnt[0] = 0;
  uint32_t code = 0;
  d.next[0] = 0;
  for (uint32_t bl = 1; bl < 16; bl++) d.next[bl] = code = (code + d.cnt[bl - 1]) << 1;
  for (uint32_t s = 0; s < nsym; s++) {
    const uint32_t bl = lens[s];
    tab[s] = bl ? huff(d.next[bl]++, bl) | bl << 16 : 0u;
  }
}

// The lengths the header describes, literal/length lengths first: runs cross the seam.
ZH_BS_HD uint32_t header_len(const DynWork& d, uint32_t hlit, uint32_t i) {
  return d.lens[i < hlit ? i : kLitLen + (i - hlit)];
}
ZH_BS_HD void header_item(DynWork& d, uint32_t sym, uint32_t ex) {
  d.items[d.nitems++] = (uint16_t)(sym | ex << 5);
  d.clhist[sym]++;
}

// From the block's histogram (hist; the end-of-block counted): the code lengths of both sets,
// the header, and the exact bits of the fixed and the dynamic form, each from its three header
// bits to its end-of-block code.
//   * the literal/length set holds two used symbols or more (a literal or a length, and the
//     end of block): it is complete.  One used distance code has length 1; no match: HDIST 0 and
//     one length of 0;
//   * HLIT and HDIST lose their trailing zero lengths; the HLIT + 257 + HDIST + 1 lengths are one
//     sequence, coded greedily: zero runs of 11..138 are symbol 18, of 3..10 symbol 17; another
//     length is sent once and its repeats in runs of 3..6 as symbol 16; what is left is sent
//     plain;
//   * the code-length code has at most 7 bits; HCLEN loses its trailing zeros in cl_order.  A
//     code-length code of one symbol is incomplete and zlib rejects it: the form is then not
//     offered (never: every header holds a length and something else).
template <class W>
ZH_BS_HD void plan_dynamic(DynWork& d, W& w) {
  uint32_t fx = 0;
  for (uint32_t s = w.lane; s < kSyms; s += W::n)
    fx += d.hist[s] * ((fixed_entry(s) >> 16) + sym_extra(s));
  fx = w.sum(fx);
  bool ok = code_lengths(d.hist, kLitLen, 15, d.lens, d, w);
  ok = code_lengths(d.hist + kLitLen, kDist, 15, d.lens + kLitLen, d, w) && ok;
  uint32_t dy = 0;
  for (uint32_t s = w.lane; s < kSyms; s += W::n) dy += d.hist[s] * (d.lens[s] + sym_extra(s));
  dy = w.sum(dy);
  if (w.lane == 0) {  // first lane: the header's symbols
    uint32_t hlit = kLitLen, hdist = kDist;
    while (hlit > 257 && d.lens[hlit - 1] == 0) hlit--;
    while (hdist > 1 && d.lens[kLitLen + hdist - 1] == 0) hdist--;
    d.hlit = hlit, d.hdist = hdist, d.nitems = 0;
    for (uint32_t s = 0; s < kClSyms; s++) d.clhist[s] = 0;
    const uint32_t total = hlit + hdist;
    for (uint32_t i = 0; i < total;) {
      const uint32_t v = header_len(d, hlit, i);
      uint32_t run = 1;
      while (i + run < total && header_len(d, hlit, i + run) == v) run++;
      i += run;
      if (v == 0) {
        for (uint32_t t; run >= 11; run -= t) header_item(d, 18, (t = run < 138 ? run : 138) - 11);
        if (run >= 3) header_item(d, 17, run - 3), run = 0;
      } else {
        header_item(d, v, 0);
        run--;
        for (uint32_t t; run >= 3; run -= t) header_item(d, 16, (t = run < 6 ? run : 6) - 3);
      }
      for (; run; run--) header_item(d, v, 0);
    }
  }
  w.order();
  ok = code_lengths(d.clhist, kClSyms, 7, d.cllens, d, w) && ok;
  if (w.lane == 0) {
    uint32_t hclen = kClSyms, hdr = 0, clused = 0;
    while (hclen > 4 && d.cllens[cl_order(hclen - 1)] == 0) hclen--;
    for (uint32_t s = 0; s < kClSyms; s++) {
      hdr += d.clhist[s] * (d.cllens[s] + cl_extra(s));
      clused += d.clhist[s] ? 1u : 0u;
    }
    d.hclen = hclen;
    d.fixed_bits = 3 + fx;
    d.dyn_bits = 3 + 14 + 3 * hclen + hdr + dy;
    d.offered = ok && clused >= 2 ? 1u : 0u;
  }
  w.order();
}

// The bytes of a fixed or dynamic segment of `bits` bits up to its end-of-block code: the three
// marker bits, zero bits to the byte boundary, 00 00 ff ff.
ZH_BS_HD uint32_t segment_bytes(uint32_t bits) { return (bits + 3 + 7) / 8 + 4; }

// The form of the block's segment and its size: the smallest of stored (0), fixed (1) and
// dynamic (2); stored wins a tie, fixed wins one against dynamic.
ZH_BS_HD uint32_t choose_form(uint32_t n, const DynWork& d, uint32_t* size) {
  uint32_t form = 0;
  *size = n + kStoredOver;
  if (segment_bytes(d.fixed_bits) < *size) form = 1, *size = segment_bytes(d.fixed_bits);
  if (d.offered && segment_bytes(d.dyn_bits) < *size) form = 2, *size = segment_bytes(d.dyn_bits);
  return form;
}

// The (code, length) tables of the chosen form into d.tab (and d.cltab).
template <class W>
ZH_BS_HD void form_tables(uint32_t form, DynWork& d, W& w) {
  if (form == 1) {
    for (uint32_t s = w.lane; s < kSyms; s += W::n) d.tab[s] = fixed_entry(s);
  } else if (w.lane == 0) {
    make_codes(d.lens, kLitLen, d.tab, d);
    make_codes(d.lens + kLitLen, kDist, d.tab + kLitLen, d);
    make_codes(d.cllens, kClSyms, d.cltab, d);
  }
  w.order();
}

// The host's histogram walk: every literal, the length code of every piece and its distance
// code, one end-of-block.  False when the records do not partition the block (never).
inline bool hist_block(const uint8_t* s, uint32_t n, const uint16_t* seq, uint32_t ns,
                       DynWork& d) {
  for (uint32_t i = 0; i < kSyms; i++) d.hist[i] = 0;
  uint32_t pos = 0;
  for (uint32_t k = 0; k <= ns; k++) {
    const uint32_t lit = k < ns ? seq[3 * k] : n - pos;
    if (lit > n - pos) return false;
    for (uint32_t i = 0; i < lit; i++) d.hist[s[pos + i]]++;
    pos += lit;
    if (k == ns) break;
    const uint32_t ml = seq[3 * k + 1], off = seq[3 * k + 2];
    if (ml < kMinPiece || ml > n - pos || off == 0 || off > pos) return false;
    uint32_t eb, ex;
    for (uint32_t j = 0, np = piece_count(ml); j < np; j++)
      d.hist[257 + len_code(piece_len(ml, j), &eb, &ex)]++;
    d.hist[kLitLen + dist_code(off, &eb, &ex)] += piece_count(ml);
    pos += ml;
  }
  d.hist[kEob] = 1;
  return true;
}

// deflate_block with the dynamic form in the choice: the size of the block's segment, written
// to out (room for n + 4 bytes) unless it is stored.  The sizes are known before a bit is
// written; the fixed form comes out of the same table walk as the dynamic one.
inline uint32_t deflate_block_dynamic(const uint8_t* s, uint32_t n, const uint16_t* seq,
                                      uint32_t ns, uint32_t covered, uint8_t* out, DynWork& d) {
  const uint32_t stored = n + kStoredOver;
  if (covered > n || !hist_block(s, n, seq, ns, d)) return stored;
  OneLane w;
  plan_dynamic(d, w);
  uint32_t size = 0, nb = 0;
  const uint32_t form = choose_form(n, d, &size);
  if (form == 0) return stored;
  form_tables(form, d, w);
  BitOut b{out, 0, stored - 1};
  b.add(form == 2 ? 4 : 2, 3);  // BFINAL 0, BTYPE 10 or 01
  if (form == 2) {
    b.add((d.hlit - 257) | (d.hdist - 1) << 5 | (d.hclen - 4) << 10, 14);
    for (uint32_t i = 0; i < d.hclen; i++) b.add(d.cllens[cl_order(i)], 3);
    for (uint32_t i = 0; i < d.nitems; i++) {
      const uint32_t sym = d.items[i] & 31u;
      const uint32_t v = entry_bits(d.cltab[sym], d.items[i] >> 5, cl_extra(sym), &nb);
      b.add(v, nb);
    }
  }
  uint32_t pos = 0;
  for (uint32_t k = 0; k <= ns; k++) {
    const uint32_t lit = k < ns ? seq[3 * k] : n - pos;
    for (uint32_t i = 0; i < lit; i++) b.add(d.tab[s[pos + i]] & 0xFFFFu, d.tab[s[pos + i]] >> 16);
    pos += lit;
    if (k == ns) break;
    const uint32_t ml = seq[3 * k + 1], off = seq[3 * k + 2];
    for (uint32_t j = 0, np = piece_count(ml); j < np; j++) {
      uint32_t eb, ex;
      const uint32_t lc = len_code(piece_len(ml, j), &eb, &ex);
      uint32_t v = entry_bits(d.tab[257 + lc], ex, eb, &nb);
      b.add(v, nb);
      const uint32_t dc = dist_code(off, &eb, &ex);
      v = entry_bits(d.tab[kLitLen + dc], ex, eb, &nb);
      b.add(v, nb);
    }
    pos += ml;
  }
  b.add(d.tab[kEob] & 0xFFFFu, d.tab[kEob] >> 16);
  b.add(0, 3);  // the marker: BFINAL 0, BTYPE 00
  if (b.cnt) b.add(0, 8 - b.cnt);
  b.add(0xFFFF0000u, 32);  // LEN 0, NLEN ffff
  return b.over || b.o != size ? stored : b.o;  // never stored here: the sizes are exact
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
// LEN, NLEN of a stored segment as one little-endian word
inline uint32_t stored_word(uint32_t len) { return len | ((~len & 0xFFFFu) << 16); }
// A stored segment: 00, LEN, NLEN, the block's n bytes: n + kStoredOver bytes at d.
inline void put_stored(uint8_t* d, const uint8_t* s, uint32_t n) {
  const uint32_t word = stored_word(n);
  d[0] = 0;
  for (int i = 0; i < 4; i++) d[1 + i] = (uint8_t)(word >> (8 * i));
  for (uint32_t q = 0; q < n; q++) d[kStoredOver + q] = s[q];
}
// The final empty fixed block that ends the segments: kEnding bytes (the zlib streams of the
// blosc writer, zh_blosc_enc.h, end with the same two).
inline void put_final(uint8_t* d) { d[0] = 3, d[1] = 0; }
// 03 00, CRC-32, ISIZE: kEnding + kTrailer bytes
inline void put_ending(uint8_t* d, uint32_t crc, size_t n) {
  put_final(d);
  for (int i = 0; i < 4; i++) d[2 + i] = (uint8_t)(crc >> (8 * i));
  for (int i = 0; i < 4; i++) d[6 + i] = (uint8_t)((uint64_t)n >> (8 * i));
}

struct Params {
  uint32_t B = kDefaultBlock;
  bool dynamic = false;
};
inline bool read_params(const zh_gzip_enc_params* p, Params* out) {
  if (!p || p->blocksize < 0 || (p->dynamic != 0 && p->dynamic != 1)) return false;
  out->B = block_bytes(p->blocksize);
  out->dynamic = p->dynamic == 1;
  return true;
}
// read_params refused the `dynamic` field, not the block size
inline bool bad_dynamic(const zh_gzip_enc_params* p) {
  return p && p->blocksize >= 0 && p->dynamic != 0 && p->dynamic != 1;
}

// One block (s, bsz) as its segment at d (room for bsz + kStoredOver bytes) on the host: the
// records into seq (3 * (bsz / 4) + 3 uint16), the smallest form written, the stored one when
// no other is smaller.  dyn: the work of the dynamic form, or null (stored and fixed only).
// Returns the segment's size.
inline uint32_t put_segment(const uint8_t* s, uint32_t bsz, uint8_t* d, uint16_t* seq,
                            uint32_t* table, zh_lz::HostLanes& w, DynWork* dyn) {
  uint32_t covered = 0;
  const uint32_t ns = match_block(s, bsz, seq, table, w, &covered);
  const uint32_t size = dyn ? deflate_block_dynamic(s, bsz, seq, ns, covered, d, *dyn)
                            : deflate_block(s, bsz, seq, ns, covered, d);
  if (size == bsz + kStoredOver) put_stored(d, s, bsz);
  return size;
}

// One member on the host with HostLanes.  dst == nullptr: *len = the bound.
inline int compress_member(const uint8_t* src, size_t n, const zh_gzip_enc_params* prm,
                           uint8_t* dst, size_t cap, size_t* len, const char** msg) {
  Params P;
  if (!read_params(prm, &P) || (n > 0 && !src) || !len) {
    *msg = bad_dynamic(prm) ? "zh_gzip_compress: dynamic is 0 or 1"
                            : "zh_gzip_compress: blocksize >= 0";
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
  uint16_t* seq = new uint16_t[3 * (size_t)(P.B / 4) + 3];
  uint32_t* table = new uint32_t[zh_lz::kHashSize];
  DynWork* dyn = P.dynamic ? new DynWork : nullptr;
  zh_lz::HostLanes w;
  w.wide = true;
  put_header(dst);
  size_t p = kHeader;
  for (size_t k = 0; k < nb; k++)  // the bound leaves every segment its stored size
    p += put_segment(src + k * P.B, block_size(n, P.B, k), dst + p, seq, table, w, dyn);
  put_ending(dst + p, crc_finish(crc_raw(0, src, n), n), n);
  p += kEnding + kTrailer;
  delete dyn;
  delete[] table;
  delete[] seq;
  if (p > bound) {
    *msg = "zh_gzip_compress: layout and bound disagree";
    return ZH_EINVAL;
  }
  *len = p;
  return ZH_OK;
}

}  // namespace zh_gz
