// zh_zstd_enc.h — the zstd frame writer shared by the host and the device (RFC 8878 as
// zh_zstd.cpp reads it; libzstd is the independent reader).
//
// Frame: magic, descriptor (8-byte content size, single segment, checksum flag, no dictionary),
// the blocks, then the low 32 bits of XXH64(content, 0) when the checksum is on: the header
// zh_zstd_compress_raw writes.  One chunk is one frame.
// Blocks: the content is cut into blocks of B bytes (the last one shorter); each is compressed
// on its own: no match reaches before the block's first byte and no repeat-offset code is
// written (every offset is offset_value = offset + 3), so one wave can take one block.
//   * compressed block (type 2): raw literals under the 3-byte header (size format 3, 20-bit
//     size: the literals start at a fixed place and are written while matching), the sequence
//     count in its 1- or 2-byte form, the modes byte 0 (predefined tables for literal lengths,
//     offsets and match lengths), then the FSE bitstream: sequences last first, extra bits and
//     state bits in the reverse of the order decode_block (zh_zstd_dec.h) consumes them, the
//     three states, the 1-bit end marker;
//   * a block whose compressed form would reach its raw size is raw (type 0); neighbouring raw
//     blocks are merged and cut every 128 KiB, so a frame in which nothing compresses is, byte
//     for byte, what zh_zstd_compress_raw writes; a frame that would reach that size is written
//     that way as well, so no frame is larger;
//   * no RLE blocks, no RLE or Huffman literals; `level` is not honoured.
// Two phases per block, because sequences are coded in reverse:
//   match_block   over a lane policy W (zh_lz_match.h): literals to the block's output region,
//                 (literal length, match length, offset) records, 3 x uint16, to a list.  A
//                 sequence covers kMinMatch bytes or more, which bounds the list at n / 4;
//   fse_block     serial: walks the list backwards through the three FSE encoders into a
//                 64-bit accumulator flushed in whole bytes after every field (the widest
//                 sequence is 16 + 16 + 16 extra bits and 6 + 6 + 5 state bits).
// The encoding tables (Tables) are derived once on the host, in zh_zstd.cpp, from the fse_build
// the decoder runs on the predefined distributions: for a symbol, the decode-table states that
// carry it partition the next-state range, so (symbol, next state) -> state is one lookup and
// encoder and decoder agree by construction.
// The output is a pure function of (input bytes, B, checksum flag).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "zh_lz_match.h"

namespace zh_ze {

constexpr uint32_t kMaxBlock = zh_lz::kMaxBlock;  // 64 KiB: positions and lengths fit 16 bits
constexpr uint32_t kMinBlock = 1u << 10;
constexpr uint32_t kDefaultBlock = 16u << 10;  // DESIGN.md "Zstd frames encoded on the device"
constexpr uint32_t kRawBlock = 128u << 10;     // Block_Maximum_Size
constexpr uint32_t kRaw = 0xFFFFFFFFu;         // match_block: store the block raw
constexpr size_t kFrameHeader = 4 + 1 + 8;
// the 3-byte form of the sequence count starts at 0x7F00 sequences: never reached
static_assert(kMaxBlock / zh_lz::kMinMatch < 0x7F00, "a block can pass the 2-byte sequence count");

// What the encoder needs of the three predefined FSE tables (accuracy 6 / 6 / 5) and of the
// length codes.  POD: uploaded as it is.
struct Tables {
  uint8_t ll_state[36][64], ml_state[53][64], of_state[29][32];  // (symbol, next state) -> state
  uint8_t ll_first[36], ml_first[53], of_first[29];  // the lowest state carrying the symbol
  uint8_t ll_nb[64], ml_nb[64], of_nb[32];           // decode table: bits read at a state
  uint16_t ll_base[64], ml_base[64], of_base[32];    // decode table: next-state base
  uint8_t ll_code[64], ml_code[128];                 // codes of ll < 64 and of ml - 3 < 128
  uint8_t ll_cbits[36], ml_cbits[53];                // extra bits per code
  uint32_t ll_cbase[36], ml_cbase[53];               // first value per code
};
// Built once from zh_zd::fse_build (in zh_zstd.cpp).
const Tables& tables();

ZH_BS_HD uint32_t highbit32(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// Block size of a configuration: 0 is the default; other values are advice, as blosc's.
ZH_BS_HD uint32_t block_bytes(int32_t configured) {
  if (configured <= 0) return kDefaultBlock;
  return (uint32_t)configured < kMinBlock   ? kMinBlock
         : (uint32_t)configured > kMaxBlock ? kMaxBlock
                                            : (uint32_t)configured;
}

// Phase 1.  s: the block (n <= kMaxBlock bytes); lits: room for n bytes (the block's output
// region + 3); seq: room for 3 * (n / 4) uint16; table: kHashSize slots.  Returns the number of
// sequences and *nlit, or kRaw as soon as the literals and a lower bound of 12 bits per
// sequence reach the raw size (nothing is written past lits[n - 4]).
template <class W>
ZH_BS_HD uint32_t match_block(const uint8_t* s, uint32_t n, uint8_t* lits, uint16_t* seq,
                              uint32_t* table, W& w, uint32_t* nlit) {
  if (n < 16 || n > kMaxBlock) return kRaw;
  w.clear(table);
  const uint32_t lim = n - 4;  // the last position 4 bytes can be read at
  uint32_t p = 0, a = 0, nl = 0, ns = 0;
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
    const uint32_t lit = m - a;
    if (3 + nl + lit + 3 + ns + (ns >> 1) >= n) return kRaw;
    w.copy(lits + nl, s + a, lit);
    nl += lit;
    w.put16(seq + 3 * ns, lit);
    w.put16(seq + 3 * ns + 1, ml);  // m >= 1: ml <= 65535
    w.put16(seq + 3 * ns + 2, m - ref);
    ns++;
    w.insert(p, m + ml < lim + 1 ? m + ml : lim + 1, table);
    p = a = m + ml;
  }
  const uint32_t tail = n - a;
  if (3 + nl + tail + 3 + ns + (ns >> 1) >= n) return kRaw;
  w.copy(lits + nl, s + a, tail);
  *nlit = nl + tail;
  return ns;
}

// LSB-first bit writer of a stream that is read backwards; stops at cap.
struct BitWriter {
  uint8_t* d;
  uint32_t o, cap;
  uint64_t acc = 0;
  uint32_t cnt = 0;
  bool over = false;
  ZH_BS_HD void add(uint32_t v, uint32_t nb) {
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

// Phase 2.  out: the block's output region (n bytes), its literals already at out + 3.  Returns
// the size of the compressed block, or n when it would reach n (the block is stored raw).
ZH_BS_HD uint32_t fse_block(const Tables& T, const uint16_t* seq, uint32_t ns, uint32_t nl,
                            uint8_t* out, uint32_t n) {
  if (ns == 0 || ns == kRaw || 3 + nl + 4 >= n) return n;
  out[0] = (uint8_t)((3u << 2) | ((nl & 15u) << 4));  // Raw_Literals_Block, size format 3
  out[1] = (uint8_t)(nl >> 4);
  out[2] = (uint8_t)(nl >> 12);
  uint32_t o = 3 + nl;
  if (ns < 128) {
    out[o++] = (uint8_t)ns;
  } else {
    out[o++] = (uint8_t)((ns >> 8) + 128);
    out[o++] = (uint8_t)(ns & 255u);
  }
  out[o++] = 0;  // Predefined_Mode three times
  BitWriter b{out, o, n - 1};
  uint32_t sll = 0, sml = 0, sof = 0;
  for (uint32_t k = ns; k-- > 0;) {
    const uint32_t ll = seq[3 * k], ml = seq[3 * k + 1], ofv = (uint32_t)seq[3 * k + 2] + 3;
    const uint32_t llc = ll < 64 ? T.ll_code[ll] : highbit32(ll) + 19;
    const uint32_t mb = ml - 3;
    const uint32_t mlc = mb < 128 ? T.ml_code[mb] : highbit32(mb) + 36;
    const uint32_t ofc = highbit32(ofv);
    if (k == ns - 1) {  // the states the decoder ends in: nothing is read after them
      sll = T.ll_first[llc], sml = T.ml_first[mlc], sof = T.of_first[ofc];
    } else {  // the decoder updates LL, ML, OF: written OF, ML, LL
      uint32_t t = T.of_state[ofc][sof];
      b.add(sof - T.of_base[t], T.of_nb[t]);
      sof = t;
      t = T.ml_state[mlc][sml];
      b.add(sml - T.ml_base[t], T.ml_nb[t]);
      sml = t;
      t = T.ll_state[llc][sll];
      b.add(sll - T.ll_base[t], T.ll_nb[t]);
      sll = t;
    }
    // the decoder reads the extra bits of OF, ML, LL: written LL, ML, OF
    b.add(ll - T.ll_cbase[llc], T.ll_cbits[llc]);
    b.add(ml - T.ml_cbase[mlc], T.ml_cbits[mlc]);
    b.add(ofv - (1u << ofc), ofc);
    if (b.over) return n;
  }
  b.add(sml, 6);  // the decoder starts with LL, OF, ML
  b.add(sof, 5);
  b.add(sll, 6);
  b.add(1, 1);  // the end marker
  b.add(0, 7);  // flushes the last partial byte (a whole zero byte is never written: cnt < 8)
  if (b.over) return n;
  return b.o;
}

// ---- frame layout ---------------------------------------------------------------------------
inline size_t raw_frame_size(size_t n, bool checksum) {
  const size_t nblk = n == 0 ? 1 : (n + kRawBlock - 1) / kRawBlock;
  return kFrameHeader + 3 * nblk + n + (checksum ? 4 : 0);
}
inline size_t block_count(size_t n, uint32_t B) { return (n + B - 1) / B; }
inline uint32_t block_size(size_t n, uint32_t B, size_t k) {
  const size_t rest = n - k * B;
  return rest < B ? (uint32_t)rest : B;
}
ZH_BS_HD void put_frame_header(uint8_t* d, size_t n, bool checksum) {
  d[0] = 0x28, d[1] = 0xB5, d[2] = 0x2F, d[3] = 0xFD;
  d[4] = (uint8_t)((3u << 6) | (1u << 5) | (checksum ? 4u : 0u));  // 8-byte FCS, single segment
  for (int i = 0; i < 8; i++) d[5 + i] = (uint8_t)((uint64_t)n >> (8 * i));
}
ZH_BS_HD uint32_t block_header(uint32_t size, uint32_t type, bool last) {
  return (size << 3) | (type << 1) | (last ? 1u : 0u);
}

// The blocks of a frame in order.  cs[k]: the compressed size of block k, or its raw size (or
// more) when it is stored raw; all_raw: every block is.  E:
//     void raw(uint32_t header, size_t offset, uint32_t len)   content bytes as they are
//     void comp(uint32_t header, size_t k, uint32_t len)       the compressed form of block k
template <class E>
inline void walk_blocks(size_t n, uint32_t B, const uint32_t* cs, bool all_raw, E& e) {
  if (n == 0) {
    e.raw(block_header(0, 0, true), 0, 0);
    return;
  }
  const size_t nb = block_count(n, B);
  auto is_raw = [&](size_t k) { return all_raw || cs[k] >= block_size(n, B, k); };
  for (size_t k = 0; k < nb;) {
    if (!is_raw(k)) {
      e.comp(block_header(cs[k], 2, k + 1 == nb), k, cs[k]);
      k++;
      continue;
    }
    size_t k2 = k;
    while (k2 < nb && is_raw(k2)) k2++;
    const size_t end = k2 * B < n ? k2 * B : n;
    for (size_t o = k * (size_t)B; o < end;) {  // the run, cut every 128 KiB
      const uint32_t len = end - o < kRawBlock ? (uint32_t)(end - o) : kRawBlock;
      e.raw(block_header(len, 0, o + len == n), o, len);
      o += len;
    }
    k = k2;
  }
}

struct Sizer {
  size_t total = 0;
  void raw(uint32_t, size_t, uint32_t len) { total += 3 + (size_t)len; }
  void comp(uint32_t, size_t, uint32_t len) { total += 3 + (size_t)len; }
};
// Size of the frame and whether it is written all raw (cs == nullptr: it is).
inline size_t frame_size(size_t n, uint32_t B, const uint32_t* cs, bool checksum, bool* all_raw) {
  const size_t rawsz = raw_frame_size(n, checksum);
  *all_raw = true;
  if (!cs || n == 0) return rawsz;
  Sizer sz;
  walk_blocks(n, B, cs, false, sz);
  const size_t total = kFrameHeader + sz.total + (checksum ? 4 : 0);
  if (total >= rawsz) return rawsz;
  *all_raw = false;
  return total;
}

struct HostEmit {
  uint8_t* d;
  size_t p;
  const uint8_t* src;
  const uint8_t* scratch;
  uint32_t B;
  void head(uint32_t h) {
    d[p] = (uint8_t)h, d[p + 1] = (uint8_t)(h >> 8), d[p + 2] = (uint8_t)(h >> 16);
    p += 3;
  }
  void raw(uint32_t h, size_t off, uint32_t len) {
    head(h);
    for (uint32_t q = 0; q < len; q++) d[p + q] = src[off + q];
    p += len;
  }
  void comp(uint32_t h, size_t k, uint32_t len) {
    head(h);
    for (uint32_t q = 0; q < len; q++) d[p + q] = scratch[k * B + q];
    p += len;
  }
};

struct Params {
  bool checksum = true;
  uint32_t B = kDefaultBlock;
};
inline bool read_params(const zh_zstd_enc_params* p, Params* out) {
  if (!p || p->blocksize < 0 || (p->checksum != 0 && p->checksum != 1)) return false;
  out->checksum = p->checksum == 1;
  out->B = block_bytes(p->blocksize);
  return true;
}

// One frame on the host with HostLanes.  dst == nullptr: *len = the bound (the raw-block frame).
inline int compress_frame(const Tables& T, const uint8_t* src, size_t n,
                          const zh_zstd_enc_params* prm, uint8_t* dst, size_t cap, size_t* len,
                          const char** msg) {
  Params P;
  if (!read_params(prm, &P) || (n > 0 && !src) || !len) {
    *msg = "zh_zstd_compress: checksum 0 or 1, blocksize >= 0";
    return ZH_EINVAL;
  }
  const size_t bound = raw_frame_size(n, P.checksum);
  if (!dst) {
    *len = bound;
    return ZH_OK;
  }
  if (cap < bound) {
    *msg = "zh_zstd_compress: destination smaller than the bound";
    return ZH_EINVAL;
  }
  const size_t nb = block_count(n, P.B);
  uint8_t* scratch = new uint8_t[n ? n : 1];
  uint16_t* seq = new uint16_t[3 * (size_t)(P.B / 4) + 3];
  uint32_t* table = new uint32_t[zh_lz::kHashSize];
  uint32_t* cs = new uint32_t[nb ? nb : 1];
  zh_lz::HostLanes w;
  w.wide = true;
  for (size_t k = 0; k < nb; k++) {
    const uint32_t bsz = block_size(n, P.B, k);
    uint8_t* out = scratch + k * P.B;
    uint32_t nl = 0;
    const uint32_t ns = match_block(src + k * P.B, bsz, out + 3, seq, table, w, &nl);
    cs[k] = fse_block(T, seq, ns, nl, out, bsz);
  }
  bool all_raw;
  const size_t total = frame_size(n, P.B, cs, P.checksum, &all_raw);
  put_frame_header(dst, n, P.checksum);
  HostEmit e{dst, kFrameHeader, src, scratch, P.B};
  walk_blocks(n, P.B, cs, all_raw, e);
  if (P.checksum) {
    const uint32_t h = (uint32_t)zh_xxh64(src, n, 0);
    for (int i = 0; i < 4; i++) dst[e.p++] = (uint8_t)(h >> (8 * i));
  }
  delete[] cs;
  delete[] table;
  delete[] seq;
  delete[] scratch;
  if (e.p != total) {
    *msg = "zh_zstd_compress: layout and size disagree";
    return ZH_EINVAL;
  }
  *len = total;
  return ZH_OK;
}

}  // namespace zh_ze
