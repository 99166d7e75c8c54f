// zh_blosc_enc.h — the blosc1 frame writer shared by the host and the device: LZ4 streams,
// (ZH_BLOSC_ENC_ZSTD) zstd streams or (ZH_BLOSC_ENC_ZLIB) zlib streams.
//
// The writer emits what zh_blosc_streams.h reads (build_table is the contract): version 2,
// versionlz 1, compressor code 1 (LZ4), 3 (zlib) or 4 (zstd: with_compressor), flags 0x01 byte shuffle /
// 0x04 bit shuffle (format-2 rule: kShufBit2) / 0x10 blocks not split, the block starts, then per
// stream an int32 csize and the payload.  This header holds what both sides need, and nothing
// that needs a device:
//   * make_layout: block size, split rule and flags of a frame of n bytes;
//   * shuffled_byte_at: byte o of the shuffled block, read from the raw block (the inverse of
//     zh_bs::unshuffle_byte_at);
//   * encode_stream: one stream (s, n) -> LZ4 bytes, written once over a lane policy W: the
//     match finder, its determinism rule and the policy's members are stated in zh_lz_match.h
//     (HostLanes there, the kernel's WaveLanes in zh_enc_device.h), so the output is a pure
//     function of (input bytes, n).  A stream whose encoding would reach its raw size returns
//     n before writing past out[n - 1]: the caller stores it raw;
//   * compress_frame: the whole frame on the host with HostLanes (zh_blosc_compress[_ex], the
//     kernels' byte-for-byte oracle, tools/blosc_enc_check.cpp and blosc_zstd_enc_check.cpp
//     under sanitizers) over a stream coder: Lz4Coder (encode_stream), ZstdCoder or ZlibCoder.
// Zstd streams (compressor code 4): the layout, the shuffles and the split rule are the LZ4
// writer's.  A stream's payload is, byte for byte, the frame zh_zstd_compress writes for the
// shuffled bytes with checksum 0 and block size 64 KiB: the 13-byte header with the 8-byte
// content size, then one compressed block under its 3-byte header (a stream is at most 64 KiB:
// always one block), zh_ze::match_block and zh_ze::fse_block behind kZstdHead bytes.  A stream
// whose kZstdHead + block size would reach its raw size is stored raw (zstd_stream_size).
// Zlib streams (compressor code 3): again the LZ4 writer's layout.  A stream's payload is one
// RFC 1950 stream: 78 01 (CM 8, CINFO 7, FLEVEL 0, no dictionary), then what the gzip member
// writer (zh_gzip_enc.h) puts between its header and its trailer for the shuffled bytes with
// blocks of zh_gz::kDefaultBlock bytes: one byte-aligned segment per 16 KiB piece (stored or
// fixed; with ZH_BLOSC_ENC_DYNAMIC the dynamic form is in the choice) and the final empty fixed
// block 03 00; then the Adler-32 of the shuffled bytes, big-endian.  No match crosses a piece.
// A stream whose payload would reach its raw size is stored raw (zlib_stream_size).
// LZ4 end rules (liblz4 decodes the streams): the last 5 bytes are literals, no match starts
// within the last 12 bytes, a stream shorter than 13 bytes is never encoded, offsets are
// 1..65535 (a stream is at most 64 KiB).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "zh_blosc_streams.h"
#include "zh_gzip_enc.h"
#include "zh_lz_match.h"
#include "zh_zstd_enc.h"

namespace zh_be {

// the match finder and its host lane policy: zh_lz_match.h, shared with the zstd writer
using zh_lz::HostLanes;
using zh_lz::hash4;
using zh_lz::kHashBits;
using zh_lz::kHashSize;
using zh_lz::kMaxBlock;  // kLdsBlock of the decoder: blocks stay in LDS
using zh_lz::ld32;

constexpr uint32_t kDefaultBlock = 16u << 10;  // DESIGN.md "Blosc frames encoded on the device"
constexpr size_t kMaxFrame = 0x7fffffffu - 16;   // blosc1: nbytes + 16 fits an int32

struct Layout {
  uint32_t typesize = 1, shuffle = 0 /* zh_bs::Shuffle */, blocksize = 0, nblocks = 0, flags = 0;
  bool split = false;
};

inline int make_layout(size_t n, const zh_blosc_enc_params* p, Layout* L) {
  if (!p || p->typesize < 1 || p->typesize > 255 || p->shuffle < 0 || p->shuffle > 2 ||
      p->blocksize < 0 || n > kMaxFrame)
    return ZH_EINVAL;
  const uint32_t ts = (uint32_t)p->typesize;
  size_t bs = p->blocksize > 0 ? (size_t)p->blocksize : kDefaultBlock;
  if (bs > kMaxBlock) bs = kMaxBlock;  // blosc treats the configured block size as advice
  if (bs > n) bs = n;
  if (bs > ts) bs = bs / ts * ts;
  L->typesize = ts;
  L->shuffle = p->shuffle == 1 ? zh_bs::kShufByte : (p->shuffle == 2 ? zh_bs::kShufBit2
                                                                      : zh_bs::kShufNone);
  L->blocksize = (uint32_t)bs;
  L->nblocks = bs ? (uint32_t)((n + bs - 1) / bs) : 0;
  L->split = p->shuffle == 1 && ts <= 16 && bs / ts >= 128;
  L->flags = (1u << 5) | (p->shuffle == 1 ? 0x01u : 0u) | (p->shuffle == 2 ? 0x04u : 0u) |
             (L->split ? 0u : 0x10u);
  return ZH_OK;
}

// The layout with another compressor code in the flags (1 LZ4, 3 zlib, 4 zstd).
inline void with_compressor(Layout* L, uint32_t code) {
  L->flags = (L->flags & 0x1Fu) | (code << 5);
}

// Size and stream count of block k (a leftover block is never split).
inline uint32_t block_size(const Layout& L, size_t n, uint32_t k) {
  const size_t rest = n - (size_t)k * L.blocksize;
  return rest < L.blocksize ? (uint32_t)rest : L.blocksize;
}
inline uint32_t block_streams(const Layout& L, uint32_t bsz) {
  return L.split && bsz == L.blocksize ? L.typesize : 1;
}

// Byte o of the shuffled form of the raw block `in` of `size` bytes.
ZH_BS_HD uint8_t shuffled_byte_at(const uint8_t* in, uint32_t o, uint32_t size, uint32_t ts,
                                  uint32_t shuffle) {
  if (shuffle == zh_bs::kShufByte) {
    const uint32_t ne = size / ts;
    if (o >= ne * ts) return in[o];
    return in[(o % ne) * ts + o / ne];
  }
  if (shuffle == zh_bs::kShufBit2 || shuffle == zh_bs::kShufBit3) {
    const uint32_t ne = zh_bs::bitshuffle_elems(size, ts, shuffle);
    if (o >= ne * ts) return in[o];
    const uint32_t rowb = ne / 8, row = o / rowb, p = o % rowb, j = row / 8, k = row % 8;
    uint32_t v = 0;
    for (uint32_t m = 0; m < 8; m++) v |= ((in[(size_t)(8 * p + m) * ts + j] >> k) & 1u) << m;
    return (uint8_t)v;
  }
  return in[o];
}

// bytes a length beyond the token's 4 bits takes (0 below 15)
ZH_BS_HD uint32_t len_extra(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }

// One LZ4 sequence at out + o: token, literal length, literals, then (ml != 0) offset and match
// length.  The caller has checked the room.
template <class W>
ZH_BS_HD uint32_t put_sequence(uint8_t* out, uint32_t o, const uint8_t* lits, uint32_t lit,
                               uint32_t off, uint32_t ml, W& w) {
  const uint32_t mcode = ml ? ml - 4 : 0;
  w.put(out + o, ((lit < 15 ? lit : 15u) << 4) | (mcode < 15 ? mcode : 15u));
  o++;
  if (lit >= 15) {
    w.lenbytes(out + o, lit - 15);
    o += len_extra(lit);
  }
  w.copy(out + o, lits, lit);
  o += lit;
  if (ml) {
    w.put(out + o, off & 255u);
    w.put(out + o + 1, off >> 8);
    o += 2;
    if (mcode >= 15) {
      w.lenbytes(out + o, mcode - 15);
      o += len_extra(mcode);
    }
  }
  return o;
}

// The stream (s, n) as LZ4 into out (room for n bytes); table: kHashSize slots.  Returns the
// encoded size, or n when the encoding would reach n (out then holds nothing of use: the
// caller stores the stream raw).
template <class W>
ZH_BS_HD uint32_t encode_stream(const uint8_t* s, uint32_t n, uint8_t* out, uint32_t* table,
                                W& w) {
  if (n < 13 || n > kMaxBlock) return n;
  w.clear(table);
  const uint32_t lim = n - 13;  // the last position a match may start at
  const uint32_t mend = n - 5;  // a match ends at or before this
  uint32_t p = 0, a = 0, o = 0;
  while (p <= lim) {
    uint32_t ref = 0;
    const uint32_t lane = w.find(s, p, lim, table, &ref);
    if (lane == 64) {
      w.insert(p, lim + 1, table);
      p += 64;
      continue;
    }
    const uint32_t m = p + lane;
    const uint32_t ml = 4 + w.extend(s, ref + 4, m + 4, mend - (m + 4));
    const uint32_t lit = m - a;
    const uint32_t need = 1 + len_extra(lit) + lit + 2 + len_extra(ml - 4);
    if (o + need >= n) return n;
    o = put_sequence(out, o, s + a, lit, m - ref, ml, w);
    w.insert(p, m + ml < lim + 1 ? m + ml : lim + 1, table);
    p = a = m + ml;
  }
  const uint32_t lit = n - a;
  if (o + 1 + len_extra(lit) + lit >= n) return n;
  return put_sequence(out, o, s + a, lit, 0, 0, w);
}

inline void wr32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

inline void put_header(uint8_t* d, const Layout& L, uint32_t flags, size_t n, size_t cbytes) {
  d[0] = 2, d[1] = 1, d[2] = (uint8_t)flags, d[3] = (uint8_t)L.typesize;
  wr32(d + 4, (uint32_t)n);
  wr32(d + 8, L.blocksize);
  wr32(d + 12, (uint32_t)cbytes);
}
// flags of a frame written MEMCPYED (the shuffle bits stay as configured; readers ignore them)
inline uint32_t memcpyed_flags(const Layout& L) { return (L.flags & ~0x10u) | 0x02u; }

// ---- zstd streams ---------------------------------------------------------------------------
// What stands before a stream's compressed block: the zstd frame header and the block header.
constexpr uint32_t kZstdHead = (uint32_t)zh_ze::kFrameHeader + 3;
// Stored size of a stream of neb raw bytes whose compressed block has cs bytes (cs >= neb: there
// is none): neb says the stream is stored raw.
ZH_BS_HD uint32_t zstd_stream_size(uint32_t neb, uint32_t cs) {
  return cs < neb && kZstdHead + cs < neb ? kZstdHead + cs : neb;
}

// ---- zlib streams ---------------------------------------------------------------------------
constexpr uint32_t kZlibPiece = zh_gz::kDefaultBlock;  // a stream of 64 KiB is four segments
// What a stream carries besides its segments: 78 01, 03 00 and the Adler-32.
constexpr uint32_t kZlibOver = 2 + (uint32_t)zh_gz::kEnding + 4;
// Room a stream's payload needs beyond its raw size: kZlibOver and the stored segments' headers.
constexpr uint32_t kZlibHead = kZlibOver + zh_gz::kStoredOver * (kMaxBlock / kZlibPiece);
ZH_BS_HD uint32_t zlib_pieces(uint32_t neb) { return (neb + kZlibPiece - 1) / kZlibPiece; }
ZH_BS_HD uint32_t zlib_piece_size(uint32_t neb, uint32_t k) {
  const uint32_t rest = neb - k * kZlibPiece;
  return rest < kZlibPiece ? rest : kZlibPiece;
}
// Stored size of a stream of neb raw bytes whose segments have `segs` bytes together: neb says
// the stream is stored raw.
ZH_BS_HD uint32_t zlib_stream_size(uint32_t neb, uint64_t segs) {
  return kZlibOver + segs < neb ? kZlibOver + (uint32_t)segs : neb;
}
inline void put_zlib_head(uint8_t* d) { d[0] = 0x78, d[1] = 0x01; }
// 03 00 and the Adler-32, big-endian: zh_gz::kEnding + 4 bytes
inline void put_zlib_tail(uint8_t* d, uint32_t adler) {
  zh_gz::put_final(d);
  for (int i = 0; i < 4; i++) d[zh_gz::kEnding + i] = (uint8_t)(adler >> (8 * (3 - i)));
}

// ---- stream coders: (stream, neb, out, table) -> stored size, neb: store the stream raw -------
// kCode: the compressor code of the frame; kHead: room out needs beyond neb bytes.
struct Lz4Coder {
  static constexpr uint32_t kCode = 1, kHead = 0;
  HostLanes w;
  uint32_t operator()(const uint8_t* st, uint32_t neb, uint8_t* out, uint32_t* table) {
    return encode_stream(st, neb, out, table, w);
  }
};
struct ZstdCoder {
  static constexpr uint32_t kCode = 4, kHead = kZstdHead;
  const zh_ze::Tables& T;
  HostLanes w;
  uint16_t* seq;  // the records of one stream
  explicit ZstdCoder(const zh_ze::Tables& t) : T(t), seq(new uint16_t[3 * (kMaxBlock / 4) + 3]) {
    w.wide = true;
  }
  ZstdCoder(const ZstdCoder&) = delete;
  ~ZstdCoder() { delete[] seq; }
  uint32_t operator()(const uint8_t* st, uint32_t neb, uint8_t* out, uint32_t* table) {
    uint8_t* blk = out + kZstdHead;
    uint32_t nl = 0;
    const uint32_t ns = zh_ze::match_block(st, neb, blk + 3, seq, table, w, &nl);
    const uint32_t cs = zh_ze::fse_block(T, seq, ns, nl, blk, neb);
    if (zstd_stream_size(neb, cs) == neb) return neb;
    zh_ze::put_frame_header(out, neb, false);
    const uint32_t h = zh_ze::block_header(cs, 2, true);
    out[13] = (uint8_t)h, out[14] = (uint8_t)(h >> 8), out[15] = (uint8_t)(h >> 16);
    return kZstdHead + cs;
  }
};

struct ZlibCoder {
  static constexpr uint32_t kCode = 3, kHead = kZlibHead;
  HostLanes w;
  uint16_t* seq;        // the records of one piece
  zh_gz::DynWork* dyn;  // ZH_BLOSC_ENC_DYNAMIC, else null
  explicit ZlibCoder(bool dynamic)
      : seq(new uint16_t[3 * (kZlibPiece / 4) + 3]), dyn(dynamic ? new zh_gz::DynWork : nullptr) {
    w.wide = true;
  }
  ZlibCoder(const ZlibCoder&) = delete;
  ~ZlibCoder() {
    delete dyn;
    delete[] seq;
  }
  uint32_t operator()(const uint8_t* st, uint32_t neb, uint8_t* out, uint32_t* table) {
    if (neb > kMaxBlock) return neb;
    uint32_t o = 2;  // a segment is written at out + o only while o + kZlibOver - 2 < neb
    for (uint32_t k = 0, np = zlib_pieces(neb); k < np; k++) {
      const uint32_t psz = zlib_piece_size(neb, k);
      o += zh_gz::put_segment(st + (size_t)k * kZlibPiece, psz, out + o, seq, table, w, dyn);
      if (zlib_stream_size(neb, o - 2) == neb) return neb;
    }
    put_zlib_head(out);
    zh_gd::SerialLanes one;
    put_zlib_tail(out + o, zh_gd::adler32(st, neb, one));
    return o + (uint32_t)zh_gz::kEnding + 4;
  }
};

// One frame on the host.  dst == nullptr: *cbytes = the bound n + 16.  tmp, scratch: one block
// each (min(blocksize, n) bytes, scratch and the coder's kHead); table: kHashSize slots.
template <class Coder>
inline int compress_frame(const uint8_t* src, size_t n, const zh_blosc_enc_params* prm,
                          uint8_t* dst, size_t cap, size_t* cbytes, const char** msg,
                          Coder& coder) {
  Layout L;
  if (make_layout(n, prm, &L) != ZH_OK || (n > 0 && !src)) {
    *msg = "zh_blosc_compress: typesize 1..255, shuffle 0..2, blocksize >= 0, at most 2 GiB";
    return ZH_EINVAL;
  }
  with_compressor(&L, Coder::kCode);
  if (!dst) {
    *cbytes = n + 16;
    return ZH_OK;
  }
  if (cap < n + 16) {
    *msg = "zh_blosc_compress: destination smaller than nbytes + 16";
    return ZH_EINVAL;
  }
  size_t pos = 16 + 4 * (size_t)L.nblocks;
  bool fits = n > 0 && pos <= n + 16;  // tiny blocks: the block starts alone can pass the bound
  if (fits) {
    uint8_t* tmp = new uint8_t[L.blocksize];
    uint8_t* scratch = new uint8_t[L.blocksize + Coder::kHead];
    uint32_t* table = new uint32_t[kHashSize];
    for (uint32_t k = 0; k < L.nblocks && fits; k++) {
      const uint32_t bsz = block_size(L, n, k), ns = block_streams(L, bsz), neb = bsz / ns;
      const uint8_t* in = src + (size_t)k * L.blocksize;
      for (uint32_t o = 0; o < bsz; o++) tmp[o] = shuffled_byte_at(in, o, bsz, L.typesize, L.shuffle);
      wr32(dst + 16 + 4 * (size_t)k, (uint32_t)pos);
      for (uint32_t si = 0; si < ns && fits; si++) {
        const uint8_t* st = tmp + (size_t)si * neb;
        const uint32_t cs = coder(st, neb, scratch, table);
        if (pos + 4 + cs > n + 16) {
          fits = false;
          break;
        }
        wr32(dst + pos, cs);
        const uint8_t* from = cs == neb ? st : scratch;
        for (uint32_t q = 0; q < cs; q++) dst[pos + 4 + q] = from[q];
        pos += 4 + (size_t)cs;
      }
    }
    delete[] table;
    delete[] scratch;
    delete[] tmp;
  }
  if (!fits) {  // header alone (n == 0), or the raw bytes behind it
    put_header(dst, L, memcpyed_flags(L), n, n + 16);
    for (size_t q = 0; q < n; q++) dst[16 + q] = src[q];
    *cbytes = n + 16;
    return ZH_OK;
  }
  put_header(dst, L, L.flags, n, pos);
  *cbytes = pos;
  return ZH_OK;
}

}  // namespace zh_be
