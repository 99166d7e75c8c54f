// zh_blosc_streams.h — the blosc1 stream parser shared by the host and the device.
//
// A blosc1 frame (layout: zh_blosc.cpp) is independent blocks, and a split block is typesize
// independent streams.  This header holds what both sides of the batched device decode
// (zh_blosc_kernels.hip) need, and nothing that needs a device:
//   * lz4_stream / blosclz_stream: one stream (src, csize) -> (dst, rawsize), with the
//     acceptance rules of lz4_block / blosclz_block in zh_blosc.cpp.  They are parameterised on
//     a copy policy C:
//         void     begin(const uint8_t* s, uint32_t n)       a stream starts
//         uint32_t rd(const uint8_t* s, uint32_t i)          byte i of the stream (i < n)
//         void     lit(uint8_t* d, const uint8_t* s, uint32_t n)       d[k] = s[k]
//         void     match(uint8_t* d, uint32_t o, uint32_t off, uint32_t n)
//                                               d[o+k] = d[o-off + k % off]   (off <= o)
//     SerialCopy is the host's; the kernel's WaveCopy copies across the 64 lanes of a wave.
//     A match only reads bytes below o, so a policy needs one ordering point per copy.
//     Every loop consumes at least one input byte per turn and every read and write is
//     checked first: the frames are untrusted.
//   * parse_header / build_table: the walk over one frame (header, block starts, the int32
//     csize chain), every field checked against srclen, into one row per block and per stream.
//   * unshuffle_byte_at: where output byte q of a block comes from in the shuffled block.
//   * decode_frame_serial: the whole frame on the host with SerialCopy (the sanitizer checker
//     tools/blosc_stream_check.cpp; the table and parsers the kernel runs, without a device).
//   * zstd streams (compressor code 4) enter the table only when the caller passes
//     ZH_BLOSC_ZSTD_DEVICE: a stream is then stored raw or ONE plain zstd frame (zstd_stream_ok),
//     method kZstd, decoded by zh_zstd_dec.h's decode_frame and not by decode_stream.  Without
//     the flag, or with any other kind of stream, the frame is the host decoder's.
//   * zlib streams (compressor code 3) enter the table only when the caller passes
//     ZH_BLOSC_ZLIB_DEVICE: a stream is then stored raw or a zlib stream whose two header bytes
//     zlib_stream_head_ok accepts, method kZlib, decoded by zlib_stream (zh_gzip_dec.h's
//     decode_zlib_stream and adler32) with the acceptance of zlib's uncompress.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/zarrhip.h"
#include "zh_gzip_dec.h"
#include "zh_zstd_dec.h"

#if defined(__HIPCC__)
#define ZH_BS_HD __host__ __device__ inline
#else
#define ZH_BS_HD inline
#endif

namespace zh_bs {

enum Method : uint32_t { kRaw = 0, kLz4 = 1, kBloscLz = 2, kZstd = 3, kZlib = 4 };
// kShufBit2: c-blosc 1.x (frame version <= 2) bit-shuffles a block only when its element count
// is a multiple of 8; kShufBit3: later formats shuffle the multiple-of-8 prefix.
enum Shuffle : uint32_t { kShufNone = 0, kShufByte = 1, kShufBit2 = 2, kShufBit3 = 3 };

struct BlockRow {
  int64_t dst_off;  // offset of the block in the frame's decoded bytes
  uint32_t size, typesize, shuffle, first_stream, nstreams;
};
struct StreamRow {
  int64_t src_off;  // offset of the payload in the frame
  uint32_t csize, blk_off, rawsize, method;
  uint32_t max_regen;  // kZstd: the largest Huffman literals section (its literal scratch)
};

struct SerialCopy {
  ZH_BS_HD void begin(const uint8_t*, uint32_t) {}
  ZH_BS_HD uint32_t rd(const uint8_t* s, uint32_t i) { return s[i]; }
  ZH_BS_HD void lit(uint8_t* d, const uint8_t* s, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) d[k] = s[k];
  }
  ZH_BS_HD void match(uint8_t* d, uint32_t o, uint32_t off, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) d[o + k] = d[o + k - off];
  }
};

// LZ4 block format: token (literal length << 4 | match length - 4), 255-continued lengths,
// literals, 16-bit LE offset, overlapping match copy.  True when exactly cap bytes came out.
template <class C>
ZH_BS_HD bool lz4_stream(const uint8_t* s, uint32_t n, uint8_t* d, uint32_t cap, C& c) {
  uint32_t i = 0, o = 0;
  c.begin(s, n);
  while (i < n) {
    const uint32_t tok = c.rd(s, i++);
    uint64_t lit = tok >> 4;
    if (lit == 15) {
      uint32_t b;
      do {
        if (i >= n) return false;
        b = c.rd(s, i++);
        lit += b;
      } while (b == 255);
    }
    if (lit > n - i || lit > cap - o) return false;
    c.lit(d + o, s + i, (uint32_t)lit);
    i += (uint32_t)lit;
    o += (uint32_t)lit;
    if (i >= n) break;  // the last sequence has literals only
    if (n - i < 2) return false;
    const uint32_t off = c.rd(s, i) | (c.rd(s, i + 1) << 8);
    i += 2;
    uint64_t ml = tok & 15;
    if (ml == 15) {
      uint32_t b;
      do {
        if (i >= n) return false;
        b = c.rd(s, i++);
        ml += b;
      } while (b == 255);
    }
    ml += 4;
    if (off == 0 || off > o || ml > cap - o) return false;
    c.match(d, o, off, (uint32_t)ml);
    o += (uint32_t)ml;
  }
  return o == cap;
}

// BloscLZ (FastLZ-derived): ctrl < 32 -> ctrl+1 literals; else a match of (ctrl >> 5) + 2
// bytes (7 -> 255-continued), distance ((ctrl & 31) << 8) + next byte + 1, with the 16-bit
// far form (+8191) when that byte is 255 and the high part is 31.
template <class C>
ZH_BS_HD bool blosclz_stream(const uint8_t* s, uint32_t n, uint8_t* d, uint32_t cap, C& c) {
  if (n == 0) return cap == 0;
  uint32_t ip = 0, o = 0;
  c.begin(s, n);
  uint32_t ctrl = c.rd(s, ip++) & 31u;
  for (;;) {
    if (ctrl >= 32) {
      uint64_t len = (ctrl >> 5) - 1;
      uint32_t dist = (ctrl & 31) << 8;
      if (len == 6) {
        uint32_t b;
        do {
          if (ip >= n) return false;
          b = c.rd(s, ip++);
          len += b;
        } while (b == 255);
      }
      if (ip >= n) return false;
      const uint32_t code = c.rd(s, ip++);
      if (code == 255 && dist == (31u << 8)) {
        if (n - ip < 2) return false;
        dist = ((c.rd(s, ip) << 8) | c.rd(s, ip + 1)) + 8191u;
        ip += 2;
      } else {
        dist += code;
      }
      len += 3;
      if (dist + 1 > o || len > cap - o) return false;
      c.match(d, o, dist + 1, (uint32_t)len);
      o += (uint32_t)len;
    } else {
      const uint32_t lit = ctrl + 1;
      if (lit > n - ip || lit > cap - o) return false;
      c.lit(d + o, s + ip, lit);
      ip += lit;
      o += lit;
    }
    if (ip >= n) break;
    ctrl = c.rd(s, ip++);
  }
  return o == cap;
}

template <class C>
ZH_BS_HD bool decode_stream(const uint8_t* s, uint32_t n, uint8_t* d, uint32_t cap,
                            uint32_t method, C& c) {
  if (method == kLz4) return lz4_stream(s, n, d, cap, c);
  if (method == kBloscLz) return blosclz_stream(s, n, d, cap, c);
  if (n != cap) return false;
  c.lit(d, s, n);
  return true;
}

// Elements of a block that the bit shuffle covers (the rest of the block is stored as is).
ZH_BS_HD uint32_t bitshuffle_elems(uint32_t size, uint32_t ts, uint32_t shuffle) {
  uint32_t ne = ts ? size / ts : 0;
  if (shuffle == kShufBit2 && ne % 8 != 0) ne = 0;
  return ne - ne % 8;
}

// Output byte q of a block of `size` bytes, read from the shuffled block `in`.
//   byte shuffle: stream j holds byte j of every element;
//   bit shuffle (bshuf_trans_bit_elem): for byte position j and bit k, a row of ne/8 bytes
//   whose bit m of byte p is bit k of byte j of element 8p+m.
ZH_BS_HD uint8_t unshuffle_byte_at(const uint8_t* in, uint32_t q, uint32_t size, uint32_t ts,
                                   uint32_t shuffle) {
  if (shuffle == kShufByte) {
    const uint32_t ne = size / ts;
    if (q >= ne * ts) return in[q];
    return in[(q % ts) * ne + q / ts];
  }
  if (shuffle == kShufBit2 || shuffle == kShufBit3) {
    const uint32_t ne = bitshuffle_elems(size, ts, shuffle);
    if (q >= ne * ts) return in[q];
    const uint32_t e = q / ts, j = q % ts, rowb = ne / 8;
    const uint8_t* col = in + (size_t)j * 8 * rowb + e / 8;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 8; k++) v |= ((col[(size_t)k * rowb] >> (e % 8)) & 1u) << k;
    return (uint8_t)v;
  }
  return in[q];
}

// ---------------------------------------------------------------------------------------
// host: header and tables
// ---------------------------------------------------------------------------------------
struct Header {
  uint32_t version = 0, flags = 0, typesize = 0;
  size_t nbytes = 0, blocksize = 0, cbytes = 0, nblocks = 0;
  bool memcpyed = false;
  int comp = 0;
};

inline uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The checks of zh_blosc_decompress's size query, in its order and with its texts.
inline int parse_header(const uint8_t* src, size_t srclen, Header* h, const char** msg) {
  if (!src || srclen < 16) {
    *msg = "blosc frame shorter than its 16-byte header";
    return ZH_EDATA;
  }
  h->version = src[0];
  h->flags = src[2];
  h->typesize = src[3];
  h->nbytes = rd32(src + 4);
  h->blocksize = rd32(src + 8);
  h->cbytes = rd32(src + 12);
  h->memcpyed = (h->flags & 0x02) != 0;
  h->comp = (int)(h->flags >> 5);
  h->nblocks = 0;
  if (h->cbytes > srclen || (h->memcpyed && 16 + h->nbytes > srclen)) {
    *msg = "blosc frame truncated";
    return ZH_EDATA;
  }
  if (!h->memcpyed && h->nbytes > 0) {
    const size_t expand = h->comp == 4 ? 32768 : 2048;  // zstd: an RLE block (zh_blosc.cpp)
    if (h->blocksize == 0 || h->typesize == 0 ||
        h->nbytes > expand * (size_t)h->cbytes + 65536) {
      *msg = "corrupt blosc header";
      return ZH_EDATA;
    }
    h->nblocks = (h->nbytes + h->blocksize - 1) / h->blocksize;
    if (16 + 4 * h->nblocks > srclen) {
      *msg = "blosc frame truncated";
      return ZH_EDATA;
    }
  }
  return ZH_OK;
}

// Where a frame is decoded: 0 device streams, 1 host (zlib / zstd payloads), 2 memcpyed.
// (With ZH_BLOSC_ZSTD_DEVICE a zstd frame whose table build_table accepts is 0, and with
// ZH_BLOSC_ZLIB_DEVICE a zlib frame: the plan's.)
inline int frame_where(const Header& h) {
  if (h.memcpyed) return 2;
  return (h.comp == 3 || h.comp == 4) ? 1 : 0;
}

// What the device route takes of a zstd stream of `neb` raw bytes: one frame that ends exactly
// at the stream's last byte, no dictionary, no checksum, and a content size that is the stream's
// raw size (what ZSTD_compress, which c-blosc calls, writes).  Concatenated and skippable
// frames, a checksum, a missing or different content size: the host decoder's.
inline bool zstd_stream_ok(const uint8_t* s, size_t n, size_t neb, uint32_t* max_regen) {
  const zh_zd::Walk w = zh_zd::walk_frame<zh_zd::NoRows>(s, n, nullptr);
  if (!w.device || w.csum || w.fcs != (int64_t)neb) return false;
  *max_regen = (uint32_t)w.max_regen;  // <= fcs == neb < 2^32
  return true;
}

// What the device route takes of a zlib stream: a header zlib's inflate accepts (CM 8, the check
// bits, no preset dictionary) that declares the 32 KiB window (CINFO 7: what compress2, which
// c-blosc calls, writes), so that no zlib, however strictly it checks a distance against the
// declared window, can disagree with the device about one.  Any other header is the host
// decoder's to judge.
inline bool zlib_stream_head_ok(const uint8_t* s, size_t n) {
  uint32_t cinfo = 0;
  return zh_gd::zlib_header(s, n, &cinfo) == zh_gd::kOk && cinfo == 7;
}

// One zlib stream (src, csize) -> (dst, rawsize) with the acceptance of zlib_block in
// zh_blosc.cpp, which is uncompress's: exactly rawsize bytes come out and their Adler-32 is the
// stored one; bytes behind the trailer are ignored.  All lanes of P return the same verdict.
template <class P>
ZH_BS_HD zh_gd::Verdict zlib_stream(const uint8_t* s, uint32_t n, uint8_t* d, uint32_t rawsize,
                                    zh_gd::Work& w, P& p) {
  uint64_t made = 0;
  size_t used = 0;
  uint32_t adler = 0;
  zh_gd::Verdict v =
      zh_gd::decode_zlib_stream(s, (size_t)n, d, (uint64_t)rawsize, w, p, &made, &used, &adler);
  if (!v && made != (uint64_t)rawsize) v = zh_gd::kSizeMismatch;
  if (v) return v;
  p.order();  // the sums read what other lanes stored
  return zh_gd::adler32(d, made, p) == adler ? zh_gd::kOk : zh_gd::kAdlerMismatch;
}

// Block and stream rows of a frame whose header parse_header accepted and that is neither
// memcpyed nor host-decoded.  `flags`: ZH_BLOSC_ZSTD_DEVICE admits compressor code 4; a stream
// zstd_stream_ok refuses makes the frame host-decoded (ZH_EUNSUPPORTED, as without the flag).
// ZH_BLOSC_ZLIB_DEVICE admits compressor code 3 in the same way, with zlib_stream_head_ok.
// V: a vector-like with push_back / size.  Walks the frame as zh_blosc_decompress does; at the first field that fails returns that decoder's status and
// text with the rows of the blocks before it in place (the failing block's rows are dropped).
template <class VB, class VS>
inline int build_table(const uint8_t* src, size_t srclen, const Header& h, VB& blocks,
                       VS& streams, const char** msg, unsigned flags = 0) {
  const bool zstd = h.comp == 4 && (flags & ZH_BLOSC_ZSTD_DEVICE);
  const bool zlib = h.comp == 3 && (flags & ZH_BLOSC_ZLIB_DEVICE);
  if (h.comp != 0 && h.comp != 1 && !zstd && !zlib) {
    *msg = h.comp == 2 ? "blosc compressor (snappy) not available on this host"
                       : "blosc payload is decoded on the host";
    return ZH_EUNSUPPORTED;
  }
  const bool bitshuf = (h.flags & 0x04) && !(h.flags & 0x01);
  const size_t ts = h.typesize;
  for (size_t k = 0; k < h.nblocks; k++) {
    const size_t bs = k + 1 < h.nblocks ? h.blocksize : h.nbytes - k * h.blocksize;
    const bool leftover = bs < h.blocksize;
    const size_t nsplit = ((h.flags & 0x10) || leftover) ? 1 : ts;
    const size_t neb = bs / nsplit;
    if (nsplit > 1 && bs % nsplit != 0) {
      *msg = "blosc frame header corrupt (block not a multiple of the typesize)";
      return ZH_EDATA;
    }
    BlockRow b;
    b.dst_off = (int64_t)(k * h.blocksize);
    b.size = (uint32_t)bs;
    b.typesize = (uint32_t)ts;
    b.shuffle = bitshuf ? (h.version <= 2 ? kShufBit2 : kShufBit3)
                        : ((h.flags & 0x01) && ts > 1 ? kShufByte : kShufNone);
    b.first_stream = (uint32_t)streams.size();
    b.nstreams = (uint32_t)nsplit;
    size_t p = rd32(src + 16 + 4 * k);
    StreamRow rows[256];
    for (size_t sidx = 0; sidx < nsplit; sidx++) {
      if (p > srclen || srclen - p < 4) {
        *msg = "blosc frame truncated";
        return ZH_EDATA;
      }
      const size_t cs = rd32(src + p);
      p += 4;
      if (cs > srclen - p) {
        *msg = "blosc frame truncated";
        return ZH_EDATA;
      }
      StreamRow& r = rows[sidx];
      r.src_off = (int64_t)p;
      r.csize = (uint32_t)cs;
      r.blk_off = (uint32_t)(sidx * neb);
      r.rawsize = (uint32_t)neb;
      r.method = cs == neb ? kRaw : zstd ? kZstd : zlib ? kZlib : (h.comp == 0 ? kBloscLz : kLz4);
      r.max_regen = 0;
      if ((r.method == kZstd && !zstd_stream_ok(src + p, cs, neb, &r.max_regen)) ||
          (r.method == kZlib && !zlib_stream_head_ok(src + p, cs))) {
        *msg = "blosc payload is decoded on the host";
        return ZH_EUNSUPPORTED;
      }
      p += cs;
    }
    for (size_t sidx = 0; sidx < nsplit; sidx++) streams.push_back(rows[sidx]);
    blocks.push_back(b);
  }
  return ZH_OK;
}

// zh_blosc_decompress for frames with raw / LZ4 / BloscLZ streams, through the tables and the
// serial form of the shared parser.  `tmp`: scratch of at least min(blocksize, nbytes) bytes.
// `flags`: with ZH_BLOSC_ZLIB_DEVICE also the frames with zlib streams that build_table admits
// (zlib_stream on one lane); the other flags mean nothing here.
template <class VB, class VS>
inline int decode_frame_serial(const uint8_t* src, size_t srclen, uint8_t* dst, size_t dstcap,
                               uint8_t* tmp, VB& blocks, VS& streams, const char** msg,
                               unsigned flags = 0) {
  Header h;
  int st = parse_header(src, srclen, &h, msg);
  if (st != ZH_OK) return st;
  if (h.nbytes > dstcap) {
    *msg = "blosc destination too small";
    return ZH_EINVAL;
  }
  if (h.memcpyed) {
    for (size_t k = 0; k < h.nbytes; k++) dst[k] = src[16 + k];
    return ZH_OK;
  }
  const size_t b0 = blocks.size();
  const char* tmsg = nullptr;
  const int tst =
      build_table(src, srclen, h, blocks, streams, &tmsg, flags & ZH_BLOSC_ZLIB_DEVICE);
  if (tst == ZH_EUNSUPPORTED) {
    *msg = tmsg;
    return tst;
  }
  SerialCopy c;
  zh_gd::SerialLanes lanes;
  zh_gd::Work work;  // kZlib streams only
  for (size_t k = b0; k < blocks.size(); k++) {
    const BlockRow& b = blocks[k];
    uint8_t* out = b.shuffle == kShufNone ? dst + b.dst_off : tmp;
    for (uint32_t s = 0; s < b.nstreams; s++) {
      const StreamRow& r = streams[b.first_stream + s];
      const bool ok =
          r.method == kZlib
              ? zlib_stream(src + r.src_off, r.csize, out + r.blk_off, r.rawsize, work, lanes) ==
                    zh_gd::kOk
              : decode_stream(src + r.src_off, r.csize, out + r.blk_off, r.rawsize, r.method, c);
      if (!ok) {
        *msg = "corrupt blosc block";
        return ZH_EDATA;
      }
    }
    if (b.shuffle != kShufNone)
      for (uint32_t q = 0; q < b.size; q++)
        dst[b.dst_off + q] = unshuffle_byte_at(tmp, q, b.size, b.typesize, b.shuffle);
  }
  if (tst != ZH_OK) *msg = tmsg;
  return tst;
}

}  // namespace zh_bs
