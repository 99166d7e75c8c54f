// blosc_zlib_enc_check — host-only checker of the blosc frame writer with zlib streams
// (csrc/zh_blosc_enc.h over ZlibCoder), built with -fsanitize=address,undefined by
// tests/test_blosc_zlib_encode_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o blosc_zlib_enc_check tools/blosc_zlib_enc_check.cpp -lz
//   blosc_zlib_enc_check buffers.bin frames.bin <flags: 4 | 12>
//
// buffers.bin: per buffer four little-endian uint32 (length, typesize, shuffle, blocksize) and
// the bytes.  Every buffer is compressed with the host form of the writer (the lane loop the
// match kernel runs as one wave, the serial coders the coding kernels run a wave per piece),
// decoded again by its header and stream table alone (build_table as the batch decoder plans it,
// libz's uncompress per zlib stream, unshuffle_byte_at) and compared; frames.bin receives, per
// buffer, a uint32 length and the frame, for the caller to compare with zh_blosc_compress_ex.
// One line per buffer:
//   <zh_status> <cbytes> <ok | MISMATCH | message>
// Exit status 1 when a frame did not decode to its buffer.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/zh_blosc_enc.h"

// The frame by its header and stream table alone: raw streams copied, zlib streams through
// uncompress from and into heap blocks of exactly the streams' sizes, then the unshuffle.
static int decode(const uint8_t* src, size_t srclen, uint8_t* dst, size_t dstcap,
                  const char** msg) {
  zh_bs::Header h;
  int st = zh_bs::parse_header(src, srclen, &h, msg);
  if (st != ZH_OK) return st;
  if (h.nbytes > dstcap) {
    *msg = "destination too small";
    return ZH_EINVAL;
  }
  if (h.memcpyed) {
    for (size_t k = 0; k < h.nbytes; k++) dst[k] = src[16 + k];
    return ZH_OK;
  }
  if (h.comp != 3) {
    *msg = "not a zlib frame";
    return ZH_EDATA;
  }
  std::vector<zh_bs::BlockRow> blocks;
  std::vector<zh_bs::StreamRow> streams;
  st = zh_bs::build_table(src, srclen, h, blocks, streams, msg, ZH_BLOSC_ZLIB_DEVICE);
  if (st != ZH_OK) return st;
  for (const zh_bs::BlockRow& b : blocks) {
    uint8_t* win = (uint8_t*)malloc(b.size ? b.size : 1);
    for (uint32_t s = 0; s < b.nstreams && st == ZH_OK; s++) {
      const zh_bs::StreamRow& r = streams[b.first_stream + s];
      if (r.method == zh_bs::kRaw) {
        memcpy(win + r.blk_off, src + r.src_off, r.rawsize);
        continue;
      }
      uint8_t* in = (uint8_t*)malloc(r.csize);  // the decoder sees exactly the stream
      uint8_t* out = (uint8_t*)malloc(r.rawsize);
      memcpy(in, src + r.src_off, r.csize);
      uLongf got = r.rawsize;
      if (r.method != zh_bs::kZlib || r.csize >= r.rawsize || in[0] != 0x78 || in[1] != 0x01 ||
          uncompress(out, &got, in, r.csize) != Z_OK || got != r.rawsize) {
        *msg = "a stream did not inflate";
        st = ZH_EDATA;
      } else {
        memcpy(win + r.blk_off, out, r.rawsize);
      }
      free(out);
      free(in);
    }
    for (uint32_t q = 0; q < b.size && st == ZH_OK; q++)
      dst[b.dst_off + q] = zh_bs::unshuffle_byte_at(win, q, b.size, b.typesize, b.shuffle);
    free(win);
    if (st != ZH_OK) return st;
  }
  return ZH_OK;
}

int main(int argc, char** argv) {
  const unsigned flags = argc == 4 ? (unsigned)atoi(argv[3]) : 0;
  if (argc != 4 || (flags != ZH_BLOSC_ENC_ZLIB &&
                    flags != (ZH_BLOSC_ENC_ZLIB | ZH_BLOSC_ENC_DYNAMIC))) {
    fprintf(stderr, "usage: %s buffers.bin frames.bin <4 | 12>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) {
    perror(!f ? argv[1] : argv[2]);
    return 2;
  }
  int bad = 0;
  for (;;) {
    uint8_t hb[16];
    if (fread(hb, 1, 16, f) != 16) break;
    const size_t len = zh_bs::rd32(hb);
    zh_blosc_enc_params prm;
    prm.typesize = (int32_t)zh_bs::rd32(hb + 4);
    prm.shuffle = (int32_t)zh_bs::rd32(hb + 8);
    prm.blocksize = (int32_t)zh_bs::rd32(hb + 12);
    // exact-size heap copies: the sanitizer sees any access past either end
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    uint8_t* frame = (uint8_t*)malloc(len + 16);
    size_t cbytes = 0;
    const char* msg = "";
    zh_be::ZlibCoder coder((flags & ZH_BLOSC_ENC_DYNAMIC) != 0);
    int st = zh_be::compress_frame(buf, len, &prm, frame, len + 16, &cbytes, &msg, coder);
    const char* verdict = msg;
    if (st == ZH_OK) {
      // the decoder sees exactly cbytes
      uint8_t* exact = (uint8_t*)malloc(cbytes);
      memcpy(exact, frame, cbytes);
      uint8_t* dst = (uint8_t*)malloc(len ? len : 1);
      const char* dmsg = "";
      const int ds = decode(exact, cbytes, dst, len, &dmsg);
      const bool same = ds == ZH_OK && cbytes <= len + 16 && zh_bs::rd32(exact + 4) == len &&
                        (len == 0 || memcmp(dst, buf, len) == 0);
      verdict = same ? "ok" : (ds == ZH_OK ? "MISMATCH" : dmsg);
      bad += !same;
      uint8_t lb[4];
      zh_be::wr32(lb, (uint32_t)cbytes);
      fwrite(lb, 1, 4, g);
      fwrite(exact, 1, cbytes, g);
      free(dst);
      free(exact);
    }
    printf("%d %zu %s\n", st, cbytes, verdict);
    free(frame);
    free(buf);
  }
  fclose(f);
  fclose(g);
  return bad ? 1 : 0;
}
