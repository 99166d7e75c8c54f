// blosc_enc_check — host-only checker of the blosc LZ4 frame writer (csrc/zh_blosc_enc.h), built
// with -fsanitize=address,undefined by tests/test_blosc_encode_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o blosc_enc_check tools/blosc_enc_check.cpp
//   blosc_enc_check buffers.bin frames.bin
//
// buffers.bin: per buffer four little-endian uint32 (length, typesize, shuffle, blocksize) and
// the bytes.  Every buffer is compressed with the host form of the writer (the lane loop the
// kernel runs as one wave), decoded again with the serial form of the shared parser
// (decode_frame_serial) and compared; frames.bin receives, per buffer, a uint32 length and the
// frame, for the caller to compare with zh_blosc_compress.  One line per buffer:
//   <zh_status> <cbytes> <ok | MISMATCH | message>
// Exit status 1 when a frame did not decode to its buffer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/zh_blosc_enc.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s buffers.bin frames.bin\n", argv[0]);
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
    zh_be::Lz4Coder lz4;
    int st = zh_be::compress_frame(buf, len, &prm, frame, len + 16, &cbytes, &msg, lz4);
    const char* verdict = msg;
    if (st == ZH_OK) {
      // the decoder sees exactly cbytes
      uint8_t* exact = (uint8_t*)malloc(cbytes);
      memcpy(exact, frame, cbytes);
      uint8_t* dst = (uint8_t*)malloc(len ? len : 1);
      const size_t tb = len < zh_be::kMaxBlock ? len : zh_be::kMaxBlock;
      uint8_t* tmp = (uint8_t*)malloc(tb ? tb : 1);
      std::vector<zh_bs::BlockRow> blocks;
      std::vector<zh_bs::StreamRow> streams;
      const char* dmsg = "";
      const int ds = zh_bs::decode_frame_serial(exact, cbytes, dst, len, tmp, blocks, streams,
                                                &dmsg);
      const bool same = ds == ZH_OK && cbytes <= len + 16 && zh_bs::rd32(exact + 4) == len &&
                        (len == 0 || memcmp(dst, buf, len) == 0);
      verdict = same ? "ok" : "MISMATCH";
      bad += !same;
      uint8_t lb[4];
      zh_be::wr32(lb, (uint32_t)cbytes);
      fwrite(lb, 1, 4, g);
      fwrite(exact, 1, cbytes, g);
      free(tmp);
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
