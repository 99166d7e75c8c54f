// zstd_enc_check — host-only checker of the zstd frame writer (csrc/zh_zstd_enc.h), built with
// -fsanitize=address,undefined by tests/test_zstd_encode_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o zstd_enc_check tools/zstd_enc_check.cpp
//   zstd_enc_check buffers.bin frames.bin
//
// buffers.bin: per buffer three little-endian uint32 (length, checksum, blocksize) and the
// bytes.  Every buffer is compressed with the host form of the writer (the lane loop the kernel
// runs as one wave, the serial FSE pass the second kernel runs per thread), decoded again with
// the frame decoder of csrc/zh_zstd.cpp (compiled into this program, with the tables the
// encoder derives from it) and compared; frames.bin receives, per buffer, a uint32 length and
// the frame, for the caller to compare with zh_zstd_compress.  One line per buffer:
//   <zh_status> <frame bytes> <ok | MISMATCH | message>
// Exit status 1 when a frame did not decode to its buffer.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/zh_zstd.cpp"

static uint32_t rd32le(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

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
    uint8_t hb[12];
    if (fread(hb, 1, 12, f) != 12) break;
    const size_t len = rd32le(hb);
    zh_zstd_enc_params prm;
    prm.checksum = (int32_t)rd32le(hb + 4);
    prm.blocksize = (int32_t)rd32le(hb + 8);
    // exact-size heap copies: the sanitizer sees any access past either end
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    const char* msg = "";
    size_t bound = 0, flen = 0;
    int st = zh_ze::compress_frame(zh_ze::tables(), buf, len, &prm, nullptr, 0, &bound, &msg);
    uint8_t* frame = (uint8_t*)malloc(bound ? bound : 1);
    if (st == ZH_OK)
      st = zh_ze::compress_frame(zh_ze::tables(), buf, len, &prm, frame, bound, &flen, &msg);
    const char* verdict = msg;
    if (st == ZH_OK) {
      uint8_t* exact = (uint8_t*)malloc(flen);  // the decoder sees exactly the frame
      memcpy(exact, frame, flen);
      uint8_t* dst = (uint8_t*)malloc(len ? len : 1);
      size_t got = 0;
      char err[128] = "";
      const int ds = zh_zstd_decompress(exact, flen, dst, len, &got, err, sizeof err);
      const bool same = ds == ZH_OK && got == len && flen <= bound &&
                        (len == 0 || memcmp(dst, buf, len) == 0);
      verdict = same ? "ok" : "MISMATCH";
      bad += !same;
      uint8_t lb[4] = {(uint8_t)flen, (uint8_t)(flen >> 8), (uint8_t)(flen >> 16),
                       (uint8_t)(flen >> 24)};
      fwrite(lb, 1, 4, g);
      fwrite(exact, 1, flen, g);
      free(dst);
      free(exact);
    }
    printf("%d %zu %s\n", st, flen, verdict);
    free(frame);
    free(buf);
  }
  fclose(f);
  fclose(g);
  return bad ? 1 : 0;
}
