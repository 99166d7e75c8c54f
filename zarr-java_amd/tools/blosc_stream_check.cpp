// blosc_stream_check — host-only checker of the shared blosc stream parser
// (csrc/zh_blosc_streams.h), built with -fsanitize=address,undefined by
// tests/test_blosc_batch_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o blosc_stream_check tools/blosc_stream_check.cpp
//   blosc_stream_check frames.bin
//
// frames.bin: per frame a little-endian uint32 length and the frame's bytes.  Every frame is
// decoded through the tables and the serial form of the parser the kernel runs (header walk,
// LZ4 / BloscLZ / raw streams, byte and bit unshuffle); one line per frame:
//   <zh_status> <XXH64 of the decoded bytes, 16 hex digits; 0 when rejected> <message>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/zh_blosc_streams.h"

namespace {

constexpr uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL,
                   P3 = 1609587929392839161ULL, P4 = 9650029242287828579ULL,
                   P5 = 2870177450012600261ULL;
uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
uint64_t rd64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;  // little-endian hosts only
}
uint64_t rnd(uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; }
uint64_t merge(uint64_t h, uint64_t v) { return (h ^ rnd(0, v)) * P1 + P4; }

uint64_t xxh64(const uint8_t* p, size_t len) {
  const uint8_t* end = p + len;
  uint64_t h;
  if (len >= 32) {
    uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
    do {
      v1 = rnd(v1, rd64(p));
      v2 = rnd(v2, rd64(p + 8));
      v3 = rnd(v3, rd64(p + 16));
      v4 = rnd(v4, rd64(p + 24));
      p += 32;
    } while (p + 32 <= end);
    h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    h = merge(h, v1), h = merge(h, v2), h = merge(h, v3), h = merge(h, v4);
  } else {
    h = P5;
  }
  h += (uint64_t)len;
  for (; p + 8 <= end; p += 8) h = rotl(h ^ rnd(0, rd64(p)), 27) * P1 + P4;
  if (p + 4 <= end) {
    uint32_t v;
    memcpy(&v, p, 4);
    h = rotl(h ^ (v * P1), 23) * P2 + P3;
    p += 4;
  }
  for (; p < end; p++) h = rotl(h ^ (*p * P5), 11) * P1;
  h ^= h >> 33, h *= P2, h ^= h >> 29, h *= P3, h ^= h >> 32;
  return h;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s frames.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  for (;;) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const size_t len = zh_bs::rd32(lb);
    // exact-size heap copies: the sanitizer sees any access past either end
    uint8_t* frame = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(frame, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    zh_bs::Header h;
    const char* msg = "";
    int st = zh_bs::parse_header(frame, len, &h, &msg);
    uint64_t hash = 0;
    if (st == ZH_OK) {
      const size_t tb = h.blocksize < h.nbytes ? h.blocksize : h.nbytes;
      uint8_t* dst = (uint8_t*)malloc(h.nbytes ? h.nbytes : 1);
      uint8_t* tmp = (uint8_t*)malloc(tb ? tb : 1);
      std::vector<zh_bs::BlockRow> blocks;
      std::vector<zh_bs::StreamRow> streams;
      st = zh_bs::decode_frame_serial(frame, len, dst, h.nbytes, tmp, blocks, streams, &msg);
      if (st == ZH_OK) hash = xxh64(dst, h.nbytes);
      free(tmp);
      free(dst);
    }
    printf("%d %016llx %s\n", st, (unsigned long long)hash, st == ZH_OK ? "" : msg);
    free(frame);
  }
  fclose(f);
  return 0;
}
