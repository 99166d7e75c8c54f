// blosc_zstd_check — host-only checker of the device route for blosc frames with zstd streams
// (ZH_BLOSC_ZSTD_DEVICE: csrc/zh_blosc_streams.h, csrc/zh_zstd_dec.h), built with
// -fsanitize=address,undefined by tests/test_blosc_zstd_host.py and by `make blosc_zstd_check`:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o blosc_zstd_check tools/blosc_zstd_check.cpp
//   blosc_zstd_check frames.bin [more.bin ...]
//
// frames.bin: per frame a little-endian uint32 length and the frame's bytes.  Every frame goes
// through what the batch does before and inside its kernels, on one lane: the header walk, the
// plan's verdict (build_table with the flag), then per block the window the rows describe (the
// block's place in the decoded frame when it is not shuffled, a temporary of the block's size
// otherwise), raw streams copied, every kZstd stream decoded by zh_zd::decode_frame with
// SerialLanes into its place in the window with a literal scratch of exactly its max_regen
// bytes, and the byte / bit unshuffle by unshuffle_byte_at.  Every buffer is a heap block of its
// exact size, so the sanitizer sees any access past either end.  One line per frame:
//   <where: 0 device, 1 host, 2 memcpyed, -1 header refused> <zh_status of the device decode>
//   <XXH64 of the decoded bytes, 16 hex digits; 0 unless where 0 and status 0> <kZstd streams>
// The test compares the lines with zh_blosc_batch_plan_ex and zh_blosc_decompress.
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

uint8_t* exact(size_t n) { return (uint8_t*)malloc(n ? n : 1); }

// One kZstd stream as pass 1 decodes it: true when exactly rawsize bytes came out of exactly
// csize bytes.
bool zstd_stream(const uint8_t* frame, const zh_bs::StreamRow& r, uint8_t* out) {
  uint8_t* src = exact(r.csize);
  memcpy(src, frame + r.src_off, r.csize);
  uint8_t* lit = exact(r.max_regen);
  zh_zd::Work* W = (zh_zd::Work*)malloc(sizeof(zh_zd::Work));
  zh_zd::SerialLanes p;
  zh_zd::Header h;
  uint64_t made = 0;
  size_t used = 0;
  const zh_zd::Verdict v = zh_zd::decode_frame(src, (size_t)r.csize, out, (uint64_t)r.rawsize, lit,
                                               (uint64_t)r.max_regen, *W, p, &made, &used, &h);
  free(W);
  free(lit);
  free(src);
  return v == zh_zd::kOk && made == r.rawsize && used == r.csize;
}

void check_frame(const uint8_t* frame, size_t len) {
  zh_bs::Header h;
  const char* msg = "";
  if (zh_bs::parse_header(frame, len, &h, &msg) != ZH_OK) {
    printf("-1 0 %016llx 0\n", 0ull);
    return;
  }
  std::vector<zh_bs::BlockRow> blocks;
  std::vector<zh_bs::StreamRow> streams;
  int where = zh_bs::frame_where(h);
  if (where == 1 && h.comp == 4 &&
      zh_bs::build_table(frame, len, h, blocks, streams, &msg, ZH_BLOSC_ZSTD_DEVICE) == ZH_OK)
    where = 0;
  if (where != 0 || h.comp != 4) {  // not this route's
    printf("%d 0 %016llx 0\n", where, 0ull);
    return;
  }
  uint8_t* dst = exact(h.nbytes);
  int st = ZH_OK;
  long nz = 0;
  for (const zh_bs::BlockRow& b : blocks) {
    // the window: the block's place in the decoded frame, or a temporary when it is shuffled
    const bool tmp = b.shuffle != zh_bs::kShufNone;
    uint8_t* win = tmp ? exact(b.size) : nullptr;
    for (uint32_t s = 0; s < b.nstreams && st == ZH_OK; s++) {
      const zh_bs::StreamRow& r = streams[b.first_stream + s];
      // a stream's place: its own exact block, so that a write past rawsize is seen
      uint8_t* out = exact(r.rawsize);
      if (r.method == zh_bs::kZstd) {
        nz++;
        if (!zstd_stream(frame, r, out)) st = ZH_EDATA;
      } else if (r.method == zh_bs::kRaw && r.csize == r.rawsize) {
        memcpy(out, frame + r.src_off, r.rawsize);
      } else {
        st = ZH_EDATA;
      }
      if ((size_t)r.blk_off + r.rawsize > b.size) st = ZH_EDATA;  // the table's promise
      if (st == ZH_OK) memcpy((tmp ? win : dst + b.dst_off) + r.blk_off, out, r.rawsize);
      free(out);
    }
    if (tmp && st == ZH_OK)
      for (uint32_t q = 0; q < b.size; q++)
        dst[b.dst_off + q] = zh_bs::unshuffle_byte_at(win, q, b.size, b.typesize, b.shuffle);
    free(win);
    if (st != ZH_OK) break;
  }
  printf("0 %d %016llx %ld\n", st, (unsigned long long)(st == ZH_OK ? xxh64(dst, h.nbytes) : 0),
         nz);
  free(dst);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s frames.bin [more.bin ...]\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      perror(argv[a]);
      return 2;
    }
    for (;;) {
      uint8_t lb[4];
      if (fread(lb, 1, 4, f) != 4) break;
      const size_t len = zh_bs::rd32(lb);
      uint8_t* frame = exact(len);
      if (len && fread(frame, 1, len, f) != len) {
        fprintf(stderr, "short input file\n");
        return 2;
      }
      check_frame(frame, len);
      free(frame);
    }
    fclose(f);
  }
  return 0;
}
