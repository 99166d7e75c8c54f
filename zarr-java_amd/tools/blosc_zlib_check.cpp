// blosc_zlib_check — host-only checker of the device route for blosc frames with zlib streams
// (ZH_BLOSC_ZLIB_DEVICE: csrc/zh_blosc_streams.h, csrc/zh_gzip_dec.h) against zlib's uncompress,
// built with -fsanitize=address,undefined by tests/test_blosc_zlib_host.py and by
// `make blosc_zlib_check`:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o blosc_zlib_check tools/blosc_zlib_check.cpp -lz
//   blosc_zlib_check frames.bin [mutations-per-stream seed]
//
// frames.bin: per frame a little-endian uint32 length and the frame's bytes.  Per frame:
//   streams   every stream of a frame with compressor code 3 that is not stored raw, found by a
//             walk of the csize chain written here (so the streams of frames the plan leaves to
//             the host are judged too), goes through zlib's uncompress with the stream's raw size
//             as the room -- zlib_block of zh_blosc.cpp -- and through zh_bs::zlib_stream on one
//             lane (decode_zlib_stream<SerialLanes>, the size, the Adler-32 by adler32).  The two
//             must agree on accept / reject and, on accept, on every byte;
//   mutations the same for `mutations-per-stream` copies of every such stream of at most 64 KiB
//             with one byte replaced or one bit flipped (xorshift64 from `seed`);
//   frame     the plan's verdict (build_table with the flag), and for a frame it admits
//             decode_frame_serial with the flag: the whole route on one lane.
// Every buffer is a heap block of its exact size, so the sanitizer sees any access past either
// end.  One line per frame:
//   <where: 0 device, 1 host, 2 memcpyed, -1 header refused> <zh_status of decode_frame_serial>
//   <XXH64 of the decoded bytes, 16 hex digits; 0 unless where 0 and status 0> <streams judged>
// then `mutations <n>`.  The test compares the lines with zh_blosc_batch_plan_ex and
// zh_blosc_decompress.  Exit status 1 when a stream is judged differently.
#include <zlib.h>

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

uint64_t g_rng = 1;
uint64_t next_random() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

int g_bad = 0;
long g_mutations = 0;

// One stream (an exact heap copy) by both decoders.  False (and a line) when they disagree.
bool judge(const uint8_t* s, uint32_t n, uint32_t rawsize, const char* what, long frame) {
  uint8_t* want = exact(rawsize);
  uLongf dl = (uLongf)rawsize;
  const bool zok = uncompress(want, &dl, s, (uLong)n) == Z_OK && dl == (uLongf)rawsize;
  uint8_t* got = exact(rawsize);
  zh_gd::Work* W = (zh_gd::Work*)malloc(sizeof(zh_gd::Work));
  memset(W, 0xA5, sizeof *W);  // nothing may depend on what an earlier stream left
  zh_gd::SerialLanes lanes;
  const zh_gd::Verdict v = zh_bs::zlib_stream(s, n, got, rawsize, *W, lanes);
  bool same = (v == zh_gd::kOk) == zok;
  if (!same)
    fprintf(stderr, "frame %ld, %s: zlib_stream %s (verdict %d), uncompress %s\n", frame, what,
           v == zh_gd::kOk ? "accepts" : "rejects", (int)v, zok ? "accepts" : "rejects");
  if (same && zok && memcmp(got, want, rawsize) != 0) {
    fprintf(stderr, "frame %ld, %s: decoded bytes differ from zlib's\n", frame, what);
    same = false;
  }
  free(W);
  free(got);
  free(want);
  if (!same) g_bad = 1;
  return same;
}

// The streams of a zlib frame that are not stored raw: build_table's walk without its verdicts
// on a stream's first bytes, every field checked against the frame.
struct Found {
  size_t off;
  uint32_t csize, rawsize;
};
std::vector<Found> find_streams(const uint8_t* f, size_t len, const zh_bs::Header& h) {
  std::vector<Found> out;
  for (size_t k = 0; k < h.nblocks; k++) {
    const size_t bs = k + 1 < h.nblocks ? h.blocksize : h.nbytes - k * h.blocksize;
    const size_t nsplit = ((h.flags & 0x10) || bs < h.blocksize) ? 1 : h.typesize;
    if (nsplit > 1 && bs % nsplit != 0) return out;
    const size_t neb = bs / nsplit;
    size_t p = zh_bs::rd32(f + 16 + 4 * k);
    for (size_t s = 0; s < nsplit; s++) {
      if (p > len || len - p < 4) return out;
      const size_t cs = zh_bs::rd32(f + p);
      p += 4;
      if (cs > len - p) return out;
      if (cs != neb) out.push_back({p, (uint32_t)cs, (uint32_t)neb});
      p += cs;
    }
  }
  return out;
}

void check_frame(const uint8_t* frame, size_t len, long index, long mutations) {
  zh_bs::Header h;
  const char* msg = "";
  if (zh_bs::parse_header(frame, len, &h, &msg) != ZH_OK) {
    printf("-1 0 %016llx 0\n", 0ull);
    return;
  }
  int where = zh_bs::frame_where(h);
  if (where == 2 || h.comp != 3) {  // not this route's
    printf("%d 0 %016llx 0\n", where, 0ull);
    return;
  }
  const std::vector<Found> found = find_streams(frame, len, h);
  for (const Found& s : found) {
    uint8_t* copy = exact(s.csize);
    memcpy(copy, frame + s.off, s.csize);
    judge(copy, s.csize, s.rawsize, "stream", index);
    for (long m = 0; m < mutations && s.csize > 0 && s.rawsize <= (64u << 10); m++) {
      const size_t at = (size_t)(next_random() % s.csize);
      const uint8_t old = copy[at];
      const uint64_t r = next_random();
      copy[at] = (m & 1) ? (uint8_t)(old ^ (1u << (r & 7))) : (uint8_t)(old + 1 + r % 255);
      judge(copy, s.csize, s.rawsize, "mutation", index);
      copy[at] = old;
      g_mutations++;
    }
    free(copy);
  }
  std::vector<zh_bs::BlockRow> blocks;
  std::vector<zh_bs::StreamRow> streams;
  {
    std::vector<zh_bs::BlockRow> pb;
    std::vector<zh_bs::StreamRow> ps;
    if (zh_bs::build_table(frame, len, h, pb, ps, &msg, ZH_BLOSC_ZLIB_DEVICE) == ZH_OK) where = 0;
  }
  if (where != 0) {
    printf("%d 0 %016llx %zu\n", where, 0ull, found.size());
    return;
  }
  const size_t tb = h.blocksize < h.nbytes ? h.blocksize : h.nbytes;
  uint8_t* dst = exact(h.nbytes);
  uint8_t* tmp = exact(tb);
  const int st = zh_bs::decode_frame_serial(frame, len, dst, h.nbytes, tmp, blocks, streams, &msg,
                                            ZH_BLOSC_ZLIB_DEVICE);
  printf("0 %d %016llx %zu\n", st, (unsigned long long)(st == ZH_OK ? xxh64(dst, h.nbytes) : 0),
         found.size());
  free(tmp);
  free(dst);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 && argc != 4) {
    fprintf(stderr, "usage: %s frames.bin [mutations-per-stream seed]\n", argv[0]);
    return 2;
  }
  const long mutations = argc == 4 ? atol(argv[2]) : 0;
  if (argc == 4) g_rng = strtoull(argv[3], nullptr, 10) | 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  for (long k = 0;; k++) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const size_t len = zh_bs::rd32(lb);
    uint8_t* frame = exact(len);
    if (len && fread(frame, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    check_frame(frame, len, k, mutations);
    free(frame);
  }
  fclose(f);
  printf("mutations %ld\n", g_mutations);
  return g_bad;
}
