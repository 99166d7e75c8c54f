// zstd_dec_check — host-only checker of the zstd frame decoder (csrc/zh_zstd_dec.h) and of its
// host caller zh_zstd_decompress (csrc/zh_zstd.cpp), built with -fsanitize=address,undefined by
// tests/test_zstd_batch_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o zstd_dec_check tools/zstd_dec_check.cpp csrc/zh_zstd.cpp
//   zstd_dec_check frames.bin
//
// frames.bin: per frame a little-endian uint32 length and the frame's bytes.  Every frame goes
// through zh_zstd_decompress (the loop over frames and the whole buffer: size query, then decode)
// and, when the header walk sends it to the device (zh_zd::walk_frame: one frame, content size,
// exact block chain), through decode_frame<SerialLanes> as the kernel calls it, into buffers of
// exactly the planned sizes.  The two must agree on accept / reject and, on accept, on every
// byte.  Every frame also goes through the policy that stores nothing (CountLanes), which must
// give the verdict and the byte count of a decoding pass with the same room.  One line per frame:
//   <where: 0 also decoded as the kernel does, 1 zh_zstd_decompress only, 2 skipped (a content
//    size above 256 MiB)>
//   <zh_status of zh_zstd_decompress>
//   <XXH64 of the decoded bytes, 16 hex digits; 0 when rejected> <zh_zstd_decompress's message>
// Exit status 1 when any frame disagrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/zarrhip.h"
#include "../csrc/zh_zstd_dec.h"

constexpr size_t kMaxContent = (size_t)256 << 20;

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
  int bad = 0;
  zh_zd::Work* W = (zh_zd::Work*)malloc(sizeof(zh_zd::Work));
  for (long k = 0;; k++) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const size_t len = zh_zd::rd_le(lb, 4);
    // exact-size heap copies: the sanitizer sees any access past either end
    uint8_t* frame = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(frame, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    char msg[256] = "";
    size_t n = 0;
    int st = zh_zstd_decompress(frame, len, nullptr, 0, &n, msg, sizeof msg);
    // what the size query said, or 1 MiB where it refused the frame: the room of the last check
    const size_t room = st == ZH_OK ? n : (size_t)1 << 20;
    uint8_t* host = nullptr;
    if (st == ZH_OK && n > kMaxContent) {  // a mutated content size: nothing here allocates it
      printf("2 %d %016llx content size beyond what this checker allocates\n", st, 0ull);
      free(frame);
      continue;
    }
    if (st == ZH_OK) {
      host = (uint8_t*)malloc(n ? n : 1);
      st = zh_zstd_decompress(frame, len, host, n, &n, msg, sizeof msg);
    }
    const zh_zd::Walk w = zh_zd::walk_frame<zh_zd::NoRows>(frame, len, nullptr);
    uint8_t* lit = (uint8_t*)malloc(zh_zd::kMaxRegen);
    zh_zd::Header h;
    uint64_t made = 0;
    size_t used = 0;
    if (w.device) {
      const size_t cap = (size_t)w.fcs;
      uint8_t* dst = (uint8_t*)malloc(cap ? cap : 1);
      uint8_t* wlit = (uint8_t*)malloc(w.max_regen ? (size_t)w.max_regen : 1);
      zh_zd::SerialLanes lanes;
      memset(W, 0xA5, sizeof *W);  // nothing may depend on what an earlier frame left
      bool ok = zh_zd::decode_frame(frame, len, dst, cap, wlit, (uint64_t)w.max_regen, *W, lanes,
                                    &made, &used, &h) == zh_zd::kOk &&
                made == cap && used == len;
      if (ok && w.csum) ok = (uint32_t)zh_xxh64(dst, cap, 0) == w.want;
      if (ok != (st == ZH_OK)) {
        fprintf(stderr, "frame %ld: decode_frame %s, zh_zstd_decompress status %d (%s)\n", k,
                ok ? "accepts" : "rejects", st, msg);
        bad = 1;
      } else if (ok && (n != cap || memcmp(dst, host, cap) != 0)) {
        fprintf(stderr, "frame %ld: decoded bytes differ\n", k);
        bad = 1;
      }
      free(wlit);
      free(dst);
    }
    // the first frame of the buffer, with the room the size query gave: storing and counting
    if (len >= 4 && zh_zd::rd_le(frame, 4) == zh_zd::kMagic) {
      uint8_t* dst = (uint8_t*)malloc(room ? room : 1);
      zh_zd::SerialLanes lanes;
      zh_zd::CountLanes count;
      uint64_t cmade = 0;
      size_t cused = 0;
      memset(W, 0xA5, sizeof *W);
      const zh_zd::Verdict vs = zh_zd::decode_frame(frame, len, dst, room, lit, zh_zd::kMaxRegen,
                                                    *W, lanes, &made, &used, &h);
      memset(W, 0xA5, sizeof *W);
      uint8_t nowhere;
      const zh_zd::Verdict vc = zh_zd::decode_frame(frame, len, &nowhere, room, lit,
                                                    zh_zd::kMaxRegen, *W, count, &cmade, &cused, &h);
      if (vs != vc || (vs == zh_zd::kOk && (made != cmade || used != cused))) {
        fprintf(stderr, "frame %ld: storing pass %d (%llu bytes), counting pass %d (%llu bytes)\n",
                k, (int)vs, (unsigned long long)made, (int)vc, (unsigned long long)cmade);
        bad = 1;
      }
      free(dst);
    }
    free(lit);
    printf("%d %d %016llx %s\n", w.device ? 0 : 1, st,
           (unsigned long long)(st == ZH_OK ? zh_xxh64(host, n, 0) : 0), st == ZH_OK ? "" : msg);
    free(host);
    free(frame);
  }
  free(W);
  fclose(f);
  return bad;
}
