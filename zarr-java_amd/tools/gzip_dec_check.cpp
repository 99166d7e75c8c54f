// gzip_dec_check — host-only checker of the gzip member decoder (csrc/zh_gzip_dec.h) against
// zlib's inflate, built with -fsanitize=address,undefined by tests/test_gzip_decode_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o gzip_dec_check tools/gzip_dec_check.cpp -lz
//   gzip_dec_check members.bin
//
// members.bin: per member a little-endian uint32 length and the member's bytes.  Every member goes
// through
//   zlib      inflate with windowBits 31 up to the end of the first member;
//   count     decode_member<CountLanes> with unbounded room: the size query;
//   store     decode_member<SerialLanes> into a buffer of exactly the counted size, and the
//             CRC-32 comparison;
//   kernel    when the batch plan would send the member to the device (the rule of
//             zh_gzip_batch_plan, on the header and the last four bytes), decode_member
//             <SerialLanes> as the kernel calls it: into a buffer of exactly the planned size,
//             accepted when it made that size, ended with the buffer and the CRC-32 matches.
// count and store must agree on the verdict and the byte count; store must agree with zlib on
// accept / reject and, on accept, on every byte; the kernel's call may refuse what zlib accepts
// (the batch then asks the host) but never the other way round, and its bytes are zlib's.
// One line per member: <0 kernel's call too, 1 not> <verdict of store> <bytes> ok.
// Exit status 1 when any member disagrees.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/zh_gzip_dec.h"

constexpr size_t kMaxContent = (size_t)256 << 20;

// zlib's view of the first member: 0 and the bytes, or an error code.
static int zlib_member(const uint8_t* src, size_t len, uint8_t** out, size_t* n) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 31) != Z_OK) return -100;
  size_t cap = 1 << 16;
  uint8_t* buf = (uint8_t*)malloc(cap);
  zs.next_in = (Bytef*)src;
  zs.avail_in = (uInt)len;
  int rc;
  for (;;) {
    zs.next_out = buf + zs.total_out;
    zs.avail_out = (uInt)(cap - zs.total_out);
    rc = inflate(&zs, Z_NO_FLUSH);
    if (rc != Z_OK) break;
    if (zs.avail_out == 0) {
      cap *= 2;
      buf = (uint8_t*)realloc(buf, cap);
    } else if (zs.avail_in == 0) {
      rc = Z_BUF_ERROR;  // the input ended before the member did
      break;
    }
  }
  *n = zs.total_out;
  *out = buf;
  inflateEnd(&zs);
  return rc == Z_STREAM_END ? 0 : rc;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s members.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int bad = 0;
  zh_gd::Work* W = (zh_gd::Work*)malloc(sizeof(zh_gd::Work));
  for (long k = 0;; k++) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const size_t len = zh_gd::rd_le(lb, 4);
    // exact-size heap copies: the sanitizer sees any access past either end
    uint8_t* m = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(m, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    uint8_t* want = nullptr;
    size_t nwant = 0;
    const bool zok = zlib_member(m, len, &want, &nwant) == 0;

    zh_gd::CountLanes count;
    uint64_t cmade = 0, smade = 0;
    size_t cused = 0, sused = 0;
    uint32_t ccrc = 0, scrc = 0;
    uint8_t nowhere;
    memset(W, 0xA5, sizeof *W);  // nothing may depend on what an earlier member left
    const zh_gd::Verdict vc =
        zh_gd::decode_member(m, len, &nowhere, UINT64_MAX, *W, count, &cmade, &cused, &ccrc);
    zh_gd::Verdict vs = vc;
    bool ok = false;
    if (vc == zh_gd::kOk && cmade <= kMaxContent) {
      uint8_t* dst = (uint8_t*)malloc(cmade ? (size_t)cmade : 1);
      zh_gd::SerialLanes lanes;
      memset(W, 0xA5, sizeof *W);
      vs = zh_gd::decode_member(m, len, dst, cmade, *W, lanes, &smade, &sused, &scrc);
      if (vs != vc || smade != cmade || sused != cused || scrc != ccrc) {
        printf("member %ld: storing pass %d (%llu bytes), counting pass %d (%llu bytes)\n", k,
               (int)vs, (unsigned long long)smade, (int)vc, (unsigned long long)cmade);
        bad = 1;
      }
      ok = vs == zh_gd::kOk && scrc == (uint32_t)crc32(crc32(0, nullptr, 0), dst, (uInt)smade);
      if (ok && zok && (smade != nwant || memcmp(dst, want, nwant) != 0)) {
        printf("member %ld: decoded bytes differ from zlib's\n", k);
        bad = 1;
      }
      free(dst);
    }
    if (ok != zok) {
      printf("member %ld: decode_member %s (verdict %d), zlib %s\n", k, ok ? "accepts" : "rejects",
             (int)vs, zok ? "accepts" : "rejects");
      bad = 1;
    }
    // the kernel's call: the plan's rule, the plan's room
    size_t hsize = 0;
    int where = 1;
    if (zh_gd::member_header(m, len, &hsize) == zh_gd::kOk && len - hsize >= 10) {
      const uint64_t isize = zh_gd::rd_le(m + len - 4, 4);
      if (isize <= (uint64_t)zh_gd::kMaxExpand * (len - hsize - 8) && isize <= kMaxContent) {
        where = 0;
        uint8_t* dst = (uint8_t*)malloc(isize ? (size_t)isize : 1);
        zh_gd::SerialLanes lanes;
        uint64_t made = 0;
        size_t used = 0;
        uint32_t crc = 0;
        memset(W, 0xA5, sizeof *W);
        const bool kok =
            zh_gd::decode_member(m, len, dst, isize, *W, lanes, &made, &used, &crc) ==
                zh_gd::kOk &&
            made == isize && used == len &&
            crc == (uint32_t)crc32(crc32(0, nullptr, 0), dst, (uInt)made);
        if (kok && (!zok || made != nwant || memcmp(dst, want, nwant) != 0)) {
          printf("member %ld: the kernel's call accepts other bytes than zlib's\n", k);
          bad = 1;
        }
        if (!kok && zok && cused == len) {  // one whole member, and still refused
          printf("member %ld: the kernel's call refuses a member zlib accepts\n", k);
          bad = 1;
        }
        free(dst);
      }
    }
    printf("%d %d %llu ok\n", where, (int)vs, (unsigned long long)(ok ? smade : 0));
    free(want);
    free(m);
  }
  free(W);
  fclose(f);
  return bad;
}
