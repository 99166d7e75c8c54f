// gzip_enc_check — host-only checker of the gzip member writer (csrc/zh_gzip_enc.h), built with
// -fsanitize=address,undefined by tests/test_gzip_encode_host.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o gzip_enc_check tools/gzip_enc_check.cpp -lz
//   gzip_enc_check buffers.bin members.bin [dynamic]
//
// dynamic (0 or 1, default 0): zh_gzip_enc_params::dynamic for every buffer.
// buffers.bin: per buffer two little-endian uint32 (length, blocksize) and the bytes.  Every
// buffer is compressed with the host form of the writer (the lane loop the kernel runs as one
// wave, the serial coder whose wave form the second kernel is), decoded again with zlib's inflate
// (gzip wrapper, which verifies CRC-32 and ISIZE) and compared; the span-wise CRC-32 the device
// batch computes (pieces of 256 bytes folded as its tree folds them, spans of 64 KiB folded as
// its host side folds them) is compared with zh_crc32; members.bin receives, per buffer, a
// uint32 length and the member, for the caller to compare with zh_gzip_compress.  One line per
// buffer:
//   <zh_status> <member bytes> <ok | MISMATCH | message>
// Exit status 1 when a member did not decode to its buffer.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/zh_gzip.cpp"

static uint32_t rd32le(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// CRC-32 as the device batch computes it: whole 256-byte pieces of a 64 KiB span folded
// pairwise, the span's tail added bytewise, the spans folded, the register finished.
static uint32_t crc_by_spans(const uint8_t* p, size_t n) {
  const size_t kSpan = 64u << 10, kPiece = 256;
  uint32_t r = 0;
  for (size_t o = 0; o < n; o += kSpan) {
    const size_t len = n - o < kSpan ? n - o : kSpan;
    const size_t nfull = len / kPiece;
    uint32_t red[256] = {0};
    for (size_t t = 256 - nfull; t < 256; t++)
      red[t] = zh_gz::crc_raw(0, p + o + (t - (256 - nfull)) * kPiece, kPiece);
    uint32_t m = zh_gz::xpow8(kPiece);
    for (size_t step = 1; step < 256; step *= 2) {
      for (size_t t = 2 * step - 1; t < 256; t += 2 * step)
        red[t] = zh_gz::crc_append(red[t - step], red[t], m);
      m = zh_gz::mulmod(m, m);
    }
    const uint32_t span = zh_gz::crc_raw(red[255], p + o + nfull * kPiece, len - nfull * kPiece);
    r = zh_gz::crc_append(r, span, zh_gz::xpow8(len));
  }
  return zh_gz::crc_finish(r, n);
}

static bool inflate_gzip(const uint8_t* src, size_t srclen, uint8_t* dst, size_t cap,
                         size_t* got) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 31) != Z_OK) return false;
  zs.next_in = (Bytef*)src;
  zs.avail_in = (uInt)srclen;
  zs.next_out = dst;
  zs.avail_out = (uInt)cap;
  const int rc = inflate(&zs, Z_FINISH);
  *got = zs.total_out;
  const bool ok = rc == Z_STREAM_END && zs.avail_in == 0;
  inflateEnd(&zs);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    fprintf(stderr, "usage: %s buffers.bin members.bin [dynamic]\n", argv[0]);
    return 2;
  }
  const int32_t dynamic = argc == 4 ? (int32_t)atoi(argv[3]) : 0;
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) {
    perror(!f ? argv[1] : argv[2]);
    return 2;
  }
  int bad = 0;
  for (;;) {
    uint8_t hb[8];
    if (fread(hb, 1, 8, f) != 8) break;
    const size_t len = rd32le(hb);
    zh_gzip_enc_params prm;
    memset(&prm, 0, sizeof prm);
    prm.blocksize = (int32_t)rd32le(hb + 4);
    prm.dynamic = dynamic;
    // exact-size heap copies: the sanitizer sees any access past either end
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) {
      fprintf(stderr, "short input file\n");
      return 2;
    }
    const char* msg = "";
    size_t bound = 0, flen = 0;
    int st = zh_gz::compress_member(buf, len, &prm, nullptr, 0, &bound, &msg);
    uint8_t* member = (uint8_t*)malloc(bound ? bound : 1);
    if (st == ZH_OK) st = zh_gz::compress_member(buf, len, &prm, member, bound, &flen, &msg);
    const char* verdict = msg;
    if (st == ZH_OK) {
      uint8_t* exact = (uint8_t*)malloc(flen);  // the decoder sees exactly the member
      memcpy(exact, member, flen);
      uint8_t* dst = (uint8_t*)malloc(len ? len : 1);
      size_t got = 0;
      const bool same = inflate_gzip(exact, flen, dst, len, &got) && got == len &&
                        flen <= bound && (len == 0 || memcmp(dst, buf, len) == 0) &&
                        crc_by_spans(buf, len) == zh_crc32(0, buf, len) &&
                        zh_crc32(0, buf, len) == (uint32_t)crc32(0, buf, (uInt)len);
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
    free(member);
    free(buf);
  }
  fclose(f);
  fclose(g);
  return bad ? 1 : 0;
}
