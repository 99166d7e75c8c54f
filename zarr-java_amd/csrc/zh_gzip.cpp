// zh_gzip.cpp — the host side of gzip members.  No device.
// Writing: the host form of the member writer (zh_gzip_enc.h over HostLanes), the byte-for-byte
// oracle of the device batch (zh_gzip_enc_kernels.hip), and CRC-32 with zlib's chaining.
// Reading: zh_gzip_decompress runs the member decoder of zh_gzip_dec.h, the one the device kernel
// runs (zh_gzip_dec_kernels.hip), on one lane, compares the CRC-32 and has the status and text of
// every reason the decoder gives; zh_gzip_batch_plan walks the members' headers for the device
// batch; zh_debug_gzip_blocks lists a member's DEFLATE blocks.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "../../include/zarrhip.h"
#include "zh_gzip_dec.h"
#include "zh_gzip_enc.h"

namespace zh {
int gzip_plan(zh_gzip_frame* frames, int64_t n, int64_t* total, char* err, size_t errlen);
}

namespace {

void set_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) {
    strncpy(err, msg, errlen - 1);
    err[errlen - 1] = 0;
  }
}

// The status and text of every reason zh_gzip_dec.h rejects a member for; the texts follow zlib's.
struct Text {
  zh_gd::Verdict why;
  int status;
  const char* msg;
};
const Text& text_of(zh_gd::Verdict v) {
  using namespace zh_gd;
  static const Text T[] = {
    {kBadMagic, ZH_EDATA, "gzip: incorrect header check"},
    {kBadMethod, ZH_EDATA, "gzip: unknown compression method"},
    {kReservedFlag, ZH_EDATA, "gzip: unknown header flags set"},
    {kHeaderTruncated, ZH_EDATA, "gzip: header truncated"},
    {kHeaderCrc, ZH_EDATA, "gzip: header crc mismatch"},
    {kBlockType, ZH_EDATA, "gzip: invalid block type"},
    {kStoredLen, ZH_EDATA, "gzip: invalid stored block lengths"},
    {kTooManyCodes, ZH_EDATA, "gzip: too many length or distance symbols"},
    {kCodeLengthSet, ZH_EDATA, "gzip: invalid code lengths set"},
    {kRepeat, ZH_EDATA, "gzip: invalid bit length repeat"},
    {kNoEndOfBlock, ZH_EDATA, "gzip: invalid code -- missing end-of-block"},
    {kLitLenSet, ZH_EDATA, "gzip: invalid literal/lengths set"},
    {kDistSet, ZH_EDATA, "gzip: invalid distances set"},
    {kLitLenCode, ZH_EDATA, "gzip: invalid literal/length code"},
    {kDistCode, ZH_EDATA, "gzip: invalid distance code"},
    {kDistTooFar, ZH_EDATA, "gzip: invalid distance too far back"},
    {kTruncated, ZH_EDATA, "gzip: incomplete or truncated stream"},
    {kNoRoom, ZH_EINVAL, "gzip: decoded data exceeds the output buffer"},
    {kTrailerTruncated, ZH_EDATA, "gzip: trailer truncated"},
    {kSizeMismatch, ZH_EDATA, "gzip: incorrect length check"},
    {kCrcMismatch, ZH_EDATA, "gzip: incorrect data check"},
    {kNotToTheEnd, ZH_EDATA, "gzip: bytes after the member"},
    // a zlib stream's (decode_zlib_stream): no gzip member is rejected for these
    {kZlibHeader, ZH_EDATA, "zlib: incorrect header check"},
    {kZlibDictionary, ZH_EDATA, "zlib: need dictionary"},
    {kZlibTrailerTruncated, ZH_EDATA, "zlib: trailer truncated"},
    {kAdlerMismatch, ZH_EDATA, "zlib: incorrect data check"},
  };
  static_assert(sizeof T / sizeof T[0] == kVerdicts - 1, "a reason without a text");
  for (const Text& t : T)
    if (t.why == v) return t;
  return T[0];  // not reached: every reason has its row
}

int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// The plan of zh_gzip_batch_plan / zh_gzip_decode_batch: the header of every frame, no block.
int zh::gzip_plan(zh_gzip_frame* frames, int64_t n, int64_t* total, char* err, size_t errlen) {
  if (n < 0 || (n > 0 && !frames)) {
    set_err(err, errlen, "zh_gzip_batch_plan: no frames");
    return ZH_EINVAL;
  }
  int64_t pos = 0;
  for (int64_t i = 0; i < n; i++) {
    zh_gzip_frame& f = frames[i];
    if (f.srclen < 0 || (!f.src && f.srclen)) {
      f.status = ZH_EINVAL;
      set_err(err, errlen, "zh_gzip_batch_plan: negative frame length");
      return ZH_EINVAL;
    }
    static const uint8_t none = 0;
    const uint8_t* s = f.src ? (const uint8_t*)f.src : &none;
    const size_t len = (size_t)f.srclen;
    size_t hsize = 0;
    const zh_gd::Verdict v = zh_gd::member_header(s, len, &hsize);
    if (v) {
      f.status = text_of(v).status;
      set_err(err, errlen, text_of(v).msg);
      return f.status;
    }
    // the device takes a member whose last four bytes can be its size: DEFLATE expands a byte
    // 1032 times at the most
    const uint64_t isize = len - hsize >= 10 ? zh_gd::rd_le(s + len - 4, 4) : 0;
    f.where = 1;
    if (!f.host_only && len - hsize >= 10 &&
        isize <= (uint64_t)zh_gd::kMaxExpand * (uint64_t)(len - hsize - 8)) {
      f.where = 0;
      f.nbytes = (int64_t)isize;
      f.status = ZH_OK;
    } else {
      size_t nb = 0;
      char msg[256] = "";
      f.status = zh_gzip_decompress(s, len, nullptr, 0, &nb, msg, sizeof msg);
      if (f.status != ZH_OK) {
        set_err(err, errlen, msg);
        return f.status;
      }
      f.nbytes = (int64_t)nb;
    }
    f.dst_off = pos;
    pos = up256(pos + f.nbytes);
  }
  *total = pos;
  return ZH_OK;
}

extern "C" {

// Size query (dst == NULL): a pass that stores nothing, never ISIZE alone.  Decode: dstcap must
// hold the content; the CRC-32 is compared afterwards.
int zh_gzip_decompress(const void* src, size_t srclen, void* dst, size_t dstcap, size_t* dstlen,
                       char* err, size_t errlen) {
  if (!src || !dstlen) return ZH_EINVAL;
  std::unique_ptr<zh_gd::Work> w(new (std::nothrow) zh_gd::Work);
  if (!w) {
    set_err(err, errlen, "gzip: out of memory");
    return ZH_ENOMEM;
  }
  uint64_t made = 0;
  size_t used = 0;
  uint32_t crc = 0;
  zh_gd::Verdict v;
  if (dst) {
    zh_gd::SerialLanes lanes;
    v = zh_gd::decode_member((const uint8_t*)src, srclen, (uint8_t*)dst, dstcap, *w, lanes, &made,
                             &used, &crc);
    if (!v && crc != zh_crc32(zh_crc32(0, nullptr, 0), dst, (size_t)made))
      v = zh_gd::kCrcMismatch;
  } else {
    zh_gd::CountLanes lanes;
    uint8_t nowhere;
    v = zh_gd::decode_member((const uint8_t*)src, srclen, &nowhere, UINT64_MAX, *w, lanes, &made,
                             &used, &crc);
  }
  if (v) {
    set_err(err, errlen, text_of(v).msg);
    return text_of(v).status;
  }
  *dstlen = (size_t)made;
  return ZH_OK;
}

int64_t zh_gzip_batch_plan(zh_gzip_frame* frames, int64_t n, char* err, size_t errlen) {
  int64_t total = 0;
  const int st = zh::gzip_plan(frames, n, &total, err, errlen);
  return st == ZH_OK ? total : -(int64_t)st;
}

int64_t zh_debug_gzip_blocks(const void* src, size_t srclen, int64_t* rows, int64_t cap, char* err,
                             size_t errlen) {
  if (!src && srclen) return -(int64_t)ZH_EINVAL;
  static const uint8_t none = 0;
  std::unique_ptr<zh_gd::Work> w(new (std::nothrow) zh_gd::Work);
  const int64_t room = rows && cap > 0 ? cap : 0;
  std::unique_ptr<zh_gd::BlockInfo[]> info(new (std::nothrow) zh_gd::BlockInfo[room ? room : 1]);
  if (!w || !info) return -(int64_t)ZH_ENOMEM;
  zh_gd::Trace tr = {info.get(), room, 0};
  zh_gd::CountLanes lanes;
  uint8_t nowhere;
  uint64_t made = 0;
  size_t used = 0;
  uint32_t crc = 0;
  const zh_gd::Verdict v = zh_gd::decode_member<zh_gd::CountLanes, true>(
      src ? (const uint8_t*)src : &none, srclen, &nowhere, UINT64_MAX, *w, lanes, &made, &used,
      &crc, &tr);
  if (v) {
    set_err(err, errlen, text_of(v).msg);
    return -(int64_t)text_of(v).status;
  }
  static_assert(sizeof(zh_gd::BlockInfo) == 9 * sizeof(int64_t), "rows of 9 int64");
  for (int64_t k = 0; k < tr.n && k < room; k++) memcpy(rows + 9 * k, &info[k], sizeof info[k]);
  return tr.n;
}

int zh_gzip_compress(const void* src, size_t n, const zh_gzip_enc_params* params, void* dst,
                     size_t cap, size_t* len, char* err, size_t errlen) {
  const char* msg = "";
  try {
    const int st = zh_gz::compress_member((const uint8_t*)src, n, params, (uint8_t*)dst, cap, len,
                                          &msg);
    if (st != ZH_OK) set_err(err, errlen, msg);
    return st;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, "gzip: out of memory");
    return ZH_ENOMEM;
  }
}

uint32_t zh_crc32(uint32_t crc, const void* data, size_t len) {
  if (!data) return 0;  // zlib: the initial value
  return ~zh_gz::crc_raw(~crc, (const uint8_t*)data, len);
}

}  // extern "C"
