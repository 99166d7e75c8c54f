// zh_gzip.cpp — the host form of the gzip member writer (zh_gzip_enc.h over HostLanes), the
// byte-for-byte oracle of the device batch (zh_gzip_enc_kernels.hip), and CRC-32 with zlib's
// chaining.  No device.  Members are read back by zlib (GzipCodec.decode), not here.
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/zarrhip.h"
#include "zh_gzip_enc.h"

namespace {

void set_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) {
    strncpy(err, msg, errlen - 1);
    err[errlen - 1] = 0;
  }
}

}  // namespace

extern "C" {

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
