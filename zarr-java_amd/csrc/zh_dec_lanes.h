// zh_dec_lanes.h — the lane policy of the frame decoders (zh_zstd_dec.h, zh_gzip_dec.h) for one
// wave.  Included by .hip files only, each of which gets its own copy (anonymous namespace).
//   order    a match reads bytes that other lanes of the same wave stored earlier, in the
//            destination in global memory; the tables in LDS are read by other lanes than wrote
//            them.  ZdLanes::order is WaveCopy::order of zh_blosc_kernels.hip and the argument is
//            the one in that file's header ("order": the wave's own stores have reached the CU's
//            L1 / L2 when vmcnt returns to 0, LDS operations of a wave complete in order).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

struct ZdLanes {
  static constexpr uint32_t W = 64;
  uint32_t l;
  __device__ uint32_t lane() const { return l; }
  __device__ bool first() const { return l == 0; }
  __device__ static void order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ bool all(bool v) { return __all(v ? 1 : 0) != 0; }
  __device__ void copy(uint8_t* d, const uint8_t* s, uint64_t n) {
    for (uint64_t k = l; k < n; k += 64) d[k] = s[k];
  }
  __device__ void fill(uint8_t* d, uint32_t v, uint64_t n) {
    for (uint64_t k = l; k < n; k += 64) d[k] = (uint8_t)v;
  }
  __device__ void match(uint8_t* d, uint64_t o, uint64_t off, uint64_t n) {
    order();
    const uint8_t* b = d + o - off;
    if (off >= n) {
      for (uint64_t k = l; k < n; k += 64) d[o + k] = b[k];
    } else {  // pattern replication: only bytes below o are read
      for (uint64_t k = l; k < n; k += 64) d[o + k] = b[k % off];
    }
  }
  // a literal run of the gzip decoder: lane k holds the k-th byte; one coalesced store
  __device__ void spread(uint8_t* d, uint32_t v, uint32_t n) {
    if (l < n) d[l] = (uint8_t)v;
  }
  // the Adler-32 step of a zlib stream: the wave's sum in every lane (a butterfly of six
  // cross-lane exchanges; no memory)
  __device__ uint32_t sum(uint32_t v) {
    for (int m = 32; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
  }
};

}  // namespace
