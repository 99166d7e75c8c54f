// zh_lz_match.h — the lane-wise match finder the frame writers share (the blosc1 LZ4 writer of
// zh_blosc_enc.h and the zstd writer of zh_zstd_enc.h), and its host lane policy.
//
// The algorithm is stated for the 64 lanes of a wave: at cursor p lane l looks at p + l, hashes
// 4 bytes, reads its candidate from the table, checks the 4 bytes (failing that, the 4 bytes one
// position back: a run, which the table cannot know inside one step; a policy set `wide` then
// tries 2, 4 and 8 positions back as well: runs of whole elements); the lowest matching lane
// wins, the match is extended 64 bytes per step, the table takes the positions before the new
// cursor, the cursor moves behind the match.
// Determinism rule: lookups of one step see the table as the previous step left it, and two
// lanes that hash to one slot resolve by maximum (the slot keeps the highest position + 1), so
// what a writer emits is a pure function of its input bytes.  A lane policy W:
//     void     clear(uint32_t* table)
//     uint32_t find(s, p, lim, table, &ref)   lowest lane whose candidate matches (64: none);
//                                             keeps every lane's hash for insert
//     void     insert(p, end, table)          table[hash] = max(., q + 1) for p <= q < end
//     uint32_t extend(s, a, b, maxn)          leading k < maxn with s[a + k] == s[b + k]
//     void     copy(d, s, n)  /  lenbytes(d, v)  /  put(d, byte)  /  put16(d, v)
// HostLanes loops over the 64 lane indices; WaveLanes (zh_enc_device.h) is one wave.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "zh_blosc_streams.h"

namespace zh_lz {

constexpr uint32_t kMaxBlock = 64u << 10;  // positions fit 16 bits; a block stays in LDS
constexpr uint32_t kHashBits = 10;
constexpr uint32_t kHashSize = 1u << kHashBits;  // uint32 slots per wave: position + 1, 0 empty
constexpr uint32_t kMinMatch = 4;                // find checks 4 bytes

ZH_BS_HD uint32_t ld32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
ZH_BS_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// The 64 lanes as a loop: the host form of the lane policy.
struct HostLanes {
  uint32_t h[64];
  bool wide = false;  // find also looks 2, 4 and 8 bytes back (the zstd writer)
  void clear(uint32_t* table) {
    for (uint32_t i = 0; i < kHashSize; i++) table[i] = 0;
  }
  uint32_t find(const uint8_t* s, uint32_t p, uint32_t lim, const uint32_t* table,
                uint32_t* ref) {
    uint32_t best = 64;
    for (uint32_t l = 0; l < 64; l++) {
      const uint32_t q = p + l;
      if (q > lim) break;
      const uint32_t v = ld32(s + q);
      h[l] = hash4(v);
      const uint32_t c = table[h[l]];
      if (best != 64) continue;
      if (c != 0 && ld32(s + c - 1) == v) {
        best = l;
        *ref = c - 1;
      } else if (q >= 1 && ld32(s + q - 1) == v) {  // a run: the table only knows earlier steps
        best = l;
        *ref = q - 1;
      } else if (wide) {  // a run of 2-, 4- or 8-byte elements
        for (uint32_t d = 2; d <= 8; d *= 2)
          if (q >= d && ld32(s + q - d) == v) {
            best = l;
            *ref = q - d;
            break;
          }
      }
    }
    return best;
  }
  void insert(uint32_t p, uint32_t end, uint32_t* table) {
    for (uint32_t l = 0; l < 64 && p + l < end; l++)
      if (table[h[l]] < p + l + 1) table[h[l]] = p + l + 1;
  }
  uint32_t extend(const uint8_t* s, uint32_t a, uint32_t b, uint32_t maxn) {
    uint32_t k = 0;
    while (k < maxn && s[a + k] == s[b + k]) k++;
    return k;
  }
  void copy(uint8_t* d, const uint8_t* s, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) d[k] = s[k];
  }
  void lenbytes(uint8_t* d, uint32_t v) {
    const uint32_t nfull = v / 255;
    for (uint32_t k = 0; k < nfull; k++) d[k] = 255;
    d[nfull] = (uint8_t)(v % 255);
  }
  void put(uint8_t* d, uint32_t b) { *d = (uint8_t)b; }
  void put16(uint16_t* d, uint32_t v) { *d = (uint16_t)v; }
};

}  // namespace zh_lz
