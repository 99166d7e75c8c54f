// zh_gzip_enc_kernels.hip — gzip members written on the device, a batch at a time
// (zh_gzip_encode_bound / zh_gzip_encode_batch); the member and the block encoder are
// zh_gzip_enc.h, the host form zh_gzip_compress (zh_gzip.cpp) is the byte-for-byte oracle.
//
// The raw bytes are in device memory (zh_array_write's chunk buffers); the members go to the host.
//   gzip_crc32_kernel   one workgroup per (source, 64 KiB span), one launch for the whole batch
//           ahead of its slabs.  The span's whole 256-byte pieces are loaded into LDS as aligned
//           words shifted into place (any source alignment), 65 words apart so that the threads'
//           reads spread over the banks; thread t hashes one piece bytewise through a 256-entry
//           table in LDS; the pieces sit at the end of the thread row (a register that starts at
//           0 ignores leading zeros), so a tree of 8 steps folds them with x^(8 * 256 * 2^k);
//           the last thread adds the span's tail.  The host folds the spans of a source
//           (zh_gz::crc_append) and finishes the register (zh_gz::crc_finish).
//   gzip_match_kernel<CAP, WAVES>   one wave per block of at most CAP bytes (16 or 32 KiB by the
//           batch's block size), WAVES blocks per workgroup: the wave loads its block into its
//           part of LDS, next to its hash table, and runs zh_gz::match_block over WaveLanes;
//           the records go to the block's part of the list in global memory.  No barrier.
//   gzip_deflate_kernel<CAP, WAVES>   one wave per block, the wave form of
//           zh_gz::deflate_block: the block again in LDS, next to a zeroed window of its size;
//           the records are read 64 at a time; the lanes take 64 consecutive literals of a
//           record (or the pieces of its match), compute (bits, count) with the functions the
//           host form uses, a wave scan of the counts gives each lane its bit offset, and the
//           bits are OR-ed into the window (deterministic: OR commutes).  The finished segment
//           goes to the block's region of the scratch buffer in whole words; its size (or the
//           stored size) goes to a table.  The kernel boundary orders the records.  The form
//           with one thread per block that was built first took 113 ms where the match kernel
//           took 5.9 ms (DESIGN.md "Gzip members encoded on the device").
//   gzip_deflate_dyn_kernel<CAP, WAVES>   its sibling for zh_gzip_enc_params::dynamic = 1, the
//           wave form of zh_gz::deflate_block_dynamic (described at the kernel): a zh_gz::DynWork
//           in LDS per wave, 160 112 B per workgroup at 16 KiB;
//   host    one small copy brings the size table back; a prefix sum lays the members out and
//           builds the copy jobs;
//   blosc_gather_kernel (zh_enc_device.h)   one workgroup per job: headers and endings from the
//           uploaded table, fixed segments from the scratch, stored segments from the source
//           behind their 5 header bytes;
//   D2H     the compact buffer through the context's page-locked out ring into host memory.
// zh::gzip_segments_launch runs the match and the coding kernel over rows another writer built:
// the blosc writer's zlib streams (zh_blosc_enc_kernels.hip), a row per 16 KiB piece.
// encode_slab keeps the planning and the layout, which are this format; the slab's memory, marks,
// cutting and tail (caps, upload, gather, download, synchronise) are the driver of zh_enc_device.h.
// Slabs of at most kSlabBytes of raw input bound the device memory: per slab the scratch (the raw
// size and up to 23 bytes a block), the records (1.5 x), the compact members and the small tables.
// Every job and block row is built on the host from validated sizes; the size table is checked
// against the block sizes before it lays anything out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <vector>

#include "zh_ctx.h"
#include "zh_enc_device.h"
#include "zh_gzip_enc.h"

namespace {

constexpr uint32_t kSpan = 64u << 10;  // bytes per workgroup of the CRC kernel
constexpr uint32_t kPiece = 256;       // bytes per thread
constexpr uint32_t kPieceWords = kPiece / 4, kPieceStride = kPieceWords + 1;
static_assert(kSpan == kThreads * kPiece, "one piece per thread");
constexpr size_t kMetaStride = 32;  // per member: the header at 0, the ending and trailer at 10

struct CrcJob {
  uint64_t src;
  uint32_t len, pad;  // len <= kSpan
};

// The block into the wave's part of LDS: 16 bytes a lane where source and block agree on it.
__device__ inline void load_block(uint8_t* blk, const uint8_t* __restrict__ src, uint32_t size,
                                  uint32_t lane) {
  const uint32_t al = (uint32_t)(((uintptr_t)src) & 15);
  for (uint32_t q0 = lane * 16; q0 < size; q0 += 64 * 16) {
    const uint32_t cnt = size - q0 < 16u ? size - q0 : 16u;
    if (cnt == 16 && al == 0) {
      *(uint4*)(blk + q0) = *(const uint4*)(src + q0);
    } else if (cnt == 16 && (al & 3) == 0) {  // inner chunks behind a shard's index
      const uint32_t* s4 = (const uint32_t*)(src + q0);
      *(uint4*)(blk + q0) = make_uint4(s4[0], s4[1], s4[2], s4[3]);
    } else {
      for (uint32_t i = 0; i < cnt; i++) blk[q0 + i] = src[q0 + i];
    }
  }
}

template <uint32_t CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gzip_match_kernel(
    const EncRow* __restrict__ blocks, uint32_t nblocks, uint16_t* __restrict__ seqs,
    uint32_t* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[WAVES][CAP];
  __shared__ uint32_t tables[WAVES][zh_lz::kHashSize];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * WAVES + wave;
  if (k >= nblocks) return;  // the whole wave: the kernel has no barrier
  const EncRow b = blocks[k];
  if (b.size > CAP) return;  // never: the host picks CAP from the block size
  uint8_t* blk = lds[wave];
  load_block(blk, (const uint8_t*)b.src, b.size, lane);
  WaveLanes::order();
  WaveLanes w;
  w.lane = lane;
  w.h = 0;
  w.wide = true;
  uint32_t covered = 0;
  const uint32_t ns = zh_gz::match_block(blk, b.size, seqs + b.seq, tables[wave], w, &covered);
  if (lane == 0) {
    info[2 * k] = ns;
    info[2 * k + 1] = covered;
  }
}

// The wave form of zh_gz::deflate_block.  The bit position of a symbol is a prefix sum of code
// lengths: the lanes take 64 consecutive literals (or the pieces of one long match), compute
// (bits, count), a wave scan gives each lane its offset, and the bits are OR-ed into the block's
// zeroed window in LDS (OR commutes: the window does not depend on the order).  A literal is 8
// or 9 bits, so its scan is two ballots and two population counts; a match of one piece needs
// none; only the pieces of a match longer than 258 go through the shuffle scan.
struct WaveCoder {
  uint32_t* win;
  uint32_t lane, bitpos, limit;  // limit: the symbols' bits may reach it, not pass it
  bool over = false;

  __device__ void bits(uint32_t at, uint32_t v, uint32_t nb) {  // nb <= 32
    const uint64_t x = (uint64_t)v << (at & 31u);
    atomicOr(&win[at >> 5], (uint32_t)x);
    if ((at & 31u) + nb > 32) atomicOr(&win[(at >> 5) + 1], (uint32_t)(x >> 32));
  }
  // up to 64 literals in lane order: 8 bits, 9 where `nine`
  __device__ void literals(uint32_t v, bool act, bool nine) {
    const unsigned long long ma = __ballot(act), m9 = __ballot(act && nine);
    const uint32_t total = 8 * (uint32_t)__popcll(ma) + (uint32_t)__popcll(m9);
    if (bitpos + total > limit) {
      over = true;
      return;
    }
    const unsigned long long lower = (1ull << lane) - 1;
    if (act)
      bits(bitpos + 8 * (uint32_t)__popcll(ma & lower) + (uint32_t)__popcll(m9 & lower), v,
           nine ? 9u : 8u);
    bitpos += total;
  }
  // one symbol, the same in every lane
  __device__ void one(uint32_t v, uint32_t nb) {
    if (bitpos + nb > limit) {
      over = true;
      return;
    }
    if (lane == 0) bits(bitpos, v, nb);
    bitpos += nb;
  }
  // every lane's (v, nb), nb == 0 for a lane without a symbol, in lane order
  __device__ void put(uint32_t v, uint32_t nb) {
    uint32_t incl = nb;
    for (int d = 1; d < 64; d *= 2) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= (uint32_t)d) incl += y;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (bitpos + total > limit) {
      over = true;
      return;
    }
    if (nb) bits(bitpos + incl - nb, v, nb);
    bitpos += total;
  }
  // put() for symbols of up to 64 bits: the two halves of a match under the dynamic codes
  __device__ void put64(uint64_t v, uint32_t nb) {
    uint32_t incl = nb;
    for (int d = 1; d < 64; d *= 2) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= (uint32_t)d) incl += y;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (bitpos + total > limit) {
      over = true;
      return;
    }
    const uint32_t at = bitpos + incl - nb;
    if (nb) bits(at, (uint32_t)v, nb < 32u ? nb : 32u);
    if (nb > 32) bits(at + 32, (uint32_t)(v >> 32), nb - 32);
    bitpos += total;
  }
};

// The wave as the lane policy of the dynamic form's rules (zh_gzip_enc.h): 64 lanes, the wave's
// LDS ordered between the steps, a butterfly sum.
struct WaveDyn {
  uint32_t lane;
  static constexpr uint32_t n = 64;
  __device__ void order() { WaveLanes::order(); }
  __device__ uint32_t sum(uint32_t v) {
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
  }
};

template <uint32_t CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gzip_deflate_kernel(
    const EncRow* __restrict__ blocks, uint32_t nblocks, uint8_t* __restrict__ scratch,
    const uint16_t* __restrict__ seqs, const uint32_t* __restrict__ info,
    uint32_t* __restrict__ csize) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[WAVES][CAP];
  __shared__ uint32_t wins[WAVES][CAP / 4 + 4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * WAVES + wave;
  if (k >= nblocks) return;  // the whole wave: the kernel has no barrier
  const EncRow b = blocks[k];
  const uint32_t n = b.size, stored = n + zh_gz::kStoredOver;
  const uint32_t ns = info[2 * k], covered = info[2 * k + 1];
  // the tests of zh_gz::deflate_block before it codes anything, and the list's room
  if (n > CAP || ns > n / zh_lz::kMinMatch || covered > n ||
      (8 * (n - covered) + 12 * ns + 13 + 7) / 8 + 4 >= stored) {
    if (lane == 0) csize[k] = stored;
    return;
  }
  uint8_t* blk = lds[wave];
  uint32_t* win = wins[wave];
  load_block(blk, (const uint8_t*)b.src, n, lane);
  const uint32_t nwin = (n + 4) / 4 + 2;  // n + 4 bytes and the word a symbol may reach into
  for (uint32_t i = lane; i < nwin; i += 64) win[i] = i == 0 ? 2u : 0u;  // BFINAL 0, BTYPE 01
  WaveLanes::order();
  // a segment of more than n + 4 bytes is stored: end of block, marker bits, 4 marker bytes
  WaveCoder c{win, lane, 3, 8 * n - 10};
  const uint16_t* __restrict__ sq = seqs + b.seq;
  uint32_t pos = 0;
  for (uint32_t k0 = 0; k0 <= ns && !c.over; k0 += 64) {  // record ns: the literals at the end
    uint32_t r_lit = 0, r_ml = 0, r_off = 0;
    if (k0 + lane < ns) {
      r_lit = sq[3 * (k0 + lane)];
      r_ml = sq[3 * (k0 + lane) + 1];
      r_off = sq[3 * (k0 + lane) + 2];
    }
    const uint32_t cnt = ns + 1 - k0 < 64u ? ns + 1 - k0 : 64u;
    for (uint32_t j = 0; j < cnt && !c.over; j++) {
      const bool last = k0 + j == ns;
      const uint32_t lit = last ? n - pos : (uint32_t)__builtin_amdgcn_readlane((int)r_lit, j);
      const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)r_ml, j);
      const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)r_off, j);
      if (lit > n - pos) {  // never: the records partition the block
        c.over = true;
        break;
      }
      for (uint32_t i0 = 0; i0 < lit && !c.over; i0 += 64) {
        const bool act = i0 + lane < lit;
        uint32_t v = 0, nb = 0;
        if (act) v = zh_gz::lit_bits(blk[pos + i0 + lane], &nb);
        c.literals(v, act, nb == 9);
      }
      pos += lit;
      if (last || c.over) break;
      if (ml > n - pos || off == 0 || off > pos) {  // never
        c.over = true;
        break;
      }
      const uint32_t np = zh_gz::piece_count(ml);
      if (np == 1) {
        uint32_t nb;
        const uint32_t v = zh_gz::match_bits(ml, off, &nb);
        c.one(v, nb);
      }
      for (uint32_t p0 = 0; np > 1 && p0 < np && !c.over; p0 += 64) {
        uint32_t v = 0, nb = 0;
        if (p0 + lane < np) v = zh_gz::match_bits(zh_gz::piece_len(ml, p0 + lane), off, &nb);
        c.put(v, nb);
      }
      pos += ml;
    }
  }
  if (c.over) {
    if (lane == 0) csize[k] = stored;
    return;
  }
  const uint32_t bytes = (c.bitpos + 10 + 7) / 8;  // end of block, marker bits, zero bits
  if (lane == 0) {
    c.bits(8 * (bytes + 2), 0xFFFFu, 16);  // LEN 0, NLEN ffff
    csize[k] = bytes + 4;
  }
  WaveLanes::order();
  uint32_t* __restrict__ out = (uint32_t*)(scratch + b.out);  // 16-byte aligned, size + 8 long
  for (uint32_t i = lane; i < (bytes + 4 + 3) / 4; i += 64) out[i] = win[i];
}

// gzip_deflate_kernel with the dynamic form in the choice, the wave form of
// zh_gz::deflate_block_dynamic: next to the block and its window the wave has a zh_gz::DynWork in
// LDS.  Four steps:
//   histogram   the records 64 at a time (each lane the pieces of its own match) and the literals
//               64 at a time, added into the 316 counters with LDS atomics;
//   codes       zh_gz::plan_dynamic: the code lengths (the keys ranked by all lanes, the merge,
//               the depths and the header's run-length coding on the first lane), the exact sizes;
//   choice      zh_gz::choose_form, then the (code, length) tables of the form chosen: the fixed
//               codes are one such table, so one walk writes either form;
//   coding      the header's symbols 64 at a time and the block's symbols as in
//               gzip_deflate_kernel, looked up in the tables; the code lengths vary, so 64
//               literals take a wave scan; a match of one piece is two symbols from the first
//               lane.
// WaveLanes::order() stands between the atomics and every read of the counters, and between the
// first lane's tables and their readers (inside the shared steps).
template <uint32_t CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gzip_deflate_dyn_kernel(
    const EncRow* __restrict__ blocks, uint32_t nblocks, uint8_t* __restrict__ scratch,
    const uint16_t* __restrict__ seqs, const uint32_t* __restrict__ info,
    uint32_t* __restrict__ csize) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[WAVES][CAP];
  __shared__ uint32_t wins[WAVES][CAP / 4 + 4];
  __shared__ zh_gz::DynWork works[WAVES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * WAVES + wave;
  if (k >= nblocks) return;  // the whole wave: the kernel has no barrier
  const EncRow b = blocks[k];
  const uint32_t n = b.size, stored = n + zh_gz::kStoredOver;
  const uint32_t ns = info[2 * k], covered = info[2 * k + 1];
  if (n > CAP || ns > n / zh_lz::kMinMatch || covered > n) {
    if (lane == 0) csize[k] = stored;
    return;
  }
  uint8_t* blk = lds[wave];
  uint32_t* win = wins[wave];
  zh_gz::DynWork& d = works[wave];
  load_block(blk, (const uint8_t*)b.src, n, lane);
  const uint32_t nwin = (n + 4) / 4 + 2;  // n + 4 bytes and the word a symbol may reach into
  for (uint32_t i = lane; i < nwin; i += 64) win[i] = 0;
  for (uint32_t i = lane; i < zh_gz::kSyms; i += 64) d.hist[i] = 0;
  WaveLanes::order();
  const uint16_t* __restrict__ sq = seqs + b.seq;

  // the histogram, and the tests of zh_gz::hist_block
  bool bad = false;
  uint32_t pos = 0;
  for (uint32_t k0 = 0; k0 <= ns && !bad; k0 += 64) {
    uint32_t r_lit = 0, r_ml = 0, r_off = 0;
    if (k0 + lane < ns) {
      r_lit = sq[3 * (k0 + lane)];
      r_ml = sq[3 * (k0 + lane) + 1];
      r_off = sq[3 * (k0 + lane) + 2];
    }
    // a record the walk below refuses is not counted: its codes may lie outside the counters
    if (r_ml >= zh_gz::kMinPiece && r_off >= 1 && r_off <= zh_gz::kMaxBlock) {
      uint32_t eb, ex;
      const uint32_t np = zh_gz::piece_count(r_ml);
      for (uint32_t j = 0; j < np; j++)
        atomicAdd(&d.hist[257 + zh_gz::len_code(zh_gz::piece_len(r_ml, j), &eb, &ex)], 1u);
      atomicAdd(&d.hist[zh_gz::kLitLen + zh_gz::dist_code(r_off, &eb, &ex)], np);
    }
    const uint32_t cnt = ns + 1 - k0 < 64u ? ns + 1 - k0 : 64u;
    for (uint32_t j = 0; j < cnt; j++) {
      const bool last = k0 + j == ns;
      const uint32_t lit = last ? n - pos : (uint32_t)__builtin_amdgcn_readlane((int)r_lit, j);
      const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)r_ml, j);
      const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)r_off, j);
      if (lit > n - pos) {  // never: the records partition the block
        bad = true;
        break;
      }
      for (uint32_t i0 = 0; i0 < lit; i0 += 64)
        if (i0 + lane < lit) atomicAdd(&d.hist[blk[pos + i0 + lane]], 1u);
      pos += lit;
      if (last) break;
      if (ml < zh_gz::kMinPiece || ml > n - pos || off == 0 || off > pos) {  // never
        bad = true;
        break;
      }
      pos += ml;
    }
  }
  if (bad) {
    if (lane == 0) csize[k] = stored;
    return;
  }
  if (lane == 0) d.hist[zh_gz::kEob] = 1;  // no atomic adds to it
  WaveLanes::order();

  WaveDyn w{lane};
  zh_gz::plan_dynamic(d, w);
  uint32_t size = 0;
  const uint32_t form = zh_gz::choose_form(n, d, &size);
  if (form == 0) {
    if (lane == 0) csize[k] = stored;
    return;
  }
  zh_gz::form_tables(form, d, w);

  // The sizes are exact.  Here the header bits and the end-of-block code go through the coder
  // too (gzip_deflate_kernel adds its end-of-block code outside): size <= n + 4 means
  // ceil((bits + 3) / 8) <= n, so all of them end at 8 n - 3 bits or before, inside the window.
  WaveCoder c{win, lane, 0, 8 * n - 3};
  c.one(form == 2 ? 4u : 2u, 3);  // BFINAL 0, BTYPE 10 or 01
  if (form == 2) {
    c.one((d.hlit - 257) | (d.hdist - 1) << 5 | (d.hclen - 4) << 10, 14);
    c.put(lane < d.hclen ? d.cllens[zh_gz::cl_order(lane)] : 0u, lane < d.hclen ? 3u : 0u);
    for (uint32_t i0 = 0; i0 < d.nitems && !c.over; i0 += 64) {
      uint32_t v = 0, nb = 0;
      if (i0 + lane < d.nitems) {
        const uint32_t it = d.items[i0 + lane], sym = it & 31u;
        v = zh_gz::entry_bits(d.cltab[sym], it >> 5, zh_gz::cl_extra(sym), &nb);
      }
      c.put(v, nb);
    }
  }
  pos = 0;
  for (uint32_t k0 = 0; k0 <= ns && !c.over; k0 += 64) {  // record ns: the literals at the end
    uint32_t r_lit = 0, r_ml = 0, r_off = 0;
    if (k0 + lane < ns) {
      r_lit = sq[3 * (k0 + lane)];
      r_ml = sq[3 * (k0 + lane) + 1];
      r_off = sq[3 * (k0 + lane) + 2];
    }
    const uint32_t cnt = ns + 1 - k0 < 64u ? ns + 1 - k0 : 64u;
    for (uint32_t j = 0; j < cnt && !c.over; j++) {
      const bool last = k0 + j == ns;
      const uint32_t lit = last ? n - pos : (uint32_t)__builtin_amdgcn_readlane((int)r_lit, j);
      const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)r_ml, j);
      const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)r_off, j);
      for (uint32_t i0 = 0; i0 < lit && !c.over; i0 += 64) {
        const uint32_t t = i0 + lane < lit ? d.tab[blk[pos + i0 + lane]] : 0u;
        c.put(t & 0xFFFFu, t >> 16);
      }
      pos += lit;
      if (last || c.over) break;
      uint32_t eb, ex, nb1, nb2;
      const uint32_t dc = zh_gz::dist_code(off, &eb, &ex);
      const uint32_t v2 = zh_gz::entry_bits(d.tab[zh_gz::kLitLen + dc], ex, eb, &nb2);
      const uint32_t np = zh_gz::piece_count(ml);
      if (np == 1) {
        const uint32_t lc = zh_gz::len_code(ml, &eb, &ex);
        const uint32_t v1 = zh_gz::entry_bits(d.tab[257 + lc], ex, eb, &nb1);
        c.one(v1, nb1);
        if (!c.over) c.one(v2, nb2);
      }
      for (uint32_t p0 = 0; np > 1 && p0 < np && !c.over; p0 += 64) {
        uint64_t v = 0;
        uint32_t nb = 0;
        if (p0 + lane < np) {
          const uint32_t lc = zh_gz::len_code(zh_gz::piece_len(ml, p0 + lane), &eb, &ex);
          const uint32_t v1 = zh_gz::entry_bits(d.tab[257 + lc], ex, eb, &nb1);
          v = v1 | (uint64_t)v2 << nb1;
          nb = nb1 + nb2;
        }
        c.put64(v, nb);
      }
      pos += ml;
    }
  }
  if (!c.over) c.one(d.tab[zh_gz::kEob] & 0xFFFFu, d.tab[zh_gz::kEob] >> 16);
  const uint32_t bytes = (c.bitpos + 3 + 7) / 8;  // marker bits, zero bits
  if (c.over || bytes + 4 != size) {              // never: the sizes are exact
    if (lane == 0) csize[k] = stored;
    return;
  }
  if (lane == 0) {
    c.bits(8 * (bytes + 2), 0xFFFFu, 16);  // LEN 0, NLEN ffff
    csize[k] = size;
  }
  WaveLanes::order();
  uint32_t* __restrict__ out = (uint32_t*)(scratch + b.out);  // 16-byte aligned, size + 8 long
  for (uint32_t i = lane; i < (size + 3) / 4; i += 64) out[i] = win[i];
}

// One wave per histogram: zh_gz::code_lengths as the dynamic coder runs it
// (zh_debug_gzip_code_lengths).  255: no code.
__global__ __launch_bounds__(64) void gzip_code_lengths_kernel(const uint32_t* __restrict__ counts,
                                                               uint32_t nsym, uint32_t limit,
                                                               uint8_t* __restrict__ lens) {
  __shared__ zh_gz::DynWork d;
  const uint32_t lane = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * nsym;
  if (nsym > zh_gz::kLitLen) return;
  for (uint32_t i = lane; i < nsym; i += 64) d.hist[i] = counts[row + i];
  WaveLanes::order();
  WaveDyn w{lane};
  const bool ok = zh_gz::code_lengths(d.hist, nsym, limit, d.lens, d, w);
  for (uint32_t i = lane; i < nsym; i += 64) lens[row + i] = ok ? d.lens[i] : (uint8_t)255;
}

__global__ __launch_bounds__(kThreads) void gzip_crc32_kernel(const CrcJob* __restrict__ jobs,
                                                              uint32_t x_piece,
                                                              uint32_t* __restrict__ out) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t red[kThreads];
  __shared__ uint32_t words[kThreads * kPieceStride];
  const uint32_t t = threadIdx.x;
  tab[t] = zh_gz::crc_table_entry(t);
  const CrcJob job = jobs[blockIdx.x];
  const uint8_t* __restrict__ src = (const uint8_t*)job.src;
  const uint32_t len = job.len < kSpan ? job.len : kSpan;
  const uint32_t nfull = len / kPiece, nw = nfull * kPieceWords;
  const uint32_t sh = (uint32_t)(((uintptr_t)src) & 3);
  // aligned words; when sh != 0 the word behind holds the last byte of word j, inside the span
  const uint32_t* __restrict__ s4 = (const uint32_t*)(src - sh);
  for (uint32_t j = t; j < nw; j += kThreads) {
    const uint32_t x0 = s4[j];
    const uint32_t x1 = sh ? s4[j + 1] : 0u;
    words[(j / kPieceWords) * kPieceStride + j % kPieceWords] =
        sh ? __builtin_amdgcn_alignbyte(x1, x0, sh) : x0;
  }
  __syncthreads();
  const uint32_t first = kThreads - nfull;  // the pieces end the row: leading zeros are free
  uint32_t r = 0;
  if (t >= first) {
    const uint32_t* w = words + (t - first) * kPieceStride;
    for (uint32_t i = 0; i < kPieceWords; i++) {
      r ^= w[i];
      for (int q = 0; q < 4; q++) r = tab[r & 255u] ^ (r >> 8);
    }
  }
  red[t] = r;
  __syncthreads();
  uint32_t m = x_piece;  // x^(8 * kPiece * step)
  for (uint32_t step = 1; step < kThreads; step *= 2) {
    const uint32_t mask = 2 * step - 1;
    if ((t & mask) == mask) red[t] = zh_gz::crc_append(red[t - step], red[t], m);
    m = zh_gz::mulmod(m, m);
    __syncthreads();
  }
  if (t == kThreads - 1) {
    r = red[t];
    for (uint32_t q = nfull * kPiece; q < len; q++) r = tab[(r ^ src[q]) & 255u] ^ (r >> 8);
    out[blockIdx.x] = r;
  }
}

std::atomic<double> g_last_genc_ms{-1.0};
std::atomic<double> g_last_genc_part[4] = {{-1.0}, {-1.0}, {-1.0}, {-1.0}};
enum Part { kMatch = 0, kCoder = 1, kCrc = 2, kGather = 3 };

void launch_match(uint32_t B, hipStream_t s, const EncRow* blocks, uint32_t nblocks,
                  uint16_t* seqs, uint32_t* info) {
  if (B <= (16u << 10)) {
    hipLaunchKernelGGL((gzip_match_kernel<(16u << 10), 4>), dim3((nblocks + 3) / 4), dim3(256), 0,
                       s, blocks, nblocks, seqs, info);
  } else {
    hipLaunchKernelGGL((gzip_match_kernel<zh_gz::kMaxBlock, 4>), dim3((nblocks + 3) / 4),
                       dim3(256), 0, s, blocks, nblocks, seqs, info);
  }
}

void launch_deflate(const zh_gz::Params& P, hipStream_t s, const EncRow* blocks,
                    uint32_t nblocks, uint8_t* scratch, const uint16_t* seqs, const uint32_t* info,
                    uint32_t* csize) {
  const uint32_t B = P.B;
  if (P.dynamic && B <= (16u << 10)) {
    hipLaunchKernelGGL((gzip_deflate_dyn_kernel<(16u << 10), 4>), dim3((nblocks + 3) / 4),
                       dim3(256), 0, s, blocks, nblocks, scratch, seqs, info, csize);
  } else if (P.dynamic) {
    hipLaunchKernelGGL((gzip_deflate_dyn_kernel<zh_gz::kMaxBlock, 2>), dim3((nblocks + 1) / 2),
                       dim3(128), 0, s, blocks, nblocks, scratch, seqs, info, csize);
  } else if (B <= (16u << 10)) {
    hipLaunchKernelGGL((gzip_deflate_kernel<(16u << 10), 4>), dim3((nblocks + 3) / 4), dim3(256),
                       0, s, blocks, nblocks, scratch, seqs, info, csize);
  } else {
    hipLaunchKernelGGL((gzip_deflate_kernel<zh_gz::kMaxBlock, 2>), dim3((nblocks + 1) / 2),
                       dim3(128), 0, s, blocks, nblocks, scratch, seqs, info, csize);
  }
}

struct MemberPlan {
  int64_t first_block = 0, nblocks = 0;  // within the slab
};

// One slab [f0, f1) of the batch; crcs: the batch's, finished; *pos: the running offset in dst.
int encode_slab(zh_ctx* ctx, hipStream_t s, Ring& ring, const uint32_t* crcs,
                zh_gzip_enc_frame* frames, int64_t f0, int64_t f1, const zh_gz::Params& P,
                uint8_t* dst, int64_t* pos, double* part_ms) {
  const int64_t nf = f1 - f0;
  std::vector<MemberPlan> plan((size_t)nf);
  std::vector<EncRow> blocks;
  SlabLayout L;
  int64_t scratch_total = 0, seq_total = 0;
  for (int64_t i = f0; i < f1; i++) {
    MemberPlan& mp = plan[(size_t)(i - f0)];
    const size_t n = (size_t)frames[i].nbytes;
    mp.first_block = (int64_t)blocks.size();
    mp.nblocks = (int64_t)zh_gz::block_count(n, P.B);
    for (int64_t k = 0; k < mp.nblocks; k++) {
      EncRow b;
      b.size = zh_gz::block_size(n, P.B, (size_t)k);
      b.src = (uint64_t)(uintptr_t)frames[i].src + (uint64_t)k * P.B;
      b.out = (uint64_t)scratch_total;
      b.seq = (uint64_t)seq_total;
      b.pad = 0;
      blocks.push_back(b);
      scratch_total += up((int64_t)b.size + 8, 16);  // size + 4 bytes, stored as whole words
      seq_total += up(3 * (int64_t)(b.size / 4) + 3, 8);
    }
    L.compact_cap += up((int64_t)zh_gz::member_bound(n, P.B), 16);
    L.njobs_cap += 2 + 2 * mp.nblocks;
  }
  if (blocks.size() > (size_t)zh::kIntMax || L.njobs_cap > zh::kIntMax) return ZH_EINVAL;
  const size_t nb = blocks.size();
  L.meta_cap = nf * (int64_t)kMetaStride;

  // device memory: [blocks | info | csize | jobs | meta | seqs | scratch | compact]
  SlabMem mem;
  const size_t o_blocks = mem.add((int64_t)(nb * sizeof(EncRow)));
  const size_t o_info = mem.add((int64_t)nb * 8);
  const size_t o_cs = mem.add((int64_t)nb * 4);
  L.o_jobs = mem.add(L.njobs_cap * (int64_t)sizeof(GatherJob));
  L.o_meta = mem.add(L.meta_cap);
  const size_t o_seq = mem.add(seq_total * 2);
  const size_t o_scratch = mem.add(scratch_total);
  L.o_compact = mem.add(L.compact_cap);
  int rc = mem.alloc(ctx);
  if (rc != ZH_OK) return rc;
  Marks marks(s, 5);  // 0 match 1 coder 2, 3 gather 4
  std::vector<uint32_t> cs(nb, 0);
  if (nb && !ring.h2d(mem.at(o_blocks), (const uint8_t*)blocks.data(), nb * sizeof(EncRow)))
    rc = ZH_EHIP;
  if (rc == ZH_OK) {
    marks.mark(0);
    if (nb)
      launch_match(P.B, s, (const EncRow*)mem.at(o_blocks), (uint32_t)nb,
                   (uint16_t*)mem.at(o_seq), (uint32_t*)mem.at(o_info));
    marks.mark(1);
    if (nb)
      launch_deflate(P, s, (const EncRow*)mem.at(o_blocks), (uint32_t)nb, mem.at(o_scratch),
                     (const uint16_t*)mem.at(o_seq), (const uint32_t*)mem.at(o_info),
                     (uint32_t*)mem.at(o_cs));
    if (hipGetLastError() != hipSuccess) rc = ZH_EHIP;
    marks.mark(2);
  }
  if (rc == ZH_OK && nb && !ring.d2h((uint8_t*)cs.data(), mem.at(o_cs), nb * 4)) rc = ZH_EHIP;
  // the table lays out device copies: nothing in it may pass its block's stored size
  for (size_t k = 0; k < nb && rc == ZH_OK; k++)
    if (cs[k] < zh_gz::kMinSegment || cs[k] > blocks[k].size + zh_gz::kStoredOver) rc = ZH_EHIP;

  // layout: the members side by side in the compact buffer, each 16-byte aligned
  if (rc == ZH_OK) {
    L.meta.resize((size_t)nf * kMetaStride, 0);
    L.jobs.reserve((size_t)L.njobs_cap);
    const uint64_t d_meta = mem.addr(L.o_meta), d_scratch = mem.addr(o_scratch);
    const uint64_t d_compact = mem.addr(L.o_compact);
    for (int64_t i = f0; i < f1; i++) {
      const MemberPlan& mp = plan[(size_t)(i - f0)];
      const size_t n = (size_t)frames[i].nbytes;
      const size_t m0 = (size_t)(i - f0) * kMetaStride;
      zh_gz::put_header(L.meta.data() + m0);
      zh_gz::put_ending(L.meta.data() + m0 + zh_gz::kHeader, crcs[i], n);
      const uint64_t fbase = d_compact + (uint64_t)L.cpos;
      uint64_t d = fbase;
      L.jobs.push_back({d_meta + m0, d, (uint32_t)zh_gz::kHeader, 0, 0, 0});
      d += zh_gz::kHeader;
      for (int64_t k = 0; k < mp.nblocks; k++) {
        const EncRow& b = blocks[(size_t)(mp.first_block + k)];
        const uint32_t size = cs[(size_t)(mp.first_block + k)];
        if (size == b.size + zh_gz::kStoredOver) {  // 00, then LEN NLEN and the bytes
          L.jobs.push_back({d_meta + m0, d, 0, 0, 1, 0});
          L.jobs.push_back({b.src, d + 1, b.size, zh_gz::stored_word(b.size), 4, 0});
        } else {
          L.jobs.push_back({d_scratch + b.out, d, size, 0, 0, 0});
        }
        d += size;
      }
      L.jobs.push_back({d_meta + m0 + zh_gz::kHeader, d,
                        (uint32_t)(zh_gz::kEnding + zh_gz::kTrailer), 0, 0, 0});
      d += zh_gz::kEnding + zh_gz::kTrailer;
      const size_t total = (size_t)(d - fbase);
      if (total > zh_gz::member_bound(n, P.B)) rc = ZH_EHIP;  // layout and bound disagree
      frames[i].dst_off = *pos + L.cpos;
      frames[i].cbytes = (int64_t)total;
      frames[i].status = ZH_OK;
      L.cpos += up((int64_t)total, 16);
    }
  }
  double gather_ms = 0;
  rc = finish_slab(s, ring, mem, marks, 3, rc, L, dst, pos, &gather_ms);
  if (rc == ZH_OK) {
    part_ms[kMatch] += marks.ms(0, 1);
    part_ms[kCoder] += marks.ms(1, 2);
    part_ms[kGather] += gather_ms;
  }
  return rc;
}

// CRC-32 of every source of the batch into crcs[n] (host): one launch over all spans, the spans
// folded on the host.
int crc_frames(zh_ctx* ctx, hipStream_t s, Ring& ring, const zh_gzip_enc_frame* frames, int64_t n,
               uint32_t* crcs, double* kernel_ms) {
  std::vector<CrcJob> cj;
  for (int64_t i = 0; i < n; i++) {
    const uint64_t nbytes = (uint64_t)frames[i].nbytes;
    for (uint64_t o = 0; o < nbytes; o += kSpan)
      cj.push_back({(uint64_t)(uintptr_t)frames[i].src + o,
                    (uint32_t)std::min<uint64_t>(kSpan, nbytes - o), 0});
  }
  if (cj.size() > (size_t)zh::kIntMax) return ZH_EINVAL;
  std::vector<uint32_t> raw(cj.size(), 0);
  int rc = ZH_OK;
  if (!cj.empty()) {
    void* dmem = nullptr;
    size_t got = 0;
    const size_t o_out = (size_t)up((int64_t)(cj.size() * sizeof(CrcJob)), 256);
    if (zh::ctx_alloc(ctx, o_out + cj.size() * 4, &dmem, &got) != hipSuccess) {
      (void)hipGetLastError();
      return ZH_ENOMEM;
    }
    uint8_t* d8 = (uint8_t*)dmem;
    if (!ring.h2d(d8, (const uint8_t*)cj.data(), cj.size() * sizeof(CrcJob))) rc = ZH_EHIP;
    Marks marks(s, 2);
    if (rc == ZH_OK) {
      marks.mark(0);
      hipLaunchKernelGGL(gzip_crc32_kernel, dim3((unsigned)cj.size()), dim3(kThreads), 0, s,
                         (const CrcJob*)d8, zh_gz::xpow8(kPiece), (uint32_t*)(d8 + o_out));
      if (hipGetLastError() != hipSuccess) rc = ZH_EHIP;
      marks.mark(1);
    }
    if (rc == ZH_OK && !ring.d2h((uint8_t*)raw.data(), d8 + o_out, cj.size() * 4)) rc = ZH_EHIP;
    if (hipStreamSynchronize(s) != hipSuccess) rc = rc == ZH_OK ? ZH_EHIP : rc;
    if (rc == ZH_OK) *kernel_ms += marks.ms(0, 1);
    zh::ctx_release(ctx, dmem, got);
    if (rc != ZH_OK) return rc;
  }
  const uint32_t x_span = zh_gz::xpow8(kSpan);
  size_t j = 0;
  for (int64_t i = 0; i < n; i++) {
    const uint64_t nbytes = (uint64_t)frames[i].nbytes;
    uint32_t r = 0;
    for (uint64_t o = 0; o < nbytes; o += kSpan, j++)
      r = zh_gz::crc_append(r, raw[j], cj[j].len == kSpan ? x_span : zh_gz::xpow8(cj[j].len));
    crcs[i] = zh_gz::crc_finish(r, nbytes);
  }
  return ZH_OK;
}

bool sources_ok(const zh_gzip_enc_frame* frames, int64_t n) {
  if (n < 0 || (n > 0 && !frames)) return false;
  for (int64_t i = 0; i < n; i++)
    if (frames[i].nbytes < 0 || (frames[i].nbytes > 0 && !frames[i].src)) return false;
  return true;
}

int64_t bound_of(const zh_gzip_enc_frame* frames, int64_t n, const zh_gzip_enc_params* prm) {
  zh_gz::Params P;
  if (!sources_ok(frames, n) || !zh_gz::read_params(prm, &P)) return -(int64_t)ZH_EINVAL;
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++)
    total += up((int64_t)zh_gz::member_bound((size_t)frames[i].nbytes, P.B), 16);
  return total;
}

}  // namespace

int zh::gzip_crc_launch(hipStream_t s, const void* d_jobs, uint32_t n, uint32_t* d_raw) {
  static_assert(sizeof(::CrcJob) == 16, "the layout zh_ctx.h describes");
  if (n == 0) return ZH_OK;
  hipLaunchKernelGGL(gzip_crc32_kernel, dim3(n), dim3(kThreads), 0, s, (const ::CrcJob*)d_jobs,
                     zh_gz::xpow8(kPiece), d_raw);
  return hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
}

int zh::gzip_segments_launch(hipStream_t s, const void* d_rows, uint32_t n, bool dynamic,
                             uint8_t* d_scratch, uint16_t* d_seqs, uint32_t* d_info,
                             uint32_t* d_csize) {
  static_assert(sizeof(::EncRow) == 32, "the layout zh_ctx.h describes");
  if (n == 0) return ZH_OK;
  zh_gz::Params P;
  P.dynamic = dynamic;
  launch_match(P.B, s, (const ::EncRow*)d_rows, n, d_seqs, d_info);
  launch_deflate(P, s, (const ::EncRow*)d_rows, n, d_scratch, d_seqs, d_info, d_csize);
  return hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
}

extern "C" {

int64_t zh_gzip_encode_bound(const zh_gzip_enc_frame* frames, int64_t n,
                             const zh_gzip_enc_params* params) {
  return bound_of(frames, n, params);
}

double zh_debug_gzip_encode_kernel_ms(void) { return g_last_genc_ms.load(); }

void zh_debug_gzip_encode_kernel_parts_ms(double out[4]) {
  for (int k = 0; k < 4; k++) out[k] = g_last_genc_part[k].load();
}

int zh_gzip_encode_batch(zh_ctx* ctx, zh_gzip_enc_frame* frames, int64_t n,
                         const zh_gzip_enc_params* params, void* dst, int64_t dstcap,
                         void* stream_v, char* err, size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  const int64_t bound = bound_of(frames, n, params);
  if (bound < 0) {
    for (int64_t i = 0; i < n && frames; i++) frames[i].status = ZH_EINVAL;
    put_err(err, errlen, zh_gz::bad_dynamic(params) ? "gzip encode: dynamic is 0 or 1"
                                                    : "gzip encode: blocksize >= 0, sizes >= 0");
    return ZH_EINVAL;
  }
  if (bound > dstcap || (bound > 0 && !dst)) {
    put_err(err, errlen, "zh_gzip_encode_batch: destination smaller than zh_gzip_encode_bound");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  zh_gz::Params P;
  (void)zh_gz::read_params(params, &P);
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;
  Ring ring;
  int rc = ring.init(ctx, s);
  int64_t pos = 0;
  double part[4] = {0, 0, 0, 0};
  std::vector<uint32_t> crcs;
  if (rc == ZH_OK && n > zh::kIntMax) rc = ZH_EINVAL;
  if (rc == ZH_OK) {
    crcs.assign((size_t)n, 0);
    rc = crc_frames(ctx, s, ring, frames, n, crcs.data(), &part[kCrc]);
  }
  for (int64_t f0 = 0; f0 < n && rc == ZH_OK;) {
    const int64_t f1 = slab_end(frames, f0, n);
    rc = encode_slab(ctx, s, ring, crcs.data(), frames, f0, f1, P, (uint8_t*)dst, &pos, part);
    f0 = f1;
  }
  if (rc != ZH_OK) {
    (void)hipGetLastError();
    put_err(err, errlen, rc == ZH_ENOMEM   ? "zh_gzip_encode_batch: out of device memory"
                         : rc == ZH_EINVAL ? "zh_gzip_encode_batch: too many blocks in a slab"
                                           : "zh_gzip_encode_batch: device copy or launch failed");
    return rc;
  }
  for (int k = 0; k < 4; k++) g_last_genc_part[k].store(part[k]);
  g_last_genc_ms.store(part[0] + part[1] + part[2] + part[3]);
  return ZH_OK;
}

int zh_debug_gzip_crc32(zh_ctx* ctx, const zh_gzip_enc_frame* frames, int64_t n, uint32_t* out) {
  if (!ctx || n > zh::kIntMax || !sources_ok(frames, n) || (n > 0 && !out)) return ZH_EINVAL;
  if (n == 0) return ZH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  Ring ring;
  const int rc = ring.init(ctx, ctx->stream);
  if (rc != ZH_OK) return rc;
  double ms = 0;
  return crc_frames(ctx, ctx->stream, ring, frames, n, out, &ms);
}

int zh_debug_gzip_code_lengths(zh_ctx* ctx, const uint32_t* counts, int32_t nsym, int32_t limit,
                               int64_t rows, uint8_t* lens) {
  if (nsym < 1 || nsym > (int32_t)zh_gz::kLitLen || limit < 1 || limit > 15 || rows < 0 ||
      rows > ((int64_t)1 << 20) || (rows > 0 && (!counts || !lens)))
    return ZH_EINVAL;
  if (rows == 0) return ZH_OK;
  const size_t total = (size_t)rows * (size_t)nsym;
  int rc = ZH_OK;
  if (!ctx) {
    zh_gz::DynWork* d = new (std::nothrow) zh_gz::DynWork;
    if (!d) return ZH_ENOMEM;
    zh_gz::OneLane w;
    for (int64_t r = 0; r < rows; r++) {
      uint8_t* out = lens + (size_t)r * (size_t)nsym;
      if (!zh_gz::code_lengths(counts + (size_t)r * (size_t)nsym, (uint32_t)nsym, (uint32_t)limit,
                               d->lens, *d, w)) {
        rc = ZH_EINVAL;
        memset(out, 255, (size_t)nsym);
      } else {
        memcpy(out, d->lens, (size_t)nsym);
      }
    }
    delete d;
    return rc;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  Ring ring;
  rc = ring.init(ctx, ctx->stream);
  if (rc != ZH_OK) return rc;
  const size_t o_lens = (size_t)up((int64_t)(total * 4), 256);
  void* dmem = nullptr;
  size_t got = 0;
  if (zh::ctx_alloc(ctx, o_lens + total, &dmem, &got) != hipSuccess) {
    (void)hipGetLastError();
    return ZH_ENOMEM;
  }
  uint8_t* d8 = (uint8_t*)dmem;
  if (!ring.h2d(d8, (const uint8_t*)counts, total * 4)) rc = ZH_EHIP;
  if (rc == ZH_OK) {
    hipLaunchKernelGGL(gzip_code_lengths_kernel, dim3((unsigned)rows), dim3(64), 0, ctx->stream,
                       (const uint32_t*)d8, (uint32_t)nsym, (uint32_t)limit, d8 + o_lens);
    if (hipGetLastError() != hipSuccess) rc = ZH_EHIP;
  }
  if (rc == ZH_OK && !ring.d2h(lens, d8 + o_lens, total)) rc = ZH_EHIP;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = rc == ZH_OK ? ZH_EHIP : rc;
  zh::ctx_release(ctx, dmem, got);
  for (size_t i = 0; rc == ZH_OK && i < total; i++)
    if (lens[i] == 255) rc = ZH_EINVAL;
  return rc;
}

}  // extern "C"
