// zh_zstd_enc_kernels.hip — zstd frames written on the device, a batch at a time
// (zh_zstd_encode_bound / zh_zstd_encode_batch); the frame and the block encoder are
// zh_zstd_enc.h, the host form zh_zstd_compress (zh_zstd.cpp) is the byte-for-byte oracle.
//
// The raw bytes are in device memory (zh_array_write's chunk buffers); the frames go to the host.
//   zstd_match_kernel<CAP, WAVES>   one wave per block of at most CAP bytes (16, 32 or 64 KiB by
//           the batch's block size), WAVES blocks per workgroup.  The wave loads its block into
//           its part of LDS, next to its hash table (kHashSize slots), and runs
//           zh_ze::match_block over WaveLanes: literals go to the block's region of the scratch
//           buffer (behind the 3 bytes of the literals header), sequence records to the block's
//           part of the list, both in global memory, neither read again in this kernel.  The
//           kernel has no barrier: between steps a wave waits for its own LDS operations only.
//   zstd_fse_kernel (zh_enc_device.h)   one thread per block: zh_ze::fse_block walks the records
//           backwards and writes the sequences section behind the literals; the size of the
//           compressed block (or the raw size: store it raw) goes to a table.  The records and
//           literals were written by the kernel before: the kernel boundary orders them.
//   zstd_xxh64_kernel   one wave per frame, one launch for the whole batch ahead of its slabs
//           (a frame's hash is a serial chain: the more frames at once, the better): the lanes
//           load 16 stripes of 32 bytes at a time and multiply their word by P2, the four
//           accumulators live in the lanes l & 3 and take their words by lane shuffle, stripe
//           after stripe; merge and tail as zh_xxh64.
//   host    one small copy brings the size table back; zh_ze::walk_blocks merges raw runs, a
//           prefix sum lays the frames out and builds one copy job per piece;
//   blosc_gather_kernel (zh_enc_device.h)   one workgroup per job: the 3 bytes of a block header,
//           then the bytes, from the scratch (compressed blocks), from the raw source (raw
//           blocks), from the uploaded frame headers or from the hash table (checksums);
//   D2H     the compact buffer through the context's page-locked out ring into host memory.
// encode_slab keeps the planning and the layout, which are this format; the slab's memory, marks,
// cutting and tail (caps, upload, gather, download, synchronise) are the driver of zh_enc_device.h.
// Slabs of at most kSlabBytes of raw input bound the device memory: per slab the scratch (the raw
// size), the records (6 bytes per 4 raw bytes: 1.5 x), the compact frames (the raw size and the
// headers) and the small tables.
// Every job and block row is built on the host from validated sizes; the size table is checked
// against the block sizes before it lays anything out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "zh_ctx.h"
#include "zh_enc_device.h"
#include "zh_zstd_enc.h"

namespace {

struct HashJob {
  uint64_t src, n;
};

template <uint32_t CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void zstd_match_kernel(
    const EncRow* __restrict__ blocks, uint32_t nblocks, uint8_t* __restrict__ scratch,
    uint16_t* __restrict__ seqs, uint32_t* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[WAVES][CAP];
  __shared__ uint32_t tables[WAVES][zh_lz::kHashSize];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * WAVES + wave;
  if (k >= nblocks) return;  // the whole wave: the kernel has no barrier
  const EncRow b = blocks[k];
  if (b.size > CAP) return;  // never: the host picks CAP from the block size
  const uint8_t* __restrict__ src = (const uint8_t*)b.src;
  uint8_t* blk = lds[wave];
  const uint32_t al = (uint32_t)(((uintptr_t)src) & 15);
  for (uint32_t q0 = lane * 16; q0 < b.size; q0 += 64 * 16) {
    const uint32_t cnt = b.size - q0 < 16u ? b.size - q0 : 16u;
    if (cnt == 16 && al == 0) {
      *(uint4*)(blk + q0) = *(const uint4*)(src + q0);
    } else if (cnt == 16 && (al & 3) == 0) {  // inner chunks behind a shard's index
      const uint32_t* s4 = (const uint32_t*)(src + q0);
      *(uint4*)(blk + q0) = make_uint4(s4[0], s4[1], s4[2], s4[3]);
    } else {
      for (uint32_t i = 0; i < cnt; i++) blk[q0 + i] = src[q0 + i];
    }
  }
  WaveLanes::order();
  WaveLanes w;
  w.lane = lane;
  w.h = 0;
  w.wide = true;
  uint32_t nl = 0;
  const uint32_t ns = zh_ze::match_block(blk, b.size, scratch + b.out + 3, seqs + b.seq,
                                         tables[wave], w, &nl);
  if (lane == 0) {
    info[2 * k] = ns;
    info[2 * k + 1] = nl;
  }
}

// ---- XXH64, seed 0 ----------------------------------------------------------------------------
constexpr uint64_t XP1 = 11400714785074694791ull, XP2 = 14029467366897019727ull,
                   XP3 = 1609587929392839161ull, XP4 = 9650029242287828579ull,
                   XP5 = 2870177450012600261ull;
__device__ inline uint64_t xrotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ inline uint64_t xround(uint64_t acc, uint64_t in) {
  acc += in * XP2;
  acc = xrotl(acc, 31);
  return acc * XP1;
}
__device__ inline uint64_t xmerge(uint64_t acc, uint64_t v) {
  acc ^= xround(0, v);
  return acc * XP1 + XP4;
}
__device__ inline uint64_t xld(const uint8_t* p, int nbytes) {
  uint64_t v = 0;
  for (int i = 0; i < nbytes; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
// 8 bytes at p, whose alignment (of the frame, a multiple of 8 away) is al
__device__ inline uint64_t xld64(const uint8_t* p, uint32_t al) {
  if ((al & 7) == 0) return *(const uint64_t*)p;
  if ((al & 3) == 0) {
    const uint32_t* q = (const uint32_t*)p;
    return (uint64_t)q[0] | ((uint64_t)q[1] << 32);
  }
  return xld(p, 8);
}

__global__ __launch_bounds__(kThreads) void zstd_xxh64_kernel(const HashJob* __restrict__ jobs,
                                                              uint32_t njobs,
                                                              uint64_t* __restrict__ out) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * kWaves + wave;
  if (j >= njobs) return;
  const uint8_t* __restrict__ src = (const uint8_t*)jobs[j].src;
  const uint64_t n = jobs[j].n;
  const uint32_t al = (uint32_t)(((uintptr_t)src) & 7);
  const uint64_t nstripes = n / 32, nwords = nstripes * 4;
  const uint32_t a = lane & 3;
  uint64_t acc = a == 0 ? XP1 + XP2 : a == 1 ? XP2 : a == 2 ? 0 : 0 - XP1;
  auto load = [&](uint64_t tile) -> uint64_t {
    const uint64_t wd = tile * 64 + lane;
    return wd < nwords ? xld64(src + 8 * wd, al) : 0;
  };
  // in * P2 is off the serial chain: every lane multiplies its own word; a round is then
  // acc = rotl(acc + x, 31) * P1
  uint64_t cur = load(0) * XP2;
  for (uint64_t t = 0; t * 16 < nstripes; t++) {
    const uint64_t nxt = load(t + 1) * XP2;  // in flight while this tile's 16 rounds run
    const uint32_t cnt = nstripes - t * 16 < 16 ? (uint32_t)(nstripes - t * 16) : 16u;
    if (cnt == 16) {
#pragma unroll
      for (uint32_t s = 0; s < 16; s++) {
        const uint64_t x = (uint64_t)__shfl((unsigned long long)cur, (int)(4 * s + a));
        acc = xrotl(acc + x, 31) * XP1;
      }
    } else {
      for (uint32_t s = 0; s < cnt; s++) {
        const uint64_t x = (uint64_t)__shfl((unsigned long long)cur, (int)(4 * s + a));
        acc = xrotl(acc + x, 31) * XP1;
      }
    }
    cur = nxt;
  }
  const uint64_t v1 = (uint64_t)__shfl((unsigned long long)acc, 0),
                 v2 = (uint64_t)__shfl((unsigned long long)acc, 1),
                 v3 = (uint64_t)__shfl((unsigned long long)acc, 2),
                 v4 = (uint64_t)__shfl((unsigned long long)acc, 3);
  uint64_t h;
  if (n >= 32) {
    h = xrotl(v1, 1) + xrotl(v2, 7) + xrotl(v3, 12) + xrotl(v4, 18);
    h = xmerge(h, v1);
    h = xmerge(h, v2);
    h = xmerge(h, v3);
    h = xmerge(h, v4);
  } else {
    h = XP5;
  }
  h += n;
  const uint8_t* p = src + nstripes * 32;
  const uint8_t* end = src + n;
  while (p + 8 <= end) {
    h ^= xround(0, xld(p, 8));
    h = xrotl(h, 27) * XP1 + XP4;
    p += 8;
  }
  if (p + 4 <= end) {
    h ^= xld(p, 4) * XP1;
    h = xrotl(h, 23) * XP2 + XP3;
    p += 4;
  }
  while (p < end) {
    h ^= (uint64_t)(*p++) * XP5;
    h = xrotl(h, 11) * XP1;
  }
  h ^= h >> 33;
  h *= XP2;
  h ^= h >> 29;
  h *= XP3;
  h ^= h >> 32;
  if (lane == 0) out[j] = h;
}

std::atomic<double> g_last_zenc_ms{-1.0};

void launch_match(uint32_t B, hipStream_t s, const EncRow* blocks, uint32_t nblocks,
                  uint8_t* scratch, uint16_t* seqs, uint32_t* info) {
  if (B <= (16u << 10)) {
    hipLaunchKernelGGL((zstd_match_kernel<(16u << 10), 4>), dim3((nblocks + 3) / 4), dim3(256), 0,
                       s, blocks, nblocks, scratch, seqs, info);
  } else if (B <= (32u << 10)) {
    hipLaunchKernelGGL((zstd_match_kernel<(32u << 10), 4>), dim3((nblocks + 3) / 4), dim3(256), 0,
                       s, blocks, nblocks, scratch, seqs, info);
  } else {
    hipLaunchKernelGGL((zstd_match_kernel<zh_ze::kMaxBlock, 2>), dim3((nblocks + 1) / 2),
                       dim3(128), 0, s, blocks, nblocks, scratch, seqs, info);
  }
}

struct FramePlan {
  int64_t first_block = 0, nblocks = 0;  // within the slab
};

struct DevEmit {
  std::vector<GatherJob>* jobs;
  const EncRow* blocks;  // of this frame
  uint64_t src, scratch, dst;
  void raw(uint32_t h, size_t off, uint32_t len) {
    jobs->push_back({src + off, dst, len, h, 3, 0});
    dst += 3 + (uint64_t)len;
  }
  void comp(uint32_t h, size_t k, uint32_t len) {
    jobs->push_back({scratch + blocks[k].out, dst, len, h, 3, 0});
    dst += 3 + (uint64_t)len;
  }
};

// One slab [f0, f1) of the batch; *pos: the running offset in dst.
int encode_slab(zh_ctx* ctx, hipStream_t s, Ring& ring, const zh_ze::Tables* dtab,
                const uint64_t* d_hashes, zh_zstd_enc_frame* frames, int64_t f0, int64_t f1,
                const zh_ze::Params& P, uint8_t* dst, int64_t* pos, double* kernel_ms) {
  const int64_t nf = f1 - f0;
  std::vector<FramePlan> plan((size_t)nf);
  std::vector<EncRow> blocks;
  SlabLayout L;
  int64_t scratch_total = 0, seq_total = 0;
  for (int64_t i = f0; i < f1; i++) {
    FramePlan& fp = plan[(size_t)(i - f0)];
    const size_t n = (size_t)frames[i].nbytes;
    fp.first_block = (int64_t)blocks.size();
    fp.nblocks = (int64_t)zh_ze::block_count(n, P.B);
    for (int64_t k = 0; k < fp.nblocks; k++) {
      EncRow b;
      b.size = zh_ze::block_size(n, P.B, (size_t)k);
      b.src = (uint64_t)(uintptr_t)frames[i].src + (uint64_t)k * P.B;
      b.out = (uint64_t)scratch_total;
      b.seq = (uint64_t)seq_total;
      b.pad = 0;
      blocks.push_back(b);
      scratch_total += up(b.size, 16);
      seq_total += up(3 * (int64_t)(b.size / 4) + 3, 8);
    }
    L.compact_cap += up((int64_t)zh_ze::raw_frame_size(n, P.checksum), 16);
    L.njobs_cap += 4 + fp.nblocks + (int64_t)(n / zh_ze::kRawBlock);
  }
  if (blocks.size() > (size_t)zh::kIntMax || L.njobs_cap > zh::kIntMax) return ZH_EINVAL;
  const size_t nb = blocks.size();
  L.meta_cap = nf * 16;

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
  Marks marks(s, 4);
  std::vector<uint32_t> cs(nb, 0);
  if (nb && !ring.h2d(mem.at(o_blocks), (const uint8_t*)blocks.data(), nb * sizeof(EncRow)))
    rc = ZH_EHIP;
  if (rc == ZH_OK) {
    marks.mark(0);
    if (nb) {
      launch_match(P.B, s, (const EncRow*)mem.at(o_blocks), (uint32_t)nb, mem.at(o_scratch),
                   (uint16_t*)mem.at(o_seq), (uint32_t*)mem.at(o_info));
      hipLaunchKernelGGL(zstd_fse_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, s,
                         (const EncRow*)mem.at(o_blocks), (uint32_t)nb, dtab, mem.at(o_scratch),
                         (const uint16_t*)mem.at(o_seq), (const uint32_t*)mem.at(o_info),
                         (uint32_t*)mem.at(o_cs));
    }
    if (hipGetLastError() != hipSuccess) rc = ZH_EHIP;
    marks.mark(1);
  }
  if (rc == ZH_OK && nb && !ring.d2h((uint8_t*)cs.data(), mem.at(o_cs), nb * 4)) rc = ZH_EHIP;
  // the table lays out device copies: nothing in it may pass its block's raw size
  for (size_t k = 0; k < nb && rc == ZH_OK; k++)
    if (cs[k] == 0 || cs[k] > blocks[k].size) rc = ZH_EHIP;

  // layout: the frames side by side in the compact buffer, each 16-byte aligned
  if (rc == ZH_OK) {
    L.meta.resize((size_t)nf * 16, 0);
    L.jobs.reserve((size_t)L.njobs_cap);
    const uint64_t d_meta = mem.addr(L.o_meta), d_scratch = mem.addr(o_scratch);
    const uint64_t d_compact = mem.addr(L.o_compact);
    const uint64_t d_hash = (uint64_t)(uintptr_t)d_hashes;
    for (int64_t i = f0; i < f1; i++) {
      const FramePlan& fp = plan[(size_t)(i - f0)];
      const size_t n = (size_t)frames[i].nbytes;
      bool all_raw;
      const uint32_t* fcs = fp.nblocks ? cs.data() + fp.first_block : nullptr;
      const size_t total = zh_ze::frame_size(n, P.B, fcs, P.checksum, &all_raw);
      const size_t m0 = (size_t)(i - f0) * 16;
      zh_ze::put_frame_header(L.meta.data() + m0, n, P.checksum);
      const uint64_t fbase = d_compact + (uint64_t)L.cpos;
      L.jobs.push_back({d_meta + m0, fbase, (uint32_t)zh_ze::kFrameHeader, 0, 0, 0});
      DevEmit e{&L.jobs, blocks.data() + fp.first_block, (uint64_t)(uintptr_t)frames[i].src,
                d_scratch, fbase + zh_ze::kFrameHeader};
      zh_ze::walk_blocks(n, P.B, cs.data() + fp.first_block, all_raw, e);
      if (P.checksum) {
        L.jobs.push_back({d_hash + 8 * (uint64_t)i, e.dst, 4, 0, 0, 0});
        e.dst += 4;
      }
      if (e.dst - fbase != total) rc = ZH_EHIP;  // layout and size disagree
      frames[i].dst_off = *pos + L.cpos;
      frames[i].cbytes = (int64_t)total;
      frames[i].status = ZH_OK;
      L.cpos += up((int64_t)total, 16);
    }
  }
  double gather_ms = 0;
  rc = finish_slab(s, ring, mem, marks, 2, rc, L, dst, pos, &gather_ms);
  if (rc == ZH_OK) *kernel_ms += marks.ms(0, 1) + gather_ms;
  return rc;
}

// XXH64 of every frame of the batch into hashes[n] (device), one launch.
int hash_frames(hipStream_t s, Ring& ring, const zh_zstd_enc_frame* frames, int64_t n,
                uint8_t* d_jobs, uint64_t* d_hashes, double* kernel_ms) {
  std::vector<HashJob> hj((size_t)n);
  for (int64_t i = 0; i < n; i++)
    hj[(size_t)i] = {(uint64_t)(uintptr_t)frames[i].src, (uint64_t)frames[i].nbytes};
  if (!ring.h2d(d_jobs, (const uint8_t*)hj.data(), hj.size() * sizeof(HashJob))) return ZH_EHIP;
  Marks marks(s, 2);
  marks.mark(0);
  hipLaunchKernelGGL(zstd_xxh64_kernel, dim3((unsigned)((n + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, s, (const HashJob*)d_jobs, (uint32_t)n, d_hashes);
  int rc = hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
  marks.mark(1);
  if (hipStreamSynchronize(s) != hipSuccess) rc = ZH_EHIP;
  if (rc == ZH_OK) *kernel_ms += marks.ms(0, 1);
  return rc;
}

int64_t bound_of(const zh_zstd_enc_frame* frames, int64_t n, const zh_zstd_enc_params* prm) {
  zh_ze::Params P;
  if (n < 0 || (n > 0 && !frames) || !zh_ze::read_params(prm, &P)) return -(int64_t)ZH_EINVAL;
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (frames[i].nbytes < 0 || (frames[i].nbytes > 0 && !frames[i].src))
      return -(int64_t)ZH_EINVAL;
    total += up((int64_t)zh_ze::raw_frame_size((size_t)frames[i].nbytes, P.checksum), 16);
  }
  return total;
}

}  // namespace

// The hash kernel for the decode batch (zh_zstd_dec_kernels.hip), which verifies checksums.
int zh::zstd_hash_launch(hipStream_t s, const void* d_jobs, uint32_t n, uint64_t* d_hashes) {
  static_assert(sizeof(HashJob) == 16, "the decode batch builds these rows");
  if (n == 0) return ZH_OK;
  hipLaunchKernelGGL(zstd_xxh64_kernel, dim3((n + kWaves - 1) / kWaves), dim3(kThreads), 0, s,
                     (const HashJob*)d_jobs, n, d_hashes);
  return hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
}

extern "C" {

int64_t zh_zstd_encode_bound(const zh_zstd_enc_frame* frames, int64_t n,
                             const zh_zstd_enc_params* params) {
  return bound_of(frames, n, params);
}

double zh_debug_zstd_encode_kernel_ms(void) { return g_last_zenc_ms.load(); }

int zh_zstd_encode_batch(zh_ctx* ctx, zh_zstd_enc_frame* frames, int64_t n,
                         const zh_zstd_enc_params* params, void* dst, int64_t dstcap,
                         void* stream_v, char* err, size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  const int64_t bound = bound_of(frames, n, params);
  if (bound < 0) {
    for (int64_t i = 0; i < n && frames; i++) frames[i].status = ZH_EINVAL;
    put_err(err, errlen, "zstd encode: checksum 0 or 1, blocksize >= 0, sizes >= 0");
    return ZH_EINVAL;
  }
  if (bound > dstcap || (bound > 0 && !dst)) {
    put_err(err, errlen, "zh_zstd_encode_batch: destination smaller than zh_zstd_encode_bound");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  zh_ze::Params P;
  (void)zh_ze::read_params(params, &P);
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;
  const zh_ze::Tables* dtab = device_tables(ctx);
  Ring ring;
  int rc = dtab ? ring.init(ctx, s) : ZH_ENOMEM;
  int64_t pos = 0;
  double ms = 0;
  void* hmem = nullptr;  // [hash jobs | hashes] of the whole batch
  size_t hgot = 0;
  const size_t o_hashes = (size_t)up(n * (int64_t)sizeof(HashJob), 256);
  if (rc == ZH_OK && n > zh::kIntMax) rc = ZH_EINVAL;
  if (rc == ZH_OK && P.checksum) {
    if (zh::ctx_alloc(ctx, o_hashes + (size_t)n * 8, &hmem, &hgot) != hipSuccess) {
      (void)hipGetLastError();
      rc = ZH_ENOMEM;
    } else {
      rc = hash_frames(s, ring, frames, n, (uint8_t*)hmem, (uint64_t*)((uint8_t*)hmem + o_hashes),
                       &ms);
    }
  }
  const uint64_t* d_hashes = hmem ? (const uint64_t*)((uint8_t*)hmem + o_hashes) : nullptr;
  for (int64_t f0 = 0; f0 < n && rc == ZH_OK;) {
    const int64_t f1 = slab_end(frames, f0, n);
    rc = encode_slab(ctx, s, ring, dtab, d_hashes, frames, f0, f1, P, (uint8_t*)dst, &pos, &ms);
    f0 = f1;
  }
  if (hmem) zh::ctx_release(ctx, hmem, hgot);
  if (rc != ZH_OK) {
    (void)hipGetLastError();
    put_err(err, errlen, rc == ZH_ENOMEM ? "zh_zstd_encode_batch: out of device memory"
                                         : "zh_zstd_encode_batch: device copy or launch failed");
    return rc;
  }
  g_last_zenc_ms.store(ms);
  return ZH_OK;
}

int zh_debug_zstd_xxh64(zh_ctx* ctx, const zh_zstd_enc_frame* frames, int64_t n, uint64_t* out) {
  if (!ctx || n < 0 || n > zh::kIntMax || (n > 0 && (!frames || !out))) return ZH_EINVAL;
  for (int64_t i = 0; i < n; i++)
    if (frames[i].nbytes < 0 || (frames[i].nbytes > 0 && !frames[i].src)) return ZH_EINVAL;
  if (n == 0) return ZH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  Ring ring;
  int rc = ring.init(ctx, ctx->stream);
  if (rc != ZH_OK) return rc;
  void* hmem = nullptr;
  size_t hgot = 0;
  const size_t o_hashes = (size_t)up(n * (int64_t)sizeof(HashJob), 256);
  if (zh::ctx_alloc(ctx, o_hashes + (size_t)n * 8, &hmem, &hgot) != hipSuccess) {
    (void)hipGetLastError();
    return ZH_ENOMEM;
  }
  uint8_t* d8 = (uint8_t*)hmem;
  double ms = 0;
  rc = hash_frames(ctx->stream, ring, frames, n, d8, (uint64_t*)(d8 + o_hashes), &ms);
  if (rc == ZH_OK && !ring.d2h((uint8_t*)out, d8 + o_hashes, (size_t)n * 8)) rc = ZH_EHIP;
  zh::ctx_release(ctx, hmem, hgot);
  return rc;
}

}  // extern "C"
