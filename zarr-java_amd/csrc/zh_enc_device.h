// zh_enc_device.h — what the device frame writers share (zh_blosc_enc_kernels.hip,
// zh_zstd_enc_kernels.hip, zh_gzip_enc_kernels.hip).  Device code: the wave form of the lane
// policy of zh_lz_match.h, the EncRow row of the block kernels, the second phase of the zstd
// block writer (zstd_fse_kernel, with the encoding tables in device memory) and the gather kernel
// that lays finished pieces out as compact frames.  Host code, the one driver of a slab: the
// copies through the context's page-locked rings (Ring), the slab's device memory (SlabMem), its
// timing marks (Marks), the cutter of a batch into slabs (slab_end) and the tail every writer
// ends a slab with (finish_slab: caps, upload, gather, download, synchronise).  A writer keeps
// what is its format: the plan of its rows, its launch, the check of the sizes that come back
// and the layout of its jobs.  Included by .hip files only, each of which gets its own copy
// (anonymous namespace).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "zh_ctx.h"
#include "zh_lz_match.h"
#include "zh_zstd_enc.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;

// One copy of the gather kernel: an optional word of 1..4 bytes (a blosc csize, a zstd block
// header), then n bytes.
struct GatherJob {
  uint64_t src, dst;  // device addresses
  uint32_t n, word, wbytes, pad;  // wbytes (0..4) low bytes of word go before the n bytes
};


// The lane policy of zh_lz_match.h for one wave.
struct WaveLanes {
  uint32_t lane, h;
  bool wide = false;  // as HostLanes::wide

  // Between two steps only the table in LDS is read by other lanes than wrote it: the wave
  // waits for its LDS operations, never for its stores to the scratch (nothing reads those back).
  __device__ static void order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  // Before the raw copy overwrites what the abandoned encoding stored in the same region.
  __device__ static void drain_stores() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __device__ void clear(uint32_t* table) {
    for (uint32_t i = lane; i < zh_lz::kHashSize; i += 64) table[i] = 0;
    order();
  }
  __device__ uint32_t find(const uint8_t* s, uint32_t p, uint32_t lim, const uint32_t* table,
                           uint32_t* ref) {
    const uint32_t q = p + lane;
    uint32_t c = 0;
    bool ok = false;
    if (q <= lim) {
      const uint32_t v = zh_lz::ld32(s + q);
      h = zh_lz::hash4(v);
      c = table[h];
      ok = c != 0 && zh_lz::ld32(s + c - 1) == v;
      if (!ok && q >= 1 && zh_lz::ld32(s + q - 1) == v) ok = true, c = q;  // a run
      if (wide) {
        for (uint32_t d = 2; d <= 8; d *= 2)
          if (!ok && q >= d && zh_lz::ld32(s + q - d) == v) ok = true, c = q - d + 1;
      }
    }
    const unsigned long long b = __ballot(ok);
    if (!b) return 64;
    const int first = __builtin_ctzll(b);
    *ref = (uint32_t)__builtin_amdgcn_readlane((int)c, first) - 1;
    return (uint32_t)first;
  }
  __device__ void insert(uint32_t p, uint32_t end, uint32_t* table) {
    if (p + lane < end) atomicMax(&table[h], p + lane + 1);
    order();
  }
  __device__ uint32_t extend(const uint8_t* s, uint32_t a, uint32_t b, uint32_t maxn) {
    for (uint32_t k0 = 0; k0 < maxn; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool differ = k >= maxn || s[a + k] != s[b + k];
      const unsigned long long m = __ballot(differ);
      if (m) return k0 + (uint32_t)__builtin_ctzll(m);
    }
    return maxn;
  }
  __device__ void copy(uint8_t* d, const uint8_t* s, uint32_t n) {
    for (uint32_t k = lane; k < n; k += 64) d[k] = s[k];
  }
  __device__ void lenbytes(uint8_t* d, uint32_t v) {
    const uint32_t nfull = v / 255;
    for (uint32_t k = lane; k <= nfull; k += 64) d[k] = k < nfull ? 255 : (uint8_t)(v % 255);
  }
  __device__ void put(uint8_t* d, uint32_t b) {
    if (lane == 0) *d = (uint8_t)b;
  }
  __device__ void put16(uint16_t* d, uint32_t v) {
    if (lane == 0) *d = (uint16_t)v;
  }
};

__global__ __launch_bounds__(kThreads) void blosc_gather_kernel(
    const GatherJob* __restrict__ jobs) {
  const GatherJob j = jobs[blockIdx.x];
  const uint8_t* s = (const uint8_t*)j.src;
  uint8_t* d = (uint8_t*)j.dst;
  const uint32_t t = threadIdx.x;
  if (j.wbytes) {
    if (t < j.wbytes) d[t] = (uint8_t)(j.word >> (8 * t));
    d += j.wbytes;
  }
  uint32_t n = j.n;
  uint32_t head = (uint32_t)((16 - (((uintptr_t)d) & 15)) & 15);
  if (head > n) head = n;
  if (t < head) d[t] = s[t];
  s += head, d += head, n -= head;
  const uint32_t nv = n / 16;
  const uint32_t sh = (uint32_t)(((uintptr_t)s) & 3);
  if ((((uintptr_t)s) & 15) == 0) {
    for (uint32_t i = t; i < nv; i += kThreads) ((uint4*)d)[i] = ((const uint4*)s)[i];
  } else {
    // the source is not aligned with the destination: aligned words, shifted into place.  The
    // fifth word holds at least one byte of the range when sh != 0, and is not read otherwise.
    const uint32_t* s4 = (const uint32_t*)(s - sh);
    for (uint32_t i = t; i < nv; i += kThreads) {
      uint32_t x[5];
      for (int k = 0; k < 4; k++) x[k] = s4[4 * i + k];
      x[4] = sh ? s4[4 * i + 4] : 0u;
      uint32_t y[4];
      for (int k = 0; k < 4; k++) y[k] = sh ? __builtin_amdgcn_alignbyte(x[k + 1], x[k], sh) : x[k];
      ((uint4*)d)[i] = make_uint4(y[0], y[1], y[2], y[3]);
    }
  }
  for (uint32_t q = nv * 16 + t; q < n; q += kThreads) d[q] = s[q];
}

// One row of the block kernels.  The zstd block writer (zh_zstd_enc.h): a block of a zstd frame,
// or a stream of a blosc frame whose streams are zstd frames (src unused).  The gzip segment
// writer (zh_gzip_enc.h): a block of a gzip member, or a 16 KiB piece of a stream of a blosc
// frame whose streams are zlib streams.
struct EncRow {
  uint64_t src;  // device address of the raw block
  uint64_t out;  // offset of the block's region in the scratch buffer
  uint64_t seq;  // offset of the block's records in the list, in uint16
  uint32_t size, pad;
};
static_assert(sizeof(EncRow) == 32, "the layout zh_ctx.h describes");

// One thread per block: zh_ze::fse_block walks the block's records backwards and writes the
// sequences section behind the literals; the size of the compressed block (or the raw size:
// store it raw) goes to a table.  The records and literals were written by the kernel before:
// the kernel boundary orders them.  (The gzip writer includes this header and does not launch it.)
[[maybe_unused]] __global__ __launch_bounds__(64) void zstd_fse_kernel(
    const EncRow* __restrict__ blocks, uint32_t nblocks, const zh_ze::Tables* __restrict__ tg,
    uint8_t* __restrict__ scratch, const uint16_t* __restrict__ seqs,
    const uint32_t* __restrict__ info, uint32_t* __restrict__ csize) {
  __shared__ zh_ze::Tables T;
  for (uint32_t i = threadIdx.x; i < sizeof(zh_ze::Tables) / 4; i += 64)
    ((uint32_t*)&T)[i] = ((const uint32_t*)tg)[i];
  __syncthreads();
  const uint32_t k = blockIdx.x * 64 + threadIdx.x;
  if (k >= nblocks) return;
  const EncRow b = blocks[k];
  csize[k] = zh_ze::fse_block(T, seqs + b.seq, info[2 * k], info[2 * k + 1], scratch + b.out,
                              b.size);
}
static_assert(sizeof(zh_ze::Tables) % 4 == 0, "the tables are copied as words");

// The encoding tables in device memory, uploaded once per context (under ctx->mu).
inline const zh_ze::Tables* device_tables(zh_ctx* ctx) {
  if (!ctx->zstd_tables) {
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(zh_ze::Tables)) != hipSuccess) return nullptr;
    if (hipMemcpy(p, &zh_ze::tables(), sizeof(zh_ze::Tables), hipMemcpyHostToDevice) !=
        hipSuccess) {
      (void)hipFree(p);
      return nullptr;
    }
    ctx->zstd_tables = p;
  }
  return (const zh_ze::Tables*)ctx->zstd_tables;
}

void put_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) {
    strncpy(err, msg, errlen - 1);
    err[errlen - 1] = 0;
  }
}

inline int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// Through the context's page-locked rings, one slot at a time in flight per ring slot.
struct Ring {
  zh_ctx* ctx;
  hipStream_t s;
  size_t slot_bytes = 0;
  std::vector<hipEvent_t> ev;

  int init(zh_ctx* c, hipStream_t st) {
    ctx = c, s = st;
    int lanes;
    int64_t window;
    const int rc = zh::pipe_out_ring(ctx, &lanes, &window);
    if (rc != ZH_OK) return rc;
    slot_bytes = (size_t)window;
    ev.assign(ctx->ring_out.size(), nullptr);
    for (auto& e : ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ZH_EHIP;
    return ev.empty() || slot_bytes == 0 ? ZH_EHIP : ZH_OK;
  }
  ~Ring() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  // device -> host memory, the copies pipelined over the out ring's slots; returns when done
  bool d2h(uint8_t* h, const uint8_t* d, size_t n) {
    const size_t nslots = ev.size(), nchunks = (n + slot_bytes - 1) / slot_bytes;
    auto land = [&](size_t i) {
      if (hipEventSynchronize(ev[i % nslots]) != hipSuccess) return false;
      const size_t off = i * slot_bytes;
      memcpy(h + off, ctx->ring_out[i % nslots], std::min(slot_bytes, n - off));
      return true;
    };
    for (size_t i = 0; i < nchunks; i++) {
      if (i >= nslots && !land(i - nslots)) return false;
      const size_t off = i * slot_bytes;
      if (hipMemcpyAsync(ctx->ring_out[i % nslots], d + off, std::min(slot_bytes, n - off),
                         hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipEventRecord(ev[i % nslots], s) != hipSuccess)
        return false;
    }
    for (size_t i = nchunks > nslots ? nchunks - nslots : 0; i < nchunks; i++)
      if (!land(i)) return false;
    return true;
  }
  // host tables -> device through the in ring (small: one slot, reused)
  bool h2d(uint8_t* d, const uint8_t* h, size_t n) {
    for (size_t off = 0; off < n; off += slot_bytes) {
      const size_t take = std::min(slot_bytes, n - off);
      memcpy(ctx->ring_in[0], h + off, take);
      if (hipMemcpyAsync(d + off, ctx->ring_in[0], take, hipMemcpyHostToDevice, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess)
        return false;
    }
    return true;
  }
};

// Slabs of at most kSlabBytes of raw input bound a batch's device memory.  The end of the slab
// that begins at frame f0: a larger frame is a slab of its own, the next frame joins only while
// the raw size stays within the limit.
constexpr int64_t kSlabBytes = (int64_t)128 << 20;
template <class Frame>
int64_t slab_end(const Frame* frames, int64_t f0, int64_t n) {
  int64_t f1 = f0, raw = 0;
  do raw += frames[f1++].nbytes;
  while (f1 < n && raw + frames[f1].nbytes <= kSlabBytes);
  return f1;
}

// The device memory of one slab: sections of one zh::ctx_alloc block, each 256-byte aligned, with
// 256 bytes of slack behind the last; released when the slab ends.
struct SlabMem {
  zh_ctx* ctx = nullptr;
  uint8_t* d8 = nullptr;
  size_t got = 0, next = 0, end = 0;

  size_t add(int64_t bytes) {  // the section's offset
    const size_t o = next;
    end = o + (size_t)bytes;
    next = o + (size_t)up(bytes, 256);
    return o;
  }
  int alloc(zh_ctx* c) {
    void* p = nullptr;
    if (zh::ctx_alloc(c, end + 256, &p, &got) != hipSuccess) {
      (void)hipGetLastError();
      return ZH_ENOMEM;
    }
    ctx = c, d8 = (uint8_t*)p;
    return ZH_OK;
  }
  ~SlabMem() {
    if (d8) zh::ctx_release(ctx, d8, got);
  }
  uint8_t* at(size_t o) const { return d8 + o; }
  uint64_t addr(size_t o) const { return (uint64_t)(uintptr_t)(d8 + o); }
};

// The timing marks of one slab: n events on the stream, or none that count if one is missing.
struct Marks {
  static constexpr int kMax = 5;
  hipStream_t s;
  int n;
  hipEvent_t ev[kMax] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool timed = true, set[kMax] = {false, false, false, false, false};

  Marks(hipStream_t st, int count) : s(st), n(count) {
    for (int i = 0; i < n; i++) {
      (void)hipEventCreate(&ev[i]);
      timed = timed && ev[i];
    }
  }
  ~Marks() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void mark(int i) {
    if (timed) (void)hipEventRecord(ev[i], s), set[i] = true;
  }
  // the time between two marks once the stream has passed them; 0 where there is none to report
  double ms(int i, int j) const {
    float t = 0;
    if (!set[i] || !set[j] || hipEventElapsedTime(&t, ev[i], ev[j]) != hipSuccess) t = 0;
    return (double)t;
  }
};

// What a writer's layout hands to finish_slab: the gather jobs, the bytes they copy from the meta
// section, the length of the compact buffer, and the caps of the plan that sized those sections.
struct SlabLayout {
  int64_t njobs_cap = 0, meta_cap = 0, compact_cap = 0;
  size_t o_jobs = 0, o_meta = 0, o_compact = 0;
  std::vector<GatherJob> jobs;
  std::vector<uint8_t> meta;
  int64_t cpos = 0;
};

// The tail of a slab.  rc: what the writer's part came to (the stream is synchronised either
// way).  The layout is checked against the caps that are the allocation, jobs and meta go up,
// the gather kernel runs between marks g and g + 1, the compact buffer lands at dst + *pos.
// *pos advances and *gather_ms grows only on success.
inline int finish_slab(hipStream_t s, Ring& ring, const SlabMem& mem, Marks& marks, int g, int rc,
                       const SlabLayout& L, uint8_t* dst, int64_t* pos, double* gather_ms) {
  if (rc == ZH_OK && ((int64_t)L.jobs.size() > L.njobs_cap ||
                      (int64_t)L.meta.size() > L.meta_cap || L.cpos > L.compact_cap))
    rc = ZH_EHIP;
  if (rc == ZH_OK && !L.jobs.empty()) {
    if (!ring.h2d(mem.at(L.o_jobs), (const uint8_t*)L.jobs.data(),
                  L.jobs.size() * sizeof(GatherJob)) ||
        !ring.h2d(mem.at(L.o_meta), L.meta.data(), L.meta.size()))
      rc = ZH_EHIP;
    if (rc == ZH_OK) {
      marks.mark(g);
      hipLaunchKernelGGL(blosc_gather_kernel, dim3((unsigned)L.jobs.size()), dim3(kThreads), 0, s,
                         (const GatherJob*)mem.at(L.o_jobs));
      if (hipGetLastError() != hipSuccess) rc = ZH_EHIP;
      marks.mark(g + 1);
    }
    if (rc == ZH_OK && !ring.d2h(dst + *pos, mem.at(L.o_compact), (size_t)L.cpos)) rc = ZH_EHIP;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = rc == ZH_OK ? ZH_EHIP : rc;
  if (rc != ZH_OK) return rc;
  *gather_ms += marks.ms(g, g + 1);
  *pos += L.cpos;
  return ZH_OK;
}

}  // namespace
