// zh_blosc_kernels.hip — batched device decode of blosc1 frames whose streams are LZ4, BloscLZ
// or stored raw (zh_blosc_batch_plan / zh_blosc_decode_batch / zh_debug_blosc_streams).
//
// The host walks every frame once (zh_blosc_streams.h: build_table) into block and stream rows;
// the compressed bytes cross PCIe through the context's page-locked ring; one kernel decodes:
//   grid    one workgroup (4 waves) per block;
//   stream  one wave per stream (a wave takes streams w, w+4, ... of its block).  The wave reads
//           the token chain uniformly from a 64-byte register window of the stream (one load
//           per 64 input bytes, v_readlane per byte) and copies literals and matches across
//           its 64 lanes;
//   window  the shuffled block lives in LDS when it fits kLdsBlock (64 KiB: two workgroups per
//           CU under the 160 KiB limit), else in global memory: the destination itself for an
//           unshuffled block, a temporary otherwise;
//   order   a match reads bytes that other lanes of the same wave stored earlier.  After every
//           copy the wave waits for its outstanding memory operations (s_waitcnt vmcnt(0)
//           lgkmcnt(0)) inside a workgroup-scope release/acquire fence pair.  In LDS that wait
//           is the whole argument: a wave's LDS operations complete in order.  In global memory
//           the stores have reached the CU's vector L1 / L2 when vmcnt returns to 0, and the
//           later loads of the same wave go through that same L1 (write-through, shared by
//           the CU's waves), which is what workgroup scope means on gfx950 (no threadgroup
//           split mode).  Streams never read each other's bytes;
//   after   a workgroup barrier, then all 256 threads undo the byte / bit shuffle (or copy) out
//           of the window, 16 bytes per thread and store;
//   errors  a failing stream stores 1 to its frame's flag (plain vector store); the host then
//           runs zh_blosc_decompress on that frame for the status and text.
// Every row is validated on the host against the frame, the staging size and the destination
// before launch; the parsers check every read and write against (csize, rawsize).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "zh_blosc_streams.h"
#include "zh_ctx.h"
#include "zh_stager.h"

namespace {

using zh_bs::BlockRow;
using zh_bs::StreamRow;

constexpr uint32_t kLdsBlock = 64u << 10;  // largest block decoded in LDS
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;

struct DevBlock {
  int64_t dst_off;  // in the batch destination
  int64_t tmp_off;  // in the temporary (-1: none needed)
  uint32_t size, typesize, shuffle, first_stream, nstreams, frame;
};
struct DevStream {
  int64_t src_off;  // in the staged compressed bytes
  uint32_t csize, blk_off, rawsize, method;
};

// The copy policy of zh_bs::lz4_stream / blosclz_stream for one wave.
struct WaveCopy {
  uint32_t lane, base, n, w;

  __device__ static void order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ void fill(const uint8_t* s, uint32_t i) {
    base = i;
    w = (lane < n - i) ? s[i + lane] : 0u;  // i < n
  }
  __device__ void begin(const uint8_t* s, uint32_t n_) {
    n = n_;
    fill(s, 0);
  }
  __device__ uint32_t rd(const uint8_t* s, uint32_t i) {
    if (i - base >= 64u) fill(s, i);
    return (uint32_t)__builtin_amdgcn_readlane((int)w, (int)(i - base));
  }
  __device__ void lit(uint8_t* d, const uint8_t* s, uint32_t cnt) {
    for (uint32_t k = lane; k < cnt; k += 64) d[k] = s[k];
    order();
  }
  __device__ void match(uint8_t* d, uint32_t o, uint32_t off, uint32_t cnt) {
    const uint8_t* b = d + o - off;
    if (off >= cnt) {
      for (uint32_t k = lane; k < cnt; k += 64) d[o + k] = b[k];
    } else {  // pattern replication: only bytes below o are read
      for (uint32_t k = lane; k < cnt; k += 64) d[o + k] = b[k % off];
    }
    order();
  }
};

template <class Ptr>
__device__ bool decode_block_streams(const uint8_t* __restrict__ src, const DevBlock& b,
                                     const DevStream* __restrict__ streams, Ptr win,
                                     uint32_t wave, uint32_t lane) {
  bool ok = true;
  WaveCopy c;
  c.lane = lane;
  for (uint32_t s = wave; s < b.nstreams; s += kWaves) {
    const DevStream r = streams[b.first_stream + s];
    ok &= zh_bs::decode_stream(src + r.src_off, r.csize, (uint8_t*)(win + r.blk_off), r.rawsize,
                               r.method, c);
  }
  return ok;
}

__device__ void store_out(uint8_t* __restrict__ out, const uint8_t* in, const DevBlock& b,
                          uint32_t tid) {
  const bool al = (((uintptr_t)out) & 15) == 0;
  for (uint32_t q0 = tid * 16; q0 < b.size; q0 += kThreads * 16) {
    const uint32_t cnt = b.size - q0 < 16u ? b.size - q0 : 16u;
    uint32_t v[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < cnt; k++)
      v[k >> 2] |= (uint32_t)zh_bs::unshuffle_byte_at(in, q0 + k, b.size, b.typesize, b.shuffle)
                   << (8 * (k & 3));
    if (al && cnt == 16) {
      *(uint4*)(out + q0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      for (uint32_t k = 0; k < cnt; k++) out[q0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    }
  }
}

__global__ __launch_bounds__(kThreads) void blosc_decode_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint8_t* __restrict__ tmp,
    const DevBlock* __restrict__ blocks, const DevStream* __restrict__ streams,
    uint32_t* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBlock];
  const DevBlock b = blocks[blockIdx.x];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* out = dst + b.dst_off;
  bool ok;
  if (b.size <= kLdsBlock) {  // uniform per workgroup
    ok = decode_block_streams(src, b, streams, &lds[0], wave, lane);
    if (!ok) flags[b.frame] = 1;
    __syncthreads();
    store_out(out, lds, b, threadIdx.x);
    return;
  }
  uint8_t* win = b.tmp_off >= 0 ? tmp + b.tmp_off : out;
  ok = decode_block_streams(src, b, streams, win, wave, lane);
  if (!ok) flags[b.frame] = 1;
  if (b.tmp_off < 0) return;  // unshuffled: decoded in place
  __syncthreads();
  store_out(out, win, b, threadIdx.x);
}

void put_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) {
    strncpy(err, msg, errlen - 1);
    err[errlen - 1] = 0;
  }
}

std::atomic<double> g_last_kernel_ms{-1.0};

constexpr int64_t kAlign = 256;
inline int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

int plan_frames(zh_blosc_frame* frames, int64_t n, int64_t* total, char* err, size_t errlen) {
  if (n < 0 || (n > 0 && !frames)) {
    put_err(err, errlen, "zh_blosc_batch_plan: no frames");
    return ZH_EINVAL;
  }
  int64_t pos = 0;
  for (int64_t i = 0; i < n; i++) {
    zh_blosc_frame& f = frames[i];
    zh_bs::Header h;
    const char* msg = "";
    const int st = f.srclen < 0 ? ZH_EINVAL
                                : zh_bs::parse_header((const uint8_t*)f.src, (size_t)f.srclen, &h,
                                                      &msg);
    f.status = st;
    if (st != ZH_OK) {
      put_err(err, errlen, st == ZH_EINVAL ? "zh_blosc_batch_plan: negative frame length" : msg);
      return st;
    }
    f.dst_off = pos;
    f.nbytes = (int64_t)h.nbytes;
    f.where = zh_bs::frame_where(h);
    pos = up(pos + f.nbytes, kAlign);
  }
  *total = pos;
  return ZH_OK;
}

}  // namespace

extern "C" {

int64_t zh_blosc_batch_plan(zh_blosc_frame* frames, int64_t n, char* err, size_t errlen) {
  int64_t total = 0;
  const int st = plan_frames(frames, n, &total, err, errlen);
  return st == ZH_OK ? total : -(int64_t)st;
}

double zh_debug_blosc_kernel_ms(void) { return g_last_kernel_ms.load(); }

int64_t zh_debug_blosc_streams(const void* src, size_t srclen, int64_t* rows, int64_t cap,
                               char* err, size_t errlen) {
  zh_bs::Header h;
  const char* msg = "";
  int st = zh_bs::parse_header((const uint8_t*)src, srclen, &h, &msg);
  std::vector<BlockRow> blocks;
  std::vector<StreamRow> streams;
  if (st == ZH_OK && zh_bs::frame_where(h) != 0) {
    st = ZH_EUNSUPPORTED;
    msg = h.memcpyed ? "blosc frame is memcpyed: it has no streams"
                     : "blosc payload is decoded on the host";
  }
  if (st == ZH_OK) st = zh_bs::build_table((const uint8_t*)src, srclen, h, blocks, streams, &msg);
  if (st != ZH_OK) {
    put_err(err, errlen, msg);
    return -(int64_t)st;
  }
  // rows of 6 int64: a block (0, dst_off, size, typesize, shuffle, nstreams) followed by its
  // streams (1, src_off, csize, blk_off, rawsize, method)
  int64_t k = 0;
  auto put = [&](int64_t a, int64_t b, int64_t c, int64_t d, int64_t e, int64_t f) {
    if (rows && k < cap) {
      int64_t* r = rows + 6 * k;
      r[0] = a, r[1] = b, r[2] = c, r[3] = d, r[4] = e, r[5] = f;
    }
    k++;
  };
  for (const BlockRow& b : blocks) {
    put(0, b.dst_off, b.size, b.typesize, b.shuffle, b.nstreams);
    for (uint32_t s = 0; s < b.nstreams; s++) {
      const StreamRow& r = streams[b.first_stream + s];
      put(1, r.src_off, r.csize, r.blk_off, r.rawsize, r.method);
    }
  }
  return k;
}

int zh_blosc_decode_batch(zh_ctx* ctx, zh_blosc_frame* frames, int64_t n, void* dst,
                          int64_t dstcap, void* stream_v, char* err, size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  int64_t total = 0;
  int st = plan_frames(frames, n, &total, err, errlen);
  if (st != ZH_OK) return st;
  if (total > dstcap || (total > 0 && !dst)) {
    put_err(err, errlen, "blosc destination too small");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;

  // tables
  std::vector<DevBlock> blocks;
  std::vector<DevStream> streams;
  std::vector<char> suspect((size_t)n, 0);  // the host decoder names this frame's verdict
  std::vector<int64_t> src_base((size_t)n, -1);
  int64_t src_total = 0, tmp_total = 0;
  {
    std::vector<BlockRow> fb;
    std::vector<StreamRow> fs;
    for (int64_t i = 0; i < n; i++) {
      const zh_blosc_frame& f = frames[i];
      if (f.where != 0 || f.nbytes == 0) {
        // an empty frame still answers for its compressor (snappy: unsupported)
        if (f.where == 0 && (((const uint8_t*)f.src)[2] >> 5) == 2) suspect[(size_t)i] = 1;
        continue;
      }
      zh_bs::Header h;
      const char* msg = "";
      (void)zh_bs::parse_header((const uint8_t*)f.src, (size_t)f.srclen, &h, &msg);
      fb.clear();
      fs.clear();
      if (zh_bs::build_table((const uint8_t*)f.src, (size_t)f.srclen, h, fb, fs, &msg) != ZH_OK) {
        suspect[(size_t)i] = 1;  // nothing of it is decoded on the device
        continue;
      }
      src_base[(size_t)i] = src_total;
      for (const BlockRow& b : fb) {
        DevBlock d;
        d.dst_off = f.dst_off + b.dst_off;
        d.tmp_off = -1;
        if (b.size > kLdsBlock && b.shuffle != zh_bs::kShufNone) {
          d.tmp_off = tmp_total;
          tmp_total = up(tmp_total + b.size, 16);
        }
        d.size = b.size, d.typesize = b.typesize, d.shuffle = b.shuffle;
        d.first_stream = (uint32_t)streams.size() + b.first_stream;
        d.nstreams = b.nstreams;
        d.frame = (uint32_t)i;
        blocks.push_back(d);
      }
      for (const StreamRow& r : fs)
        streams.push_back({src_total + r.src_off, r.csize, r.blk_off, r.rawsize, r.method});
      src_total = up(src_total + f.srclen, 16);
    }
  }
  if (blocks.size() > (size_t)zh::kIntMax || streams.size() > (size_t)zh::kIntMax) {
    put_err(err, errlen, "zh_blosc_decode_batch: too many blocks in one batch");
    return ZH_EINVAL;
  }

  // device memory: [streams | blocks | flags | compressed bytes | temporary]
  const size_t o_streams = 0;
  const size_t o_blocks = (size_t)up((int64_t)(streams.size() * sizeof(DevStream)), 256);
  const size_t o_flags = o_blocks + (size_t)up((int64_t)(blocks.size() * sizeof(DevBlock)), 256);
  const size_t o_src = o_flags + (size_t)up((int64_t)n * 4, 256);
  const size_t o_tmp = o_src + (size_t)up(src_total, 256);
  const size_t need = o_tmp + (size_t)tmp_total + 256;
  void* dmem = nullptr;
  size_t got = 0;
  if (zh::ctx_alloc(ctx, need, &dmem, &got) != hipSuccess) {
    (void)hipGetLastError();
    put_err(err, errlen, "zh_blosc_decode_batch: out of device memory");
    return ZH_ENOMEM;
  }
  uint8_t* d8 = (uint8_t*)dmem;
  Stager sg;
  int rc = sg.init(ctx, s);
  hipEvent_t kev[2] = {nullptr, nullptr};  // around the decode kernel
  std::vector<uint8_t> hostbuf;
  std::vector<uint32_t> flags((size_t)n, 0);
  if (rc == ZH_OK) {
    // tables and zeroed flags, then the frames, through the ring
    sg.begin(d8);
    sg.append((const uint8_t*)streams.data(), streams.size() * sizeof(DevStream));
    sg.skip(o_blocks - streams.size() * sizeof(DevStream));
    sg.append((const uint8_t*)blocks.data(), blocks.size() * sizeof(DevBlock));
    sg.skip(o_flags - o_blocks - blocks.size() * sizeof(DevBlock));
    sg.append((const uint8_t*)flags.data(), (size_t)n * 4);
    sg.skip(o_src - o_flags - (size_t)n * 4);
    int64_t pos = 0;
    for (int64_t i = 0; i < n; i++) {
      if (src_base[(size_t)i] < 0) continue;
      sg.skip((size_t)(src_base[(size_t)i] - pos));
      sg.append((const uint8_t*)frames[i].src, (size_t)frames[i].srclen);
      pos = src_base[(size_t)i] + frames[i].srclen;
    }
    sg.flush();
    // memcpyed frames: one copy; host-decoded payloads: zh_blosc_decompress, then one copy
    for (int64_t i = 0; i < n && rc == ZH_OK; i++) {
      zh_blosc_frame& f = frames[i];
      if (f.where == 2) {
        sg.copy((uint8_t*)dst + f.dst_off, (const uint8_t*)f.src + 16, (size_t)f.nbytes);
      } else if (f.where == 1) {
        hostbuf.resize(std::max<size_t>(1, (size_t)f.nbytes));
        size_t nb = 0;
        char msg[256] = "";
        const int hs = zh_blosc_decompress(f.src, (size_t)f.srclen, hostbuf.data(),
                                           hostbuf.size(), &nb, msg, sizeof msg);
        f.status = hs;
        if (hs != ZH_OK) {
          suspect[(size_t)i] = 1;
          continue;
        }
        sg.copy((uint8_t*)dst + f.dst_off, hostbuf.data(), (size_t)f.nbytes);
      }
    }
    hipEvent_t k0 = nullptr, k1 = nullptr;
    if (!blocks.empty() && hipEventCreate(&k0) == hipSuccess && hipEventCreate(&k1) == hipSuccess)
      (void)hipEventRecord(k0, s);
    if (!blocks.empty())
      hipLaunchKernelGGL(blosc_decode_kernel, dim3((unsigned)blocks.size()), dim3(kThreads), 0, s,
                         d8 + o_src, (uint8_t*)dst, d8 + o_tmp,
                         (const DevBlock*)(d8 + o_blocks), (const DevStream*)(d8 + o_streams),
                         (uint32_t*)(d8 + o_flags));
    if (hipGetLastError() != hipSuccess || sg.failed) rc = ZH_EHIP;
    if (k1) (void)hipEventRecord(k1, s);
    kev[0] = k0, kev[1] = k1;
    if (rc == ZH_OK &&
        (hipMemcpyAsync(flags.data(), d8 + o_flags, (size_t)n * 4, hipMemcpyDeviceToHost, s) !=
         hipSuccess))
      rc = ZH_EHIP;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = rc == ZH_OK ? ZH_EHIP : rc;
  float kms = 0;
  if (rc == ZH_OK && kev[0] && kev[1] && hipEventElapsedTime(&kms, kev[0], kev[1]) == hipSuccess)
    g_last_kernel_ms.store((double)kms);
  for (hipEvent_t e : kev)
    if (e) (void)hipEventDestroy(e);
  zh::ctx_release(ctx, dmem, got);
  if (rc != ZH_OK) {
    (void)hipGetLastError();
    put_err(err, errlen, "zh_blosc_decode_batch: device copy or launch failed");
    return rc;
  }
  // the first failing frame in batch order, with the host decoder's status and text
  for (int64_t i = 0; i < n; i++) {
    zh_blosc_frame& f = frames[i];
    if (!suspect[(size_t)i] && !flags[(size_t)i]) continue;
    hostbuf.resize(std::max<size_t>(1, (size_t)f.nbytes));
    size_t nb = 0;
    char msg[256] = "";
    int hs = zh_blosc_decompress(f.src, (size_t)f.srclen, hostbuf.data(), hostbuf.size(), &nb,
                                 msg, sizeof msg);
    if (hs == ZH_OK) {  // the device refused what the host accepts: never silently
      hs = ZH_EDATA;
      strcpy(msg, "corrupt blosc block");
    }
    f.status = hs;
    put_err(err, errlen, msg);
    return hs;
  }
  return ZH_OK;
}

}  // extern "C"
