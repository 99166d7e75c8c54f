// zh_blosc_kernels.hip — batched device decode of blosc1 frames whose streams are LZ4, BloscLZ
// or stored raw (zh_blosc_batch_plan / zh_blosc_decode_batch / zh_debug_blosc_streams), and, with
// ZH_BLOSC_ZSTD_DEVICE / ZH_BLOSC_ZLIB_DEVICE through the _ex forms of those calls, plain zstd
// frames and zlib streams (below).
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
//
// With ZH_BLOSC_ZSTD_DEVICE (the _ex calls) frames of compressor code 4 whose streams are raw or
// one plain zstd frame each (zh_bs::zstd_stream_ok) are decoded here too, in two passes on the
// same stream:
//   pass 1  blosc_zstd_kernel, the shape of zstd_decode_kernel (zh_zstd_dec_kernels.hip): one
//           wave per zstd stream of the slab, 4 streams per workgroup, no barrier, zh_zd::Work per
//           wave in LDS (4 x 10 008 B = 40 032 B: three workgroups, 12 waves, per CU).  The wave
//           runs zh_zd::decode_frame with ZdLanes into the stream's place in the block's window:
//           the destination itself for an unshuffled block, the temporary for a shuffled one
//           whatever its size.  Modern c-blosc does not split zstd blocks, so a block is one
//           stream, and its blocks (256 KiB at clevel 5) exceed kLdsBlock: a workgroup per block
//           would idle three waves of four through the serial part and hold 64 KiB of LDS for
//           nothing.  A failing stream stores 1 to its frame's flag.
//   pass 2  blosc_decode_kernel over the blocks of those frames that are shuffled or have raw
//           streams.  A kZstd stream is already in the global window: the waves copy only the
//           raw streams of the block, barrier, and store_out undoes the shuffle.  Blocks of zstd
//           frames never take the LDS-window branch.  The kernel boundary orders pass 1's stores
//           before pass 2's loads.
//   order   inside pass 1 the argument is ZdLanes::order (zh_dec_lanes.h), the one above: a match
//           copy loads window bytes that other lanes of the same wave stored as earlier literals
//           or matches (global memory); the lanes that copy literals load Huffman literals that
//           lanes 0..3 stored to the literal scratch (global memory); every lane loads table
//           entries that lane 0 (FSE, tree description) or all lanes (Huffman fill) stored to
//           Work (LDS).  order() stands before every match copy and after every serial or
//           parallel table / literal step.  No wave reads what another wave stored: streams own
//           disjoint ranges of the window and of the scratch.
//   memory  frames are decoded in slabs: a slab closes before the zstd frame that would take its
//           decoded zstd bytes past kSlabBytes (128 MiB; a larger frame is a slab of its own).
//           Per slab the literal scratch is at most the decoded bytes of its device zstd streams
//           (Walk::max_regen <= the stream's content size, rounded up to 16 per stream) and the
//           temporary at most the decoded bytes of its shuffled blocks (rounded up to 16 per
//           block), beside the compressed bytes and the tables.  Frames of the other
//           compressors never close a slab: without the flag a batch is one slab, as before.
//   bounds  every pass-1 row is checked on the host against the staged bytes, the window it
//           writes (destination or temporary) and the scratch before launch; decode_frame
//           checks every read against csize and every write against rawsize / litcap.
//
// With ZH_BLOSC_ZLIB_DEVICE frames of compressor code 3 whose streams are raw or a zlib stream
// with compress2's header (zh_bs::zlib_stream_head_ok) take the same two passes:
//   pass 1  blosc_zlib_kernel, the shape of gzip_decode_kernel (zh_gzip_dec_kernels.hip): one wave
//           per zlib stream of the slab, 4 streams per workgroup, no barrier, zh_gd::Work per wave
//           in LDS (4 x 3 928 B = 15 712 B: ten workgroups per CU).  The wave runs
//           zh_bs::zlib_stream with ZdLanes: zh_gd::decode_zlib_stream into the stream's place in
//           the block's global window (the destination for an unshuffled block, the temporary for
//           a shuffled one), then, behind order(), the Adler-32 of that window across its lanes
//           (zh_gd::adler32: four bytes per lane and round, 64-bit partial sums, a wave
//           reduction), compared with the stored one.  Acceptance is uncompress's, the host
//           decoder's call: exactly rawsize bytes and a matching Adler-32; bytes behind the
//           trailer are ignored.  A failing stream stores 1 to its frame's flag.
//   pass 2  as for zstd frames: DevBlock::pass1 says that pass 1 wrote to the block's global
//           window, kZlib streams are skipped like kZstd ones, and an unshuffled block of zlib
//           streams only is finished by pass 1.
//   order   the argument above: match copies and the Adler-32 load window bytes that other lanes
//           of the same wave stored; the tables in Work are read by other lanes than wrote them.
//   memory  decoded bytes of zlib device frames count towards the same kSlabBytes as zstd ones,
//           which bounds the temporary; a zlib stream needs no literal scratch.
//   bounds  every pass-1 row is checked on the host against the staged bytes and its window;
//           decode_zlib_stream checks every read against csize and every write against rawsize,
//           and adler32 reads [0, rawsize) of the window only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "zh_blosc_streams.h"
#include "zh_ctx.h"
#include "zh_dec_lanes.h"
#include "zh_stager.h"
#include "zh_zstd_dec.h"

namespace {

using zh_bs::BlockRow;
using zh_bs::StreamRow;

constexpr uint32_t kLdsBlock = 64u << 10;  // largest block decoded in LDS
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int64_t kSlabBytes = (int64_t)128 << 20;  // decoded zstd / zlib frames of one slab

struct DevBlock {
  int64_t dst_off;  // in the batch destination
  int64_t tmp_off;  // in the temporary (-1: none needed)
  uint32_t size, typesize, shuffle, first_stream, nstreams, frame;  // frame: in the slab
  uint32_t pass1;   // a block of a zstd or zlib frame: its window is global memory, pass 1 wrote
                    // to it
  uint32_t pad;
};
struct DevStream {
  int64_t src_off;  // in the staged compressed bytes
  uint32_t csize, blk_off, rawsize, method;
};
struct DevZstd {     // a kZstd stream: a row of pass 1
  int64_t src_off;   // in the staged compressed bytes
  int64_t out_off;   // its place in the window: in the temporary (in_tmp) or the destination
  int64_t lit_off;   // in the literal scratch
  uint32_t csize, rawsize, litcap, frame, in_tmp, pad;
};
struct DevZlib {     // a kZlib stream: a row of pass 1
  int64_t src_off;   // in the staged compressed bytes
  int64_t out_off;   // its place in the window: in the temporary (in_tmp) or the destination
  uint32_t csize, rawsize, frame, in_tmp;
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
    // pass 1 left it in the (global) window
    if (r.method == zh_bs::kZstd || r.method == zh_bs::kZlib) continue;
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
  if (b.size <= kLdsBlock && !b.pass1) {  // uniform per workgroup
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

// Pass 1 of a zstd frame's blocks: one wave per kZstd stream, no barrier (a wave may return
// alone).  ZdLanes: zh_dec_lanes.h.
__global__ __launch_bounds__(kThreads) void blosc_zstd_kernel(
    const uint8_t* __restrict__ src, uint8_t* dst, uint8_t* tmp, uint8_t* lit,
    const DevZstd* __restrict__ rows, uint32_t nrows, uint32_t* __restrict__ flags) {
  __shared__ zh_zd::Work work[kWaves];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t k = blockIdx.x * kWaves + wave;
  if (k >= nrows) return;  // the whole wave
  const DevZstd r = rows[k];
  ZdLanes p;
  p.l = threadIdx.x & 63;
  zh_zd::Header h;
  uint64_t made = 0;
  size_t used = 0;
  zh_zd::Verdict v =
      zh_zd::decode_frame(src + r.src_off, (size_t)r.csize, (r.in_tmp ? tmp : dst) + r.out_off,
                          (uint64_t)r.rawsize, lit + r.lit_off, (uint64_t)r.litcap, work[wave], p,
                          &made, &used, &h);
  // the plan's stream: exactly rawsize bytes of content, and nothing after the frame
  if (!v && made != (uint64_t)r.rawsize) v = zh_zd::kSizeMismatch;
  if (!v && used != (size_t)r.csize) v = zh_zd::kTrailingBytes;
  if (v && p.l == 0) flags[r.frame] = 1;
}

// Pass 1 of a zlib frame's blocks: one wave per kZlib stream, no barrier (a wave may return
// alone).  zlib_stream: the DEFLATE blocks into the window, then the Adler-32 of the window.
__global__ __launch_bounds__(kThreads) void blosc_zlib_kernel(
    const uint8_t* __restrict__ src, uint8_t* dst, uint8_t* tmp, const DevZlib* __restrict__ rows,
    uint32_t nrows, uint32_t* __restrict__ flags) {
  __shared__ zh_gd::Work work[kWaves];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t k = blockIdx.x * kWaves + wave;
  if (k >= nrows) return;  // the whole wave
  const DevZlib r = rows[k];
  ZdLanes p;
  p.l = threadIdx.x & 63;
  // any verdict, another size than rawsize, another Adler-32 than the stored one
  const zh_gd::Verdict v = zh_bs::zlib_stream(
      src + r.src_off, r.csize, (r.in_tmp ? tmp : dst) + r.out_off, r.rawsize, work[wave], p);
  if (v && p.l == 0) flags[r.frame] = 1;
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

constexpr unsigned kKnownFlags = ZH_BLOSC_ZSTD_DEVICE | ZH_BLOSC_ZLIB_DEVICE;

// The flag that admits a host-decoded compressor code to the device plan (0: none does).
inline unsigned device_flag(int comp) {
  return comp == 4 ? ZH_BLOSC_ZSTD_DEVICE : comp == 3 ? ZH_BLOSC_ZLIB_DEVICE : 0u;
}

struct CountRows {  // build_table's rows, counted only
  size_t n = 0;
  template <class T>
  void push_back(const T&) {
    n++;
  }
  size_t size() const { return n; }
};

int plan_frames(zh_blosc_frame* frames, int64_t n, unsigned flags, int64_t* total, char* err,
                size_t errlen) {
  if (flags & ~kKnownFlags) {
    put_err(err, errlen, "zh_blosc_batch_plan: unknown flags");
    return ZH_EINVAL;
  }
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
    if (f.where == 1 && (flags & device_flag(h.comp))) {
      // a sound chain of raw streams and plain zstd frames (or zlib streams): the device's
      CountRows cb, cs;
      if (zh_bs::build_table((const uint8_t*)f.src, (size_t)f.srclen, h, cb, cs, &msg, flags) ==
          ZH_OK)
        f.where = 0;
    }
    pos = up(pos + f.nbytes, kAlign);
  }
  *total = pos;
  return ZH_OK;
}

// One batch call's state across its slabs.
struct Batch {
  zh_ctx* ctx;
  hipStream_t s;
  Stager* sg;
  zh_blosc_frame* frames;
  int64_t n, total;
  unsigned flags;
  uint8_t* dst;
  std::vector<char> suspect;  // the host decoder names this frame's verdict
  std::vector<uint32_t> bad;  // a stream of this frame failed on the device
  double ms = 0;
  bool timed = false;
};

// The device frames of [i0, i1): tables, upload, both passes, flags back.  `host_frames`: the
// memcpyed and host-decoded frames of the whole batch go up between the upload and the launch
// (the first slab's).  Returns ZH_OK, ZH_ENOMEM, ZH_EINVAL (too many blocks) or ZH_EHIP.
int decode_slab(Batch& B, int64_t i0, int64_t i1, bool host_frames, const char** why) {
  zh_blosc_frame* frames = B.frames;
  const int64_t ns = i1 - i0;
  hipStream_t s = B.s;
  Stager& sg = *B.sg;
  std::vector<DevBlock> blocks;
  std::vector<DevStream> streams;
  std::vector<DevZstd> zrows;
  std::vector<DevZlib> lrows;
  std::vector<int64_t> src_base((size_t)ns, -1);
  int64_t src_total = 0, tmp_total = 0, lit_total = 0;
  {
    std::vector<BlockRow> fb;
    std::vector<StreamRow> fs;
    for (int64_t i = i0; i < i1; i++) {
      const zh_blosc_frame& f = frames[i];
      if (f.where != 0 || f.nbytes == 0) {
        // an empty frame still answers for its compressor (snappy: unsupported)
        if (f.where == 0 && (((const uint8_t*)f.src)[2] >> 5) == 2) B.suspect[(size_t)i] = 1;
        continue;
      }
      zh_bs::Header h;
      const char* msg = "";
      (void)zh_bs::parse_header((const uint8_t*)f.src, (size_t)f.srclen, &h, &msg);
      fb.clear();
      fs.clear();
      if (zh_bs::build_table((const uint8_t*)f.src, (size_t)f.srclen, h, fb, fs, &msg, B.flags) !=
          ZH_OK) {
        B.suspect[(size_t)i] = 1;  // nothing of it is decoded on the device
        continue;
      }
      const bool zf = h.comp == 4 || h.comp == 3;  // a frame with streams for pass 1
      src_base[(size_t)(i - i0)] = src_total;
      for (const BlockRow& b : fb) {
        DevBlock d;
        d.dst_off = f.dst_off + b.dst_off;
        d.tmp_off = -1;
        if (b.shuffle != zh_bs::kShufNone && (zf || b.size > kLdsBlock)) {
          d.tmp_off = tmp_total;
          tmp_total = up(tmp_total + b.size, 16);
        }
        d.size = b.size, d.typesize = b.typesize, d.shuffle = b.shuffle;
        d.first_stream = (uint32_t)streams.size() + b.first_stream;
        d.nstreams = b.nstreams;
        d.frame = (uint32_t)(i - i0);
        d.pass1 = zf ? 1u : 0u;
        d.pad = 0;
        bool raw = false;
        for (uint32_t k = 0; k < b.nstreams; k++) {
          const StreamRow& r = fs[b.first_stream + k];
          if (r.method == zh_bs::kZlib) {
            DevZlib l;
            l.src_off = src_total + r.src_off;
            l.out_off = (d.tmp_off >= 0 ? d.tmp_off : d.dst_off) + (int64_t)r.blk_off;
            l.csize = r.csize, l.rawsize = r.rawsize;
            l.frame = d.frame;
            l.in_tmp = d.tmp_off >= 0 ? 1u : 0u;
            lrows.push_back(l);
            continue;
          }
          if (r.method != zh_bs::kZstd) {
            raw = true;
            continue;
          }
          DevZstd z;
          z.src_off = src_total + r.src_off;
          z.out_off = (d.tmp_off >= 0 ? d.tmp_off : d.dst_off) + (int64_t)r.blk_off;
          z.lit_off = lit_total;
          z.csize = r.csize, z.rawsize = r.rawsize, z.litcap = r.max_regen;
          z.frame = d.frame;
          z.in_tmp = d.tmp_off >= 0 ? 1u : 0u;
          z.pad = 0;
          lit_total = up(lit_total + (int64_t)r.max_regen, 16);
          zrows.push_back(z);
        }
        // an unshuffled block of zstd (or zlib) streams only is finished by pass 1
        if (!zf || raw || d.tmp_off >= 0) blocks.push_back(d);
      }
      for (const StreamRow& r : fs)
        streams.push_back({src_total + r.src_off, r.csize, r.blk_off, r.rawsize, r.method});
      src_total = up(src_total + f.srclen, 16);
    }
  }
  if (blocks.size() > (size_t)zh::kIntMax || streams.size() > (size_t)zh::kIntMax) {
    *why = "zh_blosc_decode_batch: too many blocks in one batch";
    return ZH_EINVAL;
  }
  // pass 1 writes through these rows: each inside the staged bytes, its window and the scratch
  for (const DevZstd& z : zrows) {
    const int64_t room = z.in_tmp ? tmp_total : B.total;
    if (z.src_off < 0 || z.src_off + (int64_t)z.csize > src_total || z.out_off < 0 ||
        z.out_off + (int64_t)z.rawsize > room || z.lit_off < 0 ||
        z.lit_off + (int64_t)z.litcap > lit_total) {
      *why = "zh_blosc_decode_batch: a stream row leaves its buffers";
      return ZH_EINVAL;
    }
  }
  for (const DevZlib& l : lrows) {
    const int64_t room = l.in_tmp ? tmp_total : B.total;
    if (l.src_off < 0 || l.src_off + (int64_t)l.csize > src_total || l.out_off < 0 ||
        l.out_off + (int64_t)l.rawsize > room) {
      *why = "zh_blosc_decode_batch: a stream row leaves its buffers";
      return ZH_EINVAL;
    }
  }

  // device memory: [streams | blocks | zstd rows | zlib rows | flags | compressed bytes |
  // temporary | literals]
  const size_t o_streams = 0;
  const size_t o_blocks = (size_t)up((int64_t)(streams.size() * sizeof(DevStream)), 256);
  const size_t o_zrows = o_blocks + (size_t)up((int64_t)(blocks.size() * sizeof(DevBlock)), 256);
  const size_t o_lrows = o_zrows + (size_t)up((int64_t)(zrows.size() * sizeof(DevZstd)), 256);
  const size_t o_flags = o_lrows + (size_t)up((int64_t)(lrows.size() * sizeof(DevZlib)), 256);
  const size_t o_src = o_flags + (size_t)up(ns * 4, 256);
  const size_t o_tmp = o_src + (size_t)up(src_total, 256);
  const size_t o_lit = o_tmp + (size_t)up(tmp_total, 256);
  const size_t need = o_lit + (size_t)lit_total + 256;
  void* dmem = nullptr;
  size_t got = 0;
  if (zh::ctx_alloc(B.ctx, need, &dmem, &got) != hipSuccess) {
    (void)hipGetLastError();
    *why = "zh_blosc_decode_batch: out of device memory";
    return ZH_ENOMEM;
  }
  uint8_t* d8 = (uint8_t*)dmem;
  int rc = ZH_OK;
  hipEvent_t kev[2] = {nullptr, nullptr};  // around the decode kernels
  std::vector<uint8_t> hostbuf;
  std::vector<uint32_t> flags((size_t)std::max<int64_t>(1, ns), 0);
  {
    // tables and zeroed flags, then the frames, through the ring
    sg.begin(d8);
    sg.append((const uint8_t*)streams.data(), streams.size() * sizeof(DevStream));
    sg.skip(o_blocks - streams.size() * sizeof(DevStream));
    sg.append((const uint8_t*)blocks.data(), blocks.size() * sizeof(DevBlock));
    sg.skip(o_zrows - o_blocks - blocks.size() * sizeof(DevBlock));
    sg.append((const uint8_t*)zrows.data(), zrows.size() * sizeof(DevZstd));
    sg.skip(o_lrows - o_zrows - zrows.size() * sizeof(DevZstd));
    sg.append((const uint8_t*)lrows.data(), lrows.size() * sizeof(DevZlib));
    sg.skip(o_flags - o_lrows - lrows.size() * sizeof(DevZlib));
    sg.append((const uint8_t*)flags.data(), (size_t)ns * 4);
    sg.skip(o_src - o_flags - (size_t)ns * 4);
    int64_t pos = 0;
    for (int64_t i = i0; i < i1; i++) {
      const int64_t base = src_base[(size_t)(i - i0)];
      if (base < 0) continue;
      sg.skip((size_t)(base - pos));
      sg.append((const uint8_t*)frames[i].src, (size_t)frames[i].srclen);
      pos = base + frames[i].srclen;
    }
    sg.flush();
    // memcpyed frames: one copy; host-decoded payloads: zh_blosc_decompress, then one copy
    for (int64_t i = 0; host_frames && i < B.n; i++) {
      zh_blosc_frame& f = frames[i];
      if (f.where == 2) {
        sg.copy(B.dst + f.dst_off, (const uint8_t*)f.src + 16, (size_t)f.nbytes);
      } else if (f.where == 1) {
        hostbuf.resize(std::max<size_t>(1, (size_t)f.nbytes));
        size_t nb = 0;
        char msg[256] = "";
        const int hs = zh_blosc_decompress(f.src, (size_t)f.srclen, hostbuf.data(),
                                           hostbuf.size(), &nb, msg, sizeof msg);
        f.status = hs;
        if (hs != ZH_OK) {
          B.suspect[(size_t)i] = 1;
          continue;
        }
        sg.copy(B.dst + f.dst_off, hostbuf.data(), (size_t)f.nbytes);
      }
    }
    const bool work = !blocks.empty() || !zrows.empty() || !lrows.empty();
    hipEvent_t k0 = nullptr, k1 = nullptr;
    if (work && hipEventCreate(&k0) == hipSuccess && hipEventCreate(&k1) == hipSuccess)
      (void)hipEventRecord(k0, s);
    if (!zrows.empty())
      hipLaunchKernelGGL(blosc_zstd_kernel, dim3((unsigned)((zrows.size() + kWaves - 1) / kWaves)),
                         dim3(kThreads), 0, s, d8 + o_src, B.dst, d8 + o_tmp, d8 + o_lit,
                         (const DevZstd*)(d8 + o_zrows), (uint32_t)zrows.size(),
                         (uint32_t*)(d8 + o_flags));
    if (!lrows.empty())
      hipLaunchKernelGGL(blosc_zlib_kernel, dim3((unsigned)((lrows.size() + kWaves - 1) / kWaves)),
                         dim3(kThreads), 0, s, d8 + o_src, B.dst, d8 + o_tmp,
                         (const DevZlib*)(d8 + o_lrows), (uint32_t)lrows.size(),
                         (uint32_t*)(d8 + o_flags));
    if (!blocks.empty())
      hipLaunchKernelGGL(blosc_decode_kernel, dim3((unsigned)blocks.size()), dim3(kThreads), 0, s,
                         d8 + o_src, B.dst, d8 + o_tmp, (const DevBlock*)(d8 + o_blocks),
                         (const DevStream*)(d8 + o_streams), (uint32_t*)(d8 + o_flags));
    if (hipGetLastError() != hipSuccess || sg.failed) rc = ZH_EHIP;
    if (k1) (void)hipEventRecord(k1, s);
    kev[0] = k0, kev[1] = k1;
    if (rc == ZH_OK && ns > 0 &&
        (hipMemcpyAsync(flags.data(), d8 + o_flags, (size_t)ns * 4, hipMemcpyDeviceToHost, s) !=
         hipSuccess))
      rc = ZH_EHIP;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = rc == ZH_OK ? ZH_EHIP : rc;
  float kms = 0;
  if (rc == ZH_OK && kev[0] && kev[1] && hipEventElapsedTime(&kms, kev[0], kev[1]) == hipSuccess) {
    B.ms += (double)kms;
    B.timed = true;
  }
  for (hipEvent_t e : kev)
    if (e) (void)hipEventDestroy(e);
  zh::ctx_release(B.ctx, dmem, got);
  if (rc != ZH_OK) {
    *why = "zh_blosc_decode_batch: device copy or launch failed";
    return rc;
  }
  for (int64_t i = i0; i < i1; i++) B.bad[(size_t)i] = flags[(size_t)(i - i0)];
  return ZH_OK;
}

}  // namespace

extern "C" {

int64_t zh_blosc_batch_plan_ex(zh_blosc_frame* frames, int64_t n, unsigned flags, char* err,
                               size_t errlen) {
  int64_t total = 0;
  const int st = plan_frames(frames, n, flags, &total, err, errlen);
  return st == ZH_OK ? total : -(int64_t)st;
}

int64_t zh_blosc_batch_plan(zh_blosc_frame* frames, int64_t n, char* err, size_t errlen) {
  return zh_blosc_batch_plan_ex(frames, n, 0, err, errlen);
}

double zh_debug_blosc_kernel_ms(void) { return g_last_kernel_ms.load(); }

int64_t zh_debug_blosc_streams_ex(const void* src, size_t srclen, unsigned flags, int64_t* rows,
                                  int64_t cap, char* err, size_t errlen) {
  if (flags & ~kKnownFlags) {
    put_err(err, errlen, "zh_debug_blosc_streams: unknown flags");
    return -(int64_t)ZH_EINVAL;
  }
  zh_bs::Header h;
  const char* msg = "";
  int st = zh_bs::parse_header((const uint8_t*)src, srclen, &h, &msg);
  std::vector<BlockRow> blocks;
  std::vector<StreamRow> streams;
  const bool admitted = st == ZH_OK && !h.memcpyed && (flags & device_flag(h.comp));
  if (st == ZH_OK && zh_bs::frame_where(h) != 0 && !admitted) {
    st = ZH_EUNSUPPORTED;
    msg = h.memcpyed ? "blosc frame is memcpyed: it has no streams"
                     : "blosc payload is decoded on the host";
  }
  if (st == ZH_OK)
    st = zh_bs::build_table((const uint8_t*)src, srclen, h, blocks, streams, &msg, flags);
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

int64_t zh_debug_blosc_streams(const void* src, size_t srclen, int64_t* rows, int64_t cap,
                               char* err, size_t errlen) {
  return zh_debug_blosc_streams_ex(src, srclen, 0, rows, cap, err, errlen);
}

int zh_blosc_decode_batch_ex(zh_ctx* ctx, zh_blosc_frame* frames, int64_t n, unsigned flags,
                             void* dst, int64_t dstcap, void* stream_v, char* err,
                             size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  int64_t total = 0;
  int st = plan_frames(frames, n, flags, &total, err, errlen);
  if (st != ZH_OK) return st;
  if (total > dstcap || (total > 0 && !dst)) {
    put_err(err, errlen, "blosc destination too small");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;
  Stager sg;
  if (sg.init(ctx, s) != ZH_OK) {
    (void)hipGetLastError();
    put_err(err, errlen, "zh_blosc_decode_batch: device copy or launch failed");
    return ZH_EHIP;
  }
  Batch B;
  B.ctx = ctx, B.s = s, B.sg = &sg, B.frames = frames, B.n = n, B.total = total, B.flags = flags;
  B.dst = (uint8_t*)dst;
  B.suspect.assign((size_t)n, 0);
  B.bad.assign((size_t)n, 0);
  // slabs: a zstd or zlib device frame that would take the slab's decoded bytes of such frames
  // past kSlabBytes opens the next one
  int64_t i0 = 0, zraw = 0;
  bool first = true;
  for (int64_t i = 0; i <= n; i++) {
    const bool zf = i < n && frames[i].where == 0 && frames[i].nbytes > 0 &&
                    device_flag(((const uint8_t*)frames[i].src)[2] >> 5) != 0;
    if (i == n || (zf && zraw > 0 && zraw + frames[i].nbytes > kSlabBytes)) {
      const char* why = "";
      const int rc = decode_slab(B, i0, i, first, &why);
      if (rc != ZH_OK) {
        (void)hipGetLastError();
        put_err(err, errlen, why);
        return rc;
      }
      first = false;
      i0 = i;
      zraw = 0;
    }
    if (zf) zraw += frames[i].nbytes;
  }
  if (B.timed) g_last_kernel_ms.store(B.ms);
  // the first failing frame in batch order, with the host decoder's status and text
  std::vector<uint8_t> hostbuf;
  for (int64_t i = 0; i < n; i++) {
    zh_blosc_frame& f = frames[i];
    if (!B.suspect[(size_t)i] && !B.bad[(size_t)i]) continue;
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

int zh_blosc_decode_batch(zh_ctx* ctx, zh_blosc_frame* frames, int64_t n, void* dst,
                          int64_t dstcap, void* stream_v, char* err, size_t errlen) {
  return zh_blosc_decode_batch_ex(ctx, frames, n, 0, dst, dstcap, stream_v, err, errlen);
}

}  // extern "C"
