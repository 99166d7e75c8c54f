// zh_blosc_enc_kernels.hip — blosc1 frames written on the device, a batch at a time, with LZ4
// streams (zh_blosc_compress / zh_blosc_encode_bound / zh_blosc_encode_batch) or, with
// ZH_BLOSC_ENC_ZSTD, zstd streams, or, with ZH_BLOSC_ENC_ZLIB, zlib streams (zh_blosc_compress_ex /
// zh_blosc_encode_batch_ex).
//
// The raw bytes are in device memory (zh_array_write's chunk buffers); the frames go to the host.
//   blosc_encode_kernel<CAP>   grid: one workgroup (4 waves) per block of at most CAP bytes (16,
//           32 or 64 KiB: the smallest that holds the slab's blocks).  All 256 threads load the
//           block into LDS in its shuffled form (16-byte loads where the source is aligned; the
//           byte shuffle scatters the 16 bytes, the bit shuffle gathers 8 elements per thread).
//           After the barrier the block is read-only; wave w compresses streams w, w+4, ... with
//           zh_be::encode_stream over WaveLanes (zh_enc_device.h), its hash table (kHashSize
//           slots) in LDS next to the block, into its own region of a scratch buffer in global memory, and stores the
//           stream's csize.  A stream LZ4 does not shrink is copied raw into that region.  A wave
//           writes only its own region, so the output needs no ordering between waves; within
//           the wave the table is read and updated by different lanes in different steps, and a
//           wave's LDS operations complete in order (the fence pair only keeps the compiler
//           from moving them).  Two lanes of one step that hash to the same slot resolve by an
//           LDS atomic max: never by whichever store lands last.
//   host    one small copy brings the csize table back; a prefix sum lays the frames out
//           (a frame past nbytes + 16 becomes MEMCPYED) and builds one copy job per stream;
//   blosc_gather_kernel (zh_enc_device.h)   one workgroup per job: a 4-byte word (the csize),
//           then the bytes, from scratch (streams), from the raw source (MEMCPYED frames) or from the
//           uploaded headers and block starts, into one compact buffer of complete frames;
//   D2H     the compact buffer through the context's page-locked out ring into host memory.
// Zstd streams (the format: zh_blosc_enc.h) take three kernels in place of the first:
//   blosc_zstd_match_kernel<CAP>   the same grid, the same shuffled load (load_block) and the
//           same LDS (CAP + 16 KiB of tables: 5 / 3 / 2 workgroups per CU).  After the barrier
//           wave w runs zh_ze::match_block over WaveLanes on streams w, w+4, ...: literals to the
//           stream's region of the scratch behind the room for the 13 + 3 + 3 header bytes, the
//           (literal length, match length, offset) records to the stream's part of a list in
//           global memory, the sequence and literal counts to an info table; lane 0 writes the 13
//           bytes of the zstd frame header at the region's start.  Nothing of this is read again
//           in this kernel;
//   zstd_fse_kernel (zh_enc_device.h)   one thread per stream row: the sequences section behind
//           the literals, the size of the compressed block to the size table.  The kernel
//           boundary orders the records and literals before it;
//   blosc_raw_stream_kernel<CAP>   one workgroup per block: where the size table says that a
//           stream of the block is stored raw (zh_be::zstd_stream_size), the block is loaded
//           again in its shuffled form and those streams are copied over their regions; a
//           block without such a stream costs one read of its rows.
// Zlib streams (ZH_BLOSC_ENC_ZLIB; the format: zh_blosc_enc.h) reuse the gzip writer's kernels:
//   blosc_shuffle_kernel<CAP>   the same grid and shuffled load, LDS CAP bytes only.  After the
//           barrier the threads store the shuffled block to its 16-byte aligned region of a
//           slab-sized buffer in device memory, 16 bytes a thread from LDS, and wave w computes
//           the Adler-32 (zh_gd::adler32 over the wave) of streams w, w+4, ... from LDS into a
//           table, one word per stream;
//   zh::gzip_segments_launch (zh_gzip_enc_kernels.hip)   gzip_match_kernel and gzip_deflate_kernel
//           (or, with ZH_BLOSC_ENC_DYNAMIC, gzip_deflate_dyn_kernel) over one EncRow row per
//           16 KiB piece of every stream, the source in the shuffled buffer; the kernel boundary
//           orders the buffer before them;
//   host    the segment sizes and the Adler words come back; every size is checked against its
//           piece, summed per stream, the raw rule applied (zh_be::zlib_stream_size); the jobs:
//           per stream the csize word and 78 01, each segment from the scratch or 00 LEN NLEN and
//           the piece from the shuffled buffer, 03 00 and the Adler-32, or the whole stream from
//           the shuffled buffer.
// The host side is one function, encode_slab, over the slab driver of zh_enc_device.h (SlabMem,
// Marks, slab_end, finish_slab) and a device-side coder named after the host's: Lz4Dev, ZstdDev,
// ZlibDev.  encode_slab owns the frame format: the plan of the blocks, the caps that size the
// allocation, the largest block's CAP, and every frame's header, MEMCPYED rule, block starts and
// place.  A coder owns what one stream is: its rows and sections, its launch, the check of the
// sizes that come back and the stream's jobs (zstd: a compressed stream is two jobs, csize word +
// frame header, block header + block).
// Slabs of at most kSlabBytes of raw input bound the device memory.  LZ4: the scratch (the raw
// size) and the compact frames (the raw size and 16 bytes per frame).  Zstd: the scratch (the
// raw size and 16 bytes per stream), the records (6 bytes per 4 raw bytes: 1.5 x), the compact
// frames, and per stream 36 bytes of tables.  Zlib: the shuffled buffer (the raw size), the
// segment scratch (the raw size and up to 23 bytes a piece), the records (1.5 x), the compact
// frames and the small tables.
// Every job and block row is built on the host from validated sizes; the size tables are checked
// against the stream sizes before they lay anything out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "zh_blosc_enc.h"
#include "zh_ctx.h"
#include "zh_dec_lanes.h"
#include "zh_enc_device.h"

namespace {

constexpr uint32_t kJobBytes = 64u << 10;  // a MEMCPYED frame is copied in pieces of this size

struct EncBlock {
  uint64_t src;      // device address of the raw block
  uint64_t scratch;  // offset of the block's region in the scratch buffer
  uint32_t size, typesize, shuffle, nstreams, first_stream, pad;
};
// 16 bytes of the raw block at q0 (cnt of them valid) as four words.
__device__ void load16(const uint8_t* __restrict__ src, uint32_t q0, uint32_t cnt, bool al,
                       uint32_t v[4]) {
  if (al && cnt == 16) {
    const uint4 x = *(const uint4*)(src + q0);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    return;
  }
  v[0] = v[1] = v[2] = v[3] = 0;
  for (uint32_t k = 0; k < cnt; k++) v[k >> 2] |= (uint32_t)src[q0 + k] << (8 * (k & 3));
}

// The raw block into LDS in its shuffled form (zh_be::shuffled_byte_at, restated per shuffle so
// that the source is read once, in wide loads).
__device__ void load_block(uint8_t* lds, const uint8_t* __restrict__ src, const EncBlock& b,
                           uint32_t tid) {
  const bool al = (((uintptr_t)src) & 15) == 0;
  const uint32_t size = b.size, ts = b.typesize;
  if (b.shuffle == zh_bs::kShufByte && ts > 1) {
    const uint32_t ne = size / ts, lim = ne * ts;
    for (uint32_t q0 = tid * 16; q0 < size; q0 += kThreads * 16) {
      const uint32_t cnt = size - q0 < 16u ? size - q0 : 16u;
      uint32_t v[4];
      load16(src, q0, cnt, al, v);
      uint32_t e = q0 / ts, j = q0 % ts;
      for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t q = q0 + k;
        lds[q < lim ? j * ne + e : q] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        if (++j == ts) j = 0, e++;
      }
    }
    return;
  }
  if (b.shuffle == zh_bs::kShufBit2 || b.shuffle == zh_bs::kShufBit3) {
    const uint32_t ne = zh_bs::bitshuffle_elems(size, ts, b.shuffle), rowb = ne / 8;
    // unit (j, p): byte j of elements 8p .. 8p+7 -> bit rows j*8 .. j*8+7, byte p
    for (uint32_t u = tid; u < ts * rowb; u += kThreads) {
      const uint32_t j = u / rowb, p = u % rowb;
      uint32_t x[8];
      for (uint32_t m = 0; m < 8; m++) x[m] = src[(size_t)(8 * p + m) * ts + j];
      for (uint32_t k = 0; k < 8; k++) {
        uint32_t o = 0;
        for (uint32_t m = 0; m < 8; m++) o |= ((x[m] >> k) & 1u) << m;
        lds[(j * 8 + k) * rowb + p] = (uint8_t)o;
      }
    }
    for (uint32_t q = ne * ts + tid; q < size; q += kThreads) lds[q] = src[q];
    return;
  }
  for (uint32_t q0 = tid * 16; q0 < size; q0 += kThreads * 16) {
    const uint32_t cnt = size - q0 < 16u ? size - q0 : 16u;
    uint32_t v[4];
    load16(src, q0, cnt, al, v);
    if (cnt == 16) {
      *(uint4*)(lds + q0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      for (uint32_t k = 0; k < cnt; k++) lds[q0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// CAP: the largest block of the launch.  The streams are latency-bound (one dependent step per
// LZ4 sequence), so what LDS a launch does not need buys resident waves: 16, 32 and 64 KiB of
// block plus the 16 KiB of tables are 5, 3 and 2 workgroups per CU.
template <uint32_t CAP>
__global__ __launch_bounds__(kThreads) void blosc_encode_kernel(
    const EncBlock* __restrict__ blocks, uint8_t* __restrict__ scratch,
    uint32_t* __restrict__ csizes) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[CAP];
  __shared__ uint32_t tables[kWaves][zh_be::kHashSize];
  const EncBlock b = blocks[blockIdx.x];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  load_block(lds, (const uint8_t*)b.src, b, threadIdx.x);
  __syncthreads();
  WaveLanes w;
  w.lane = lane;
  w.h = 0;
  const uint32_t neb = b.size / b.nstreams;
  for (uint32_t s = wave; s < b.nstreams; s += kWaves) {
    const uint8_t* st = lds + (size_t)s * neb;
    uint8_t* out = scratch + b.scratch + (size_t)s * neb;
    const uint32_t cs = zh_be::encode_stream(st, neb, out, tables[wave], w);
    if (cs == neb) {  // stored raw: the shuffled bytes themselves
      WaveLanes::drain_stores();
      w.copy(out, st, neb);
    }
    if (lane == 0) csizes[b.first_stream + s] = cs;
  }
}

// The first phase of the zstd streams: rows[b.first_stream + s] names stream s's block region
// (out, behind the kZstdHead bytes of headers) and records (seq).
template <uint32_t CAP>
__global__ __launch_bounds__(kThreads) void blosc_zstd_match_kernel(
    const EncBlock* __restrict__ blocks, const EncRow* __restrict__ rows,
    uint8_t* __restrict__ scratch, uint16_t* __restrict__ seqs, uint32_t* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[CAP];
  __shared__ uint32_t tables[kWaves][zh_be::kHashSize];
  const EncBlock b = blocks[blockIdx.x];
  if (b.size > CAP) return;  // never: the host picks CAP from the block sizes (all threads)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  load_block(lds, (const uint8_t*)b.src, b, threadIdx.x);
  __syncthreads();
  WaveLanes w;
  w.lane = lane;
  w.h = 0;
  w.wide = true;
  const uint32_t neb = b.size / b.nstreams;
  for (uint32_t s = wave; s < b.nstreams; s += kWaves) {
    const uint32_t k = b.first_stream + s;
    const EncRow r = rows[k];
    uint32_t nl = 0;
    const uint32_t ns = zh_ze::match_block(lds + (size_t)s * neb, neb, scratch + r.out + 3,
                                           seqs + r.seq, tables[wave], w, &nl);
    if (lane == 0) {
      zh_ze::put_frame_header(scratch + r.out - zh_be::kZstdHead, neb, false);
      info[2 * k] = ns;
      info[2 * k + 1] = nl;
    }
  }
}

// The streams the size table stores raw, in their shuffled form, over their regions.
template <uint32_t CAP>
__global__ __launch_bounds__(kThreads) void blosc_raw_stream_kernel(
    const EncBlock* __restrict__ blocks, const EncRow* __restrict__ rows,
    const uint32_t* __restrict__ csize, uint8_t* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[CAP];
  const EncBlock b = blocks[blockIdx.x];
  if (b.size > CAP) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t neb = b.size / b.nstreams;
  bool any = false;  // the same for every thread: the barrier below is reached by all or none
  for (uint32_t s = 0; s < b.nstreams; s++)
    any |= zh_be::zstd_stream_size(neb, csize[b.first_stream + s]) == neb;
  if (!any) return;
  load_block(lds, (const uint8_t*)b.src, b, threadIdx.x);
  __syncthreads();
  for (uint32_t s = wave; s < b.nstreams; s += kWaves) {
    const uint32_t k = b.first_stream + s;
    if (zh_be::zstd_stream_size(neb, csize[k]) != neb) continue;
    uint8_t* out = scratch + rows[k].out - zh_be::kZstdHead;
    for (uint32_t q = lane; q < neb; q += 64) out[q] = lds[(size_t)s * neb + q];
  }
}

// The first phase of the zlib streams: the block in its shuffled form to shuf + b.scratch (the
// pieces the gzip kernels read, and the streams stored raw), and every stream's Adler-32.
template <uint32_t CAP>
__global__ __launch_bounds__(kThreads) void blosc_shuffle_kernel(
    const EncBlock* __restrict__ blocks, uint8_t* __restrict__ shuf,
    uint32_t* __restrict__ adlers) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[CAP];
  const EncBlock b = blocks[blockIdx.x];
  if (b.size > CAP) return;  // never: the host picks CAP from the block sizes (all threads)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  load_block(lds, (const uint8_t*)b.src, b, threadIdx.x);
  __syncthreads();
  uint8_t* __restrict__ out = shuf + b.scratch;  // 16-byte aligned, up(size, 16) long
  const uint32_t whole = b.size & ~15u;
  for (uint32_t q0 = threadIdx.x * 16; q0 < whole; q0 += kThreads * 16)
    *(uint4*)(out + q0) = *(const uint4*)(lds + q0);
  for (uint32_t q = whole + threadIdx.x; q < b.size; q += kThreads) out[q] = lds[q];
  ZdLanes p{lane};
  const uint32_t neb = b.size / b.nstreams;
  for (uint32_t s = wave; s < b.nstreams; s += kWaves) {
    const uint32_t a = zh_gd::adler32(lds + (size_t)s * neb, neb, p);
    if (lane == 0) adlers[b.first_stream + s] = a;
  }
}

std::atomic<double> g_last_enc_ms{-1.0};
// the zlib route's kernels apart: shuffle + Adler-32, match + coder, gather (-1: none yet)
std::atomic<double> g_last_zlib_part[3] = {{-1.0}, {-1.0}, {-1.0}};

// ---- the device-side coders of encode_slab, named after the host's (zh_blosc_enc.h) ------------
// A coder is what one stream adds to a slab.  While the frames are planned: begin_block (the
// block's region, EncBlock::scratch), add_stream (its rows and sizes; returns the gather jobs it
// may need), end_block, nrows.  Then reserve (its sections of the slab's memory), upload (its
// rows, once the addresses are known), launch<CAP> (its kernels over the blocks), sizes (its
// tables back and checked: nothing in them may lay out a copy past its stream; csz[k]: the
// stored size of stream k) and emit (the gather jobs and meta bytes of one stream of stored size
// c at dst; false: layout and size disagree).  kCode: the compressor code of the frame;
// kStreamMeta: meta bytes a stream may need; kMid: the mark between the coder's two timed phases
// (1: it has one).

struct Lz4Dev {
  static constexpr uint32_t kCode = zh_be::Lz4Coder::kCode;
  static constexpr int64_t kStreamMeta = 0;
  static constexpr int kMid = 1;
  int64_t scratch_total = 0;
  size_t o_cs = 0, o_scratch = 0;
  uint64_t d_scratch = 0;

  uint64_t begin_block() const { return (uint64_t)scratch_total; }
  int64_t add_stream(uint32_t, uint32_t) { return 1; }
  void end_block(uint32_t size) { scratch_total += up(size, 16); }
  size_t nrows() const { return 0; }
  void reserve(SlabMem& mem, size_t nst) {
    o_cs = mem.add((int64_t)nst * 4);
    o_scratch = mem.add(scratch_total);
  }
  bool upload(Ring&, const SlabMem& mem) {
    d_scratch = mem.addr(o_scratch);
    return true;
  }
  template <uint32_t CAP>
  int launch(hipStream_t s, Marks&, const SlabMem& mem, const EncBlock* blocks, unsigned nblocks) {
    hipLaunchKernelGGL(blosc_encode_kernel<CAP>, dim3(nblocks), dim3(kThreads), 0, s, blocks,
                       mem.at(o_scratch), (uint32_t*)mem.at(o_cs));
    return hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
  }
  int sizes(Ring& ring, const SlabMem& mem, const std::vector<uint32_t>& raw,
            std::vector<uint32_t>& csz) {
    if (!ring.d2h((uint8_t*)csz.data(), mem.at(o_cs), csz.size() * 4)) return ZH_EHIP;
    for (size_t k = 0; k < csz.size(); k++)
      if (csz[k] == 0 || csz[k] > raw[k]) return ZH_EHIP;
    return ZH_OK;
  }
  bool emit(SlabLayout& L, const EncBlock& b, uint32_t q, uint32_t neb, uint32_t c, uint64_t,
            uint64_t dst) {
    L.jobs.push_back({d_scratch + b.scratch + (uint64_t)q * neb, dst, c, c, 4, 0});
    return true;
  }
};

// One row per stream: its block region (out, behind the kZstdHead bytes of headers) and records.
struct ZstdDev {
  static constexpr uint32_t kCode = zh_be::ZstdCoder::kCode;
  static constexpr int64_t kStreamMeta = 0;
  static constexpr int kMid = 1;
  const zh_ze::Tables* dtab;  // the encoding tables in device memory
  std::vector<EncRow> rows;
  int64_t scratch_total = 0, seq_total = 0;
  size_t o_cs = 0, o_rows = 0, o_info = 0, o_seq = 0, o_scratch = 0;
  uint64_t d_scratch = 0;

  uint64_t begin_block() const { return (uint64_t)scratch_total; }
  int64_t add_stream(uint32_t, uint32_t neb) {  // region: [headers | block], 16-byte aligned
    rows.push_back({0, (uint64_t)scratch_total + zh_be::kZstdHead, (uint64_t)seq_total, neb, 0});
    scratch_total += up((int64_t)neb + zh_be::kZstdHead, 16);
    seq_total += up(3 * (int64_t)(neb / 4) + 3, 8);
    return 2;
  }
  void end_block(uint32_t) {}
  size_t nrows() const { return rows.size(); }
  void reserve(SlabMem& mem, size_t nst) {
    o_cs = mem.add((int64_t)nst * 4);
    o_rows = mem.add((int64_t)(rows.size() * sizeof(EncRow)));
    o_info = mem.add((int64_t)rows.size() * 8);
    o_seq = mem.add(seq_total * 2);
    o_scratch = mem.add(scratch_total);
  }
  bool upload(Ring& ring, const SlabMem& mem) {
    d_scratch = mem.addr(o_scratch);
    return ring.h2d(mem.at(o_rows), (const uint8_t*)rows.data(), rows.size() * sizeof(EncRow));
  }
  template <uint32_t CAP>
  int launch(hipStream_t s, Marks&, const SlabMem& mem, const EncBlock* blocks, unsigned nblocks) {
    const EncRow* d_rows = (const EncRow*)mem.at(o_rows);
    const unsigned nstreams = (unsigned)rows.size();
    uint32_t* info = (uint32_t*)mem.at(o_info);
    uint32_t* csize = (uint32_t*)mem.at(o_cs);
    hipLaunchKernelGGL(blosc_zstd_match_kernel<CAP>, dim3(nblocks), dim3(kThreads), 0, s, blocks,
                       d_rows, mem.at(o_scratch), (uint16_t*)mem.at(o_seq), info);
    hipLaunchKernelGGL(zstd_fse_kernel, dim3((nstreams + 63) / 64), dim3(64), 0, s, d_rows,
                       nstreams, dtab, mem.at(o_scratch), (const uint16_t*)mem.at(o_seq),
                       (const uint32_t*)info, csize);
    hipLaunchKernelGGL(blosc_raw_stream_kernel<CAP>, dim3(nblocks), dim3(kThreads), 0, s, blocks,
                       d_rows, (const uint32_t*)csize, mem.at(o_scratch));
    return hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
  }
  // the table holds the sizes of the compressed blocks, the raw size where there is none
  int sizes(Ring& ring, const SlabMem& mem, const std::vector<uint32_t>& raw,
            std::vector<uint32_t>& csz) {
    if (!ring.d2h((uint8_t*)csz.data(), mem.at(o_cs), csz.size() * 4)) return ZH_EHIP;
    for (size_t k = 0; k < csz.size(); k++) {
      if (csz[k] == 0 || csz[k] > raw[k]) return ZH_EHIP;
      csz[k] = zh_be::zstd_stream_size(raw[k], csz[k]);
    }
    return ZH_OK;
  }
  // the stream's region: a raw stream, or [frame header | room | block]
  bool emit(SlabLayout& L, const EncBlock& b, uint32_t q, uint32_t neb, uint32_t c, uint64_t,
            uint64_t dst) {
    const uint64_t blk = d_scratch + rows[b.first_stream + q].out;
    const uint64_t reg = blk - zh_be::kZstdHead;
    if (c == neb) {
      L.jobs.push_back({reg, dst, c, c, 4, 0});
    } else {
      const uint32_t fh = (uint32_t)zh_ze::kFrameHeader, bsz = c - zh_be::kZstdHead;
      L.jobs.push_back({reg, dst, fh, c, 4, 0});
      L.jobs.push_back({blk, dst + 4 + fh, bsz, zh_ze::block_header(bsz, 2, true), 3, 0});
    }
    return true;
  }
};

// One row per 16 KiB piece of every stream, the source in the shuffled buffer (the blocks'
// regions, EncBlock::scratch); the segments are the gzip writer's (zh::gzip_segments_launch).
struct ZlibDev {
  static constexpr uint32_t kCode = zh_be::ZlibCoder::kCode;
  static constexpr int64_t kStreamMeta = 8;  // 78 01 | 03 00 and the Adler-32
  static constexpr int kMid = 4;             // behind the shuffle
  bool dynamic;                              // ZH_BLOSC_ENC_DYNAMIC
  std::vector<EncRow> rows;
  std::vector<uint32_t> stream_row;  // the first row of every stream
  std::vector<uint32_t> seg, adlers;  // as they came back: per row, per stream
  int64_t shuf_total = 0, scratch_total = 0, seq_total = 0;
  size_t o_rows = 0, o_cs = 0, o_adler = 0, o_info = 0, o_seq = 0, o_shuf = 0, o_scratch = 0;
  uint64_t d_shuf = 0, d_scratch = 0;

  uint64_t begin_block() const { return (uint64_t)shuf_total; }
  int64_t add_stream(uint32_t q, uint32_t neb) {
    stream_row.push_back((uint32_t)rows.size());
    const uint32_t np = zh_be::zlib_pieces(neb);
    for (uint32_t j = 0; j < np; j++) {  // src: an offset here, an address once upload knows it
      const uint32_t psz = zh_be::zlib_piece_size(neb, j);
      rows.push_back({(uint64_t)shuf_total + (uint64_t)q * neb + (uint64_t)j * zh_be::kZlibPiece,
                      (uint64_t)scratch_total, (uint64_t)seq_total, psz, 0});
      scratch_total += up((int64_t)psz + 8, 16);  // size + 4 bytes, stored as whole words
      seq_total += up(3 * (int64_t)(psz / 4) + 3, 8);
    }
    return 2 + 2 * (int64_t)np;
  }
  void end_block(uint32_t size) { shuf_total += up(size, 16); }
  size_t nrows() const { return rows.size(); }
  void reserve(SlabMem& mem, size_t nst) {
    o_rows = mem.add((int64_t)(rows.size() * sizeof(EncRow)));
    o_cs = mem.add((int64_t)rows.size() * 4);
    o_adler = mem.add((int64_t)nst * 4);
    o_info = mem.add((int64_t)rows.size() * 8);
    o_seq = mem.add(seq_total * 2);
    o_shuf = mem.add(shuf_total);
    o_scratch = mem.add(scratch_total);
  }
  bool upload(Ring& ring, const SlabMem& mem) {
    d_shuf = mem.addr(o_shuf), d_scratch = mem.addr(o_scratch);
    for (EncRow& r : rows) r.src += d_shuf;
    return ring.h2d(mem.at(o_rows), (const uint8_t*)rows.data(), rows.size() * sizeof(EncRow));
  }
  template <uint32_t CAP>
  int launch(hipStream_t s, Marks& marks, const SlabMem& mem, const EncBlock* blocks,
             unsigned nblocks) {
    hipLaunchKernelGGL(blosc_shuffle_kernel<CAP>, dim3(nblocks), dim3(kThreads), 0, s, blocks,
                       mem.at(o_shuf), (uint32_t*)mem.at(o_adler));
    const int rc = hipGetLastError() == hipSuccess ? ZH_OK : ZH_EHIP;
    marks.mark(kMid);
    if (rc != ZH_OK) return rc;
    return zh::gzip_segments_launch(s, mem.at(o_rows), (uint32_t)rows.size(), dynamic,
                                    mem.at(o_scratch), (uint16_t*)mem.at(o_seq),
                                    (uint32_t*)mem.at(o_info), (uint32_t*)mem.at(o_cs));
  }
  // nothing in the segment table may pass its piece's stored size; summed per stream
  int sizes(Ring& ring, const SlabMem& mem, const std::vector<uint32_t>& raw,
            std::vector<uint32_t>& csz) {
    seg.assign(rows.size(), 0), adlers.assign(raw.size(), 0);
    if (!ring.d2h((uint8_t*)seg.data(), mem.at(o_cs), seg.size() * 4) ||
        !ring.d2h((uint8_t*)adlers.data(), mem.at(o_adler), adlers.size() * 4))
      return ZH_EHIP;
    for (size_t k = 0; k < seg.size(); k++)
      if (seg[k] < zh_gz::kMinSegment || seg[k] > rows[k].size + zh_gz::kStoredOver) return ZH_EHIP;
    for (size_t k = 0; k < raw.size(); k++) {
      uint64_t segs = 0;
      for (uint32_t j = 0, np = zh_be::zlib_pieces(raw[k]); j < np; j++)
        segs += seg[stream_row[k] + j];
      csz[k] = zh_be::zlib_stream_size(raw[k], segs);
    }
    return ZH_OK;
  }
  // the csize word and 78 01, each segment from the scratch or 00 LEN NLEN and the piece from the
  // shuffled buffer, 03 00 and the Adler-32; or the whole stream raw from the shuffled buffer
  bool emit(SlabLayout& L, const EncBlock& b, uint32_t q, uint32_t neb, uint32_t c,
            uint64_t d_meta, uint64_t dst) {
    if (c == neb) {
      L.jobs.push_back({d_shuf + b.scratch + (uint64_t)q * neb, dst, c, c, 4, 0});
      return true;
    }
    const uint32_t st = b.first_stream + q;
    const size_t sm = L.meta.size();
    L.meta.resize(sm + (size_t)kStreamMeta);
    zh_be::put_zlib_head(L.meta.data() + sm);
    zh_be::put_zlib_tail(L.meta.data() + sm + 2, adlers[st]);
    uint64_t d = dst;
    L.jobs.push_back({d_meta + sm, d, 2, c, 4, 0});
    d += 4 + 2;
    for (uint32_t j = 0, np = zh_be::zlib_pieces(neb); j < np; j++) {
      const EncRow& r = rows[stream_row[st] + j];
      const uint32_t size = seg[stream_row[st] + j];
      if (size == r.size + zh_gz::kStoredOver) {  // 00, then LEN NLEN and the bytes
        L.jobs.push_back({d_meta + sm, d, 0, 0, 1, 0});
        L.jobs.push_back({r.src, d + 1, r.size, zh_gz::stored_word(r.size), 4, 0});
      } else {
        L.jobs.push_back({d_scratch + r.out, d, size, 0, 0, 0});
      }
      d += size;
    }
    L.jobs.push_back({d_meta + sm + 2, d, (uint32_t)zh_gz::kEnding + 4, 0, 0, 0});
    d += zh_gz::kEnding + 4;
    return d - dst == 4 + (uint64_t)c;
  }
};

struct FramePlan {
  zh_be::Layout L;
  int64_t first_block = 0, first_stream = 0, nstreams = 0;  // within the slab
  bool raw_only = false;  // the block starts alone pass the bound: MEMCPYED without a launch
};

// One slab [f0, f1) of the batch; *pos: the running offset in dst.  The frame format is here
// (the plan of the blocks, the caps, the layout of every frame); what a stream is, is the coder's.
// part_ms: the coder's first phase, its second (0: it has one), the gather.
template <class Coder>
int encode_slab(zh_ctx* ctx, hipStream_t s, Ring& ring, zh_blosc_enc_frame* frames, int64_t f0,
                int64_t f1, const zh_blosc_enc_params* prm, Coder coder, uint8_t* dst,
                int64_t* pos, double* kernel_ms, double* part_ms) {
  std::vector<FramePlan> plan((size_t)(f1 - f0));
  std::vector<EncBlock> blocks;
  std::vector<uint32_t> stream_raw;  // raw size per stream
  SlabLayout L;
  for (int64_t i = f0; i < f1; i++) {
    FramePlan& fp = plan[(size_t)(i - f0)];
    const size_t n = (size_t)frames[i].nbytes;
    (void)zh_be::make_layout(n, prm, &fp.L);  // validated by the caller
    zh_be::with_compressor(&fp.L, Coder::kCode);
    fp.first_block = (int64_t)blocks.size();
    fp.first_stream = (int64_t)stream_raw.size();
    fp.raw_only = 4 * (size_t)fp.L.nblocks > n;
    int64_t frame_jobs = 0;
    for (uint32_t k = 0; k < fp.L.nblocks && !fp.raw_only; k++) {
      EncBlock b;
      b.size = zh_be::block_size(fp.L, n, k);
      b.nstreams = zh_be::block_streams(fp.L, b.size);
      b.src = (uint64_t)(uintptr_t)frames[i].src + (uint64_t)k * fp.L.blocksize;
      b.scratch = coder.begin_block();
      b.typesize = fp.L.typesize, b.shuffle = fp.L.shuffle;
      b.first_stream = (uint32_t)stream_raw.size();
      b.pad = 0;
      const uint32_t neb = b.size / b.nstreams;
      for (uint32_t q = 0; q < b.nstreams; q++) {
        stream_raw.push_back(neb);
        frame_jobs += coder.add_stream(q, neb);
      }
      blocks.push_back(b);
      coder.end_block(b.size);
    }
    fp.nstreams = (int64_t)stream_raw.size() - fp.first_stream;
    L.compact_cap += up((int64_t)n + 16, 16);
    L.meta_cap += 16 + (fp.raw_only ? 0 : 4 * (int64_t)fp.L.nblocks) +
                  Coder::kStreamMeta * fp.nstreams;
    L.njobs_cap += 1 + std::max<int64_t>(frame_jobs, ((int64_t)n + kJobBytes - 1) / kJobBytes);
  }
  if (blocks.size() > (size_t)zh::kIntMax || stream_raw.size() > (size_t)zh::kIntMax ||
      coder.nrows() > (size_t)zh::kIntMax || L.njobs_cap > zh::kIntMax)
    return ZH_EINVAL;

  // device memory: [blocks | the coder's sections | jobs | meta | compact]
  SlabMem mem;
  const size_t o_blocks = mem.add((int64_t)(blocks.size() * sizeof(EncBlock)));
  coder.reserve(mem, stream_raw.size());
  L.o_jobs = mem.add(L.njobs_cap * (int64_t)sizeof(GatherJob));
  L.o_meta = mem.add(L.meta_cap);
  L.o_compact = mem.add(L.compact_cap);
  int rc = mem.alloc(ctx);
  if (rc != ZH_OK) return rc;
  Marks marks(s, Coder::kMid == 1 ? 4 : 5);  // 0 the coder's kernels 1, 2 gather 3
  std::vector<uint32_t> cs(stream_raw.size(), 0);  // stored size per stream
  if (!blocks.empty()) {
    if (!ring.h2d(mem.at(o_blocks), (const uint8_t*)blocks.data(),
                  blocks.size() * sizeof(EncBlock)) ||
        !coder.upload(ring, mem))
      rc = ZH_EHIP;
    if (rc == ZH_OK) {
      marks.mark(0);
      uint32_t cap = 0;
      for (const EncBlock& b : blocks) cap = std::max(cap, b.size);
      const EncBlock* db = (const EncBlock*)mem.at(o_blocks);
      const unsigned nb = (unsigned)blocks.size();
      rc = cap <= (16u << 10)   ? coder.template launch<(16u << 10)>(s, marks, mem, db, nb)
           : cap <= (32u << 10) ? coder.template launch<(32u << 10)>(s, marks, mem, db, nb)
                                : coder.template launch<zh_be::kMaxBlock>(s, marks, mem, db, nb);
      marks.mark(1);
    }
    if (rc == ZH_OK) rc = coder.sizes(ring, mem, stream_raw, cs);
  }

  // layout: the frames side by side in the compact buffer, each 16-byte aligned
  if (rc == ZH_OK) {
    L.meta.reserve((size_t)L.meta_cap);
    L.jobs.reserve((size_t)L.njobs_cap);
    const uint64_t d_meta = mem.addr(L.o_meta), d_compact = mem.addr(L.o_compact);
    for (int64_t i = f0; i < f1; i++) {
      const FramePlan& fp = plan[(size_t)(i - f0)];
      const zh_be::Layout& Lf = fp.L;
      const size_t n = (size_t)frames[i].nbytes;
      size_t total = 16 + 4 * (size_t)Lf.nblocks;
      for (int64_t q = 0; q < fp.nstreams; q++) total += 4 + (size_t)cs[(size_t)(fp.first_stream + q)];
      const bool memcpyed = n == 0 || fp.raw_only || total > n + 16;
      const size_t cbytes = memcpyed ? n + 16 : total;
      const size_t m0 = L.meta.size();
      L.meta.resize(m0 + 16 + (memcpyed ? 0 : 4 * (size_t)Lf.nblocks));
      zh_be::put_header(L.meta.data() + m0, Lf, memcpyed ? zh_be::memcpyed_flags(Lf) : Lf.flags, n,
                        cbytes);
      const uint64_t fbase = d_compact + (uint64_t)L.cpos;
      L.jobs.push_back({d_meta + m0, fbase, (uint32_t)(L.meta.size() - m0), 0, 0, 0});
      if (memcpyed) {
        for (size_t o = 0; o < n; o += kJobBytes)
          L.jobs.push_back({(uint64_t)(uintptr_t)frames[i].src + o, fbase + 16 + o,
                            (uint32_t)std::min<size_t>(kJobBytes, n - o), 0, 0, 0});
      } else {
        size_t p = 16 + 4 * (size_t)Lf.nblocks;
        for (uint32_t k = 0; k < Lf.nblocks; k++) {
          const EncBlock& b = blocks[(size_t)fp.first_block + k];
          zh_be::wr32(L.meta.data() + m0 + 16 + 4 * (size_t)k, (uint32_t)p);
          const uint32_t neb = b.size / b.nstreams;
          for (uint32_t q = 0; q < b.nstreams; q++) {
            const uint32_t c = cs[b.first_stream + q];
            if (!coder.emit(L, b, q, neb, c, d_meta, fbase + p)) rc = ZH_EHIP;
            p += 4 + (size_t)c;
          }
        }
      }
      frames[i].dst_off = *pos + L.cpos;
      frames[i].cbytes = (int64_t)cbytes;
      frames[i].status = ZH_OK;
      L.cpos += up((int64_t)cbytes, 16);
    }
  }
  double gather_ms = 0;
  rc = finish_slab(s, ring, mem, marks, 2, rc, L, dst, pos, &gather_ms);
  if (rc == ZH_OK) {
    const double a = marks.ms(0, Coder::kMid), c = Coder::kMid == 1 ? 0 : marks.ms(Coder::kMid, 1);
    *kernel_ms += a + c + gather_ms;
    part_ms[0] += a, part_ms[1] += c, part_ms[2] += gather_ms;
  }
  return rc;
}

int64_t bound_of(const zh_blosc_enc_frame* frames, int64_t n, const zh_blosc_enc_params* prm) {
  if (n < 0 || (n > 0 && !frames)) return -(int64_t)ZH_EINVAL;
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    zh_be::Layout L;
    if (frames[i].nbytes < 0 || zh_be::make_layout((size_t)frames[i].nbytes, prm, &L) != ZH_OK ||
        (frames[i].nbytes > 0 && !frames[i].src))
      return -(int64_t)ZH_EINVAL;
    total += up(frames[i].nbytes + 16, 16);
  }
  return total;
}

constexpr const char* kBadFlags =
    "blosc encode: flags are 0, ZH_BLOSC_ENC_ZSTD, ZH_BLOSC_ENC_ZLIB or ZH_BLOSC_ENC_ZLIB | "
    "ZH_BLOSC_ENC_DYNAMIC";
constexpr unsigned kZlibDyn = ZH_BLOSC_ENC_ZLIB | ZH_BLOSC_ENC_DYNAMIC;
bool flags_ok(unsigned flags) {
  return flags == 0 || flags == ZH_BLOSC_ENC_ZSTD || flags == ZH_BLOSC_ENC_ZLIB ||
         flags == kZlibDyn;
}
constexpr const char* kBadParams =
    "blosc encode: typesize 1..255, shuffle 0..2, blocksize >= 0, frames of at most 2 GiB";

}  // namespace

extern "C" {

int zh_blosc_compress_ex(const void* src, size_t n, const zh_blosc_enc_params* params,
                         unsigned flags, void* dst, size_t cap, size_t* cbytes, char* err,
                         size_t errlen) {
  if (!flags_ok(flags)) {
    put_err(err, errlen, kBadFlags);
    return ZH_EINVAL;
  }
  size_t cb = 0;
  const char* msg = "";
  int st;
  try {
    if (flags & ZH_BLOSC_ENC_ZSTD) {
      zh_be::ZstdCoder coder(zh_ze::tables());
      st = zh_be::compress_frame((const uint8_t*)src, n, params, (uint8_t*)dst, cap, &cb, &msg,
                                 coder);
    } else if (flags & ZH_BLOSC_ENC_ZLIB) {
      zh_be::ZlibCoder coder((flags & ZH_BLOSC_ENC_DYNAMIC) != 0);
      st = zh_be::compress_frame((const uint8_t*)src, n, params, (uint8_t*)dst, cap, &cb, &msg,
                                 coder);
    } else {
      zh_be::Lz4Coder coder;
      st = zh_be::compress_frame((const uint8_t*)src, n, params, (uint8_t*)dst, cap, &cb, &msg,
                                 coder);
    }
  } catch (const std::bad_alloc&) {
    st = ZH_ENOMEM, msg = "zh_blosc_compress: out of memory";
  }
  if (st != ZH_OK) {
    put_err(err, errlen, msg);
    return st;
  }
  if (cbytes) *cbytes = cb;
  return ZH_OK;
}

int zh_blosc_compress(const void* src, size_t n, const zh_blosc_enc_params* params, void* dst,
                      size_t cap, size_t* cbytes, char* err, size_t errlen) {
  return zh_blosc_compress_ex(src, n, params, 0, dst, cap, cbytes, err, errlen);
}

int64_t zh_blosc_encode_bound(const zh_blosc_enc_frame* frames, int64_t n,
                              const zh_blosc_enc_params* params) {
  return bound_of(frames, n, params);
}

double zh_debug_blosc_encode_kernel_ms(void) { return g_last_enc_ms.load(); }

void zh_debug_blosc_zlib_encode_parts_ms(double out[3]) {
  for (int k = 0; k < 3; k++) out[k] = g_last_zlib_part[k].load();
}

int zh_blosc_encode_batch(zh_ctx* ctx, zh_blosc_enc_frame* frames, int64_t n,
                          const zh_blosc_enc_params* params, void* dst, int64_t dstcap,
                          void* stream_v, char* err, size_t errlen) {
  return zh_blosc_encode_batch_ex(ctx, frames, n, params, 0, dst, dstcap, stream_v, err, errlen);
}

int zh_blosc_encode_batch_ex(zh_ctx* ctx, zh_blosc_enc_frame* frames, int64_t n,
                             const zh_blosc_enc_params* params, unsigned flags, void* dst,
                             int64_t dstcap, void* stream_v, char* err, size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  if (!flags_ok(flags)) {
    for (int64_t i = 0; i < n && frames; i++) frames[i].status = ZH_EINVAL;
    put_err(err, errlen, kBadFlags);
    return ZH_EINVAL;
  }
  const int64_t bound = bound_of(frames, n, params);
  if (bound < 0) {
    for (int64_t i = 0; i < n && frames; i++) frames[i].status = ZH_EINVAL;
    put_err(err, errlen, kBadParams);
    return ZH_EINVAL;
  }
  if (bound > dstcap || (bound > 0 && !dst)) {
    put_err(err, errlen, "zh_blosc_encode_batch: destination smaller than zh_blosc_encode_bound");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;
  const zh_ze::Tables* dtab = (flags & ZH_BLOSC_ENC_ZSTD) ? device_tables(ctx) : nullptr;
  Ring ring;
  int rc = (flags & ZH_BLOSC_ENC_ZSTD) && !dtab ? ZH_ENOMEM : ring.init(ctx, s);
  int64_t pos = 0;
  double ms = 0, part[3] = {0, 0, 0};
  for (int64_t f0 = 0; f0 < n && rc == ZH_OK;) {
    const int64_t f1 = slab_end(frames, f0, n);
    auto slab = [&](auto coder) {
      return encode_slab(ctx, s, ring, frames, f0, f1, params, std::move(coder), (uint8_t*)dst,
                         &pos, &ms, part);
    };
    rc = (flags & ZH_BLOSC_ENC_ZLIB)   ? slab(ZlibDev{(flags & ZH_BLOSC_ENC_DYNAMIC) != 0})
         : (flags & ZH_BLOSC_ENC_ZSTD) ? slab(ZstdDev{dtab})
                                       : slab(Lz4Dev{});
    f0 = f1;
  }
  if (rc != ZH_OK) {
    (void)hipGetLastError();
    put_err(err, errlen, rc == ZH_ENOMEM ? "zh_blosc_encode_batch: out of device memory"
                                         : "zh_blosc_encode_batch: device copy or launch failed");
    return rc;
  }
  g_last_enc_ms.store(ms);
  if (flags & ZH_BLOSC_ENC_ZLIB)
    for (int k = 0; k < 3; k++) g_last_zlib_part[k].store(part[k]);
  return ZH_OK;
}

}  // extern "C"
