// zh_zstd_dec_kernels.hip — batched device decode of zstd frames (zh_zstd_batch_plan /
// zh_zstd_decode_batch / zh_debug_zstd_blocks).  The decoder is zh_zstd_dec.h, the same templates
// zh_zstd_decompress (zh_zstd.cpp) runs on one lane; that call has the status and text of a reason.
//
// The host walks every frame's headers once (zh_zd::walk_frame: no entropy decoding).  A single
// frame with a content size, no dictionary and a block chain that ends exactly at its last byte
// is decoded here; everything else is decoded by zh_zstd_decompress inside the call and copied
// up.  The compressed bytes cross PCIe through the context's page-locked ring.
//   zstd_decode_kernel   one wave per frame, kWaves frames per workgroup, no workgroup barrier:
//           blocks of a frame depend on each other (window, repeat offsets, repeated tables), so
//           the frame is the parallel unit.
//     tables   zh_zd::Work per wave in LDS (Huffman 2^11 x 2 B, LL / ML 2^9 x 4 B, OF 2^8 x 4 B
//              and what the builds need).  Table descriptions and the FSE spreading run on lane 0;
//              the Huffman table is filled by the 64 lanes.
//     literals Huffman literals decode into the frame's literal scratch in global memory (the
//              largest regen the plan found), the four streams on four lanes; raw literals are
//              read in place; RLE literals are a byte.
//     sequences decoded wave-uniformly: every lane reads the same backwards bit container (8
//              bytes per refill, a broadcast load) and the same table entries, so the sequence
//              values are uniform without any exchange; literal and match copies go across the
//              64 lanes.  The simple form: one sequence at a time (no look-ahead batching of
//              literal copies; no A/B of that was run).
//     order    a match reads bytes that other lanes of the same wave stored earlier, in the
//              destination in global memory; Huffman literals are read by other lanes than wrote
//              them; the tables in LDS likewise.  ZdLanes::order is WaveCopy::order of
//              zh_blosc_kernels.hip and the argument is the one in that file's header ("order":
//              the wave's own stores have reached the CU's L1 / L2 when vmcnt returns to 0, LDS
//              operations of a wave complete in order).  It stands before every match copy and
//              after every serial or parallel table / literal step.
//     failure  the decoder's reason (zh_zd::Verdict, non-zero) goes to the frame's flag (plain
//              vector store).
//   zstd_xxh64_kernel (zh_zstd_enc_kernels.hip)  over the decoded frames that carry a checksum;
//           the host compares the low 32 bits with the stored field.
//   host    flagged or mismatching frames go through zh_zstd_decompress in batch order (the flag's
//           reason is not used yet): a failure is the call's status and text; a success is copied
//           up and the frame's `where` becomes 1.
// Slabs of at most kSlabBytes of decoded bytes bound the device memory (compressed bytes, literal
// scratch <= the decoded bytes, small tables); a larger frame is its own slab.
// Every DevFrame row is built on the host from checked sizes; the decoder checks every read
// against the frame and every write against the room the plan gave it and its literal scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "zh_ctx.h"
#include "zh_dec_lanes.h"
#include "zh_stager.h"
#include "zh_zstd_dec.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int64_t kSlabBytes = (int64_t)128 << 20;
constexpr int64_t kAlign = 256;
inline int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct DevFrame {
  int64_t src_off, srclen;  // in the staged compressed bytes
  int64_t dst_off, nbytes;  // in the batch destination
  int64_t lit_off, litcap;  // in the literal scratch
};
struct HashJob {  // zstd_xxh64_kernel's
  uint64_t src, n;
};

// The lane policy of zh_zstd_dec.h for one wave: ZdLanes (zh_dec_lanes.h).

__global__ __launch_bounds__(kThreads) void zstd_decode_kernel(
    const uint8_t* __restrict__ src, uint8_t* dst, uint8_t* lit,
    const DevFrame* __restrict__ frames, uint32_t nframes, uint32_t* __restrict__ flags) {
  __shared__ zh_zd::Work work[kWaves];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t f = blockIdx.x * kWaves + wave;
  if (f >= nframes) return;  // the whole wave: the kernel has no barrier
  const DevFrame r = frames[f];
  ZdLanes p;
  p.l = threadIdx.x & 63;
  zh_zd::Header h;
  uint64_t made = 0;
  size_t used = 0;
  zh_zd::Verdict v = zh_zd::decode_frame(src + r.src_off, (size_t)r.srclen, dst + r.dst_off,
                                         (uint64_t)r.nbytes, lit + r.lit_off, (uint64_t)r.litcap,
                                         work[wave], p, &made, &used, &h);
  // the plan's frame: exactly nbytes of content, and nothing after it
  if (!v && made != (uint64_t)r.nbytes) v = zh_zd::kSizeMismatch;
  if (!v && used != (size_t)r.srclen) v = zh_zd::kTrailingBytes;
  if (p.l == 0) flags[f] = (uint32_t)v;
}

void put_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) {
    strncpy(err, msg, errlen - 1);
    err[errlen - 1] = 0;
  }
}

std::atomic<double> g_last_zdec_ms{-1.0};

int plan_frames(zh_zstd_frame* frames, int64_t n, std::vector<zh_zd::Walk>* walks, int64_t* total,
                char* err, size_t errlen) {
  if (n < 0 || (n > 0 && !frames)) {
    put_err(err, errlen, "zh_zstd_batch_plan: no frames");
    return ZH_EINVAL;
  }
  int64_t pos = 0;
  if (walks) walks->assign((size_t)n, zh_zd::Walk());
  for (int64_t i = 0; i < n; i++) {
    zh_zstd_frame& f = frames[i];
    char msg[256] = "";
    size_t nb = 0;
    int st = ZH_EINVAL;
    if (f.srclen >= 0 && (f.src || f.srclen == 0)) {
      static const uint8_t none = 0;
      st = zh_zstd_decompress(f.src ? f.src : &none, (size_t)f.srclen, nullptr, 0, &nb, msg,
                              sizeof msg);
    } else {
      snprintf(msg, sizeof msg, "zh_zstd_batch_plan: negative frame length");
    }
    if (st == ZH_OK && nb > ((size_t)1 << 62)) {
      st = ZH_EDATA;
      snprintf(msg, sizeof msg, "zstd: frame content size mismatch");
    }
    f.status = st;
    if (st != ZH_OK) {
      put_err(err, errlen, msg);
      return st;
    }
    const zh_zd::Walk w =
        zh_zd::walk_frame<zh_zd::NoRows>((const uint8_t*)f.src, (size_t)f.srclen, nullptr);
    f.dst_off = pos;
    f.nbytes = (int64_t)nb;
    f.where = w.device && w.fcs == (int64_t)nb ? 0 : 1;
    if (walks) (*walks)[(size_t)i] = w;
    pos = up(pos + f.nbytes, kAlign);
  }
  *total = pos;
  return ZH_OK;
}

// The device frames [f0, f1) of one slab: upload, decode, hash; flags[i] != 0 afterwards for a
// frame zh_zstd_decompress has to judge.
int decode_slab(zh_ctx* ctx, hipStream_t s, Stager& sg, const zh_zstd_frame* frames,
                const std::vector<zh_zd::Walk>& walks, const std::vector<int64_t>& ids,
                uint8_t* dst, std::vector<uint32_t>& flags, double* ms) {
  const size_t nf = ids.size();
  std::vector<DevFrame> rows(nf);
  std::vector<HashJob> jobs;
  std::vector<size_t> job_frame;
  int64_t src_total = 0, lit_total = 0;
  for (size_t k = 0; k < nf; k++) {
    const zh_zstd_frame& f = frames[ids[k]];
    const zh_zd::Walk& w = walks[(size_t)ids[k]];
    rows[k] = {src_total, f.srclen, f.dst_off, f.nbytes, lit_total, w.max_regen};
    src_total = up(src_total + f.srclen, 16);
    lit_total = up(lit_total + w.max_regen, 16);
    if (w.csum) {
      jobs.push_back({(uint64_t)(uintptr_t)(dst + f.dst_off), (uint64_t)f.nbytes});
      job_frame.push_back(k);
    }
  }
  // device memory: [rows | flags | hash jobs | hashes | compressed bytes | literal scratch]
  const size_t o_flags = (size_t)up((int64_t)(nf * sizeof(DevFrame)), 256);
  const size_t o_jobs = o_flags + (size_t)up((int64_t)nf * 4, 256);
  const size_t o_hashes = o_jobs + (size_t)up((int64_t)(jobs.size() * sizeof(HashJob)), 256);
  const size_t o_src = o_hashes + (size_t)up((int64_t)jobs.size() * 8, 256);
  const size_t o_lit = o_src + (size_t)up(src_total, 256);
  const size_t need = o_lit + (size_t)lit_total + 256;
  void* dmem = nullptr;
  size_t got = 0;
  if (zh::ctx_alloc(ctx, need, &dmem, &got) != hipSuccess) {
    (void)hipGetLastError();
    return ZH_ENOMEM;
  }
  uint8_t* d8 = (uint8_t*)dmem;
  std::vector<uint32_t> fl(nf, 1u);  // a frame whose wave never ran stays flagged
  std::vector<uint64_t> hashes(jobs.size(), 0);
  sg.begin(d8);
  sg.append((const uint8_t*)rows.data(), nf * sizeof(DevFrame));
  sg.skip(o_flags - nf * sizeof(DevFrame));
  sg.append((const uint8_t*)fl.data(), nf * 4);
  sg.skip(o_jobs - o_flags - nf * 4);
  sg.append((const uint8_t*)jobs.data(), jobs.size() * sizeof(HashJob));
  sg.skip(o_src - o_jobs - jobs.size() * sizeof(HashJob));
  int64_t pos = 0;
  for (size_t k = 0; k < nf; k++) {
    sg.skip((size_t)(rows[k].src_off - pos));
    sg.append((const uint8_t*)frames[ids[k]].src, (size_t)rows[k].srclen);
    pos = rows[k].src_off + rows[k].srclen;
  }
  sg.flush();
  int rc = ZH_OK;
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (auto& e : ev) (void)hipEventCreate(&e);
  if (ev[0]) (void)hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(zstd_decode_kernel, dim3((unsigned)((nf + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, s, d8 + o_src, dst, d8 + o_lit, (const DevFrame*)d8,
                     (uint32_t)nf, (uint32_t*)(d8 + o_flags));
  if (hipGetLastError() != hipSuccess || sg.failed) rc = ZH_EHIP;
  if (rc == ZH_OK && !jobs.empty())
    rc = zh::zstd_hash_launch(s, d8 + o_jobs, (uint32_t)jobs.size(), (uint64_t*)(d8 + o_hashes));
  if (ev[1]) (void)hipEventRecord(ev[1], s);
  if (rc == ZH_OK &&
      (hipMemcpyAsync(fl.data(), d8 + o_flags, nf * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (!jobs.empty() && hipMemcpyAsync(hashes.data(), d8 + o_hashes, jobs.size() * 8,
                                        hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = ZH_EHIP;
  if (hipStreamSynchronize(s) != hipSuccess) rc = rc == ZH_OK ? ZH_EHIP : rc;
  float kms = 0;
  if (rc == ZH_OK && ev[0] && ev[1] && hipEventElapsedTime(&kms, ev[0], ev[1]) == hipSuccess)
    *ms += (double)kms;
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  zh::ctx_release(ctx, dmem, got);
  if (rc != ZH_OK) return rc;
  for (size_t j = 0; j < jobs.size(); j++)
    if ((uint32_t)hashes[j] != walks[(size_t)ids[job_frame[j]]].want)
      fl[job_frame[j]] = zh_zd::kChecksumMismatch;
  for (size_t k = 0; k < nf; k++) flags[(size_t)ids[k]] = fl[k];
  return ZH_OK;
}

}  // namespace

extern "C" {

int64_t zh_zstd_batch_plan(zh_zstd_frame* frames, int64_t n, char* err, size_t errlen) {
  int64_t total = 0;
  const int st = plan_frames(frames, n, nullptr, &total, err, errlen);
  return st == ZH_OK ? total : -(int64_t)st;
}

double zh_debug_zstd_decode_kernel_ms(void) { return g_last_zdec_ms.load(); }

int64_t zh_debug_zstd_blocks(const void* src, size_t srclen, int64_t* rows, int64_t cap, char* err,
                             size_t errlen) {
  if (!src && srclen) return -(int64_t)ZH_EINVAL;
  std::vector<zh_zd::BlockInfo> blocks;
  static const uint8_t none = 0;
  const zh_zd::Walk w = zh_zd::walk_frame(src ? (const uint8_t*)src : &none, srclen, &blocks);
  if (!w.device) {
    put_err(err, errlen, "zstd frame is decoded on the host: it is not one plain frame");
    return -(int64_t)ZH_EUNSUPPORTED;
  }
  // rows of 10 int64: type, stored size, decoded size (-1: a compressed block), literals type,
  // Huffman streams, regen, nseq, LL / OF / ML mode (-1 where the block has none)
  for (size_t k = 0; k < blocks.size() && rows && (int64_t)k < cap; k++) {
    const zh_zd::BlockInfo& b = blocks[k];
    const int64_t v[10] = {b.type, b.stored, b.decoded, b.lit_type, b.streams,
                           b.regen, b.nseq, b.ll_mode, b.of_mode, b.ml_mode};
    memcpy(rows + 10 * k, v, sizeof v);
  }
  return (int64_t)blocks.size();
}

int zh_zstd_decode_batch(zh_ctx* ctx, zh_zstd_frame* frames, int64_t n, void* dst, int64_t dstcap,
                         void* stream_v, char* err, size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  int64_t total = 0;
  std::vector<zh_zd::Walk> walks;
  int st = plan_frames(frames, n, &walks, &total, err, errlen);
  if (st != ZH_OK) return st;
  if (total > dstcap || (total > 0 && !dst)) {
    put_err(err, errlen, "zstd destination too small");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  if (n > zh::kIntMax) {
    put_err(err, errlen, "zh_zstd_decode_batch: too many frames in one batch");
    return ZH_EINVAL;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;
  Stager sg;
  int rc = sg.init(ctx, s);
  std::vector<uint32_t> flags((size_t)n, 0);  // set: zh_zstd_decompress names the verdict
  std::vector<uint8_t> hostbuf;
  double ms = 0;
  // host-decoded frames: zh_zstd_decompress, then one copy
  for (int64_t i = 0; i < n && rc == ZH_OK; i++) {
    zh_zstd_frame& f = frames[i];
    if (f.where != 1) continue;
    hostbuf.resize(std::max<size_t>(1, (size_t)f.nbytes));
    size_t nb = 0;
    char msg[256] = "";
    f.status = zh_zstd_decompress(f.src, (size_t)f.srclen, hostbuf.data(), (size_t)f.nbytes, &nb,
                                  msg, sizeof msg);
    if (f.status != ZH_OK) {
      flags[(size_t)i] = 1;
      continue;
    }
    sg.copy((uint8_t*)dst + f.dst_off, hostbuf.data(), (size_t)f.nbytes);
  }
  // device frames, a slab at a time
  std::vector<int64_t> ids;
  int64_t raw = 0;
  for (int64_t i = 0; i <= n && rc == ZH_OK; i++) {
    const bool dev = i < n && frames[i].where == 0;
    if (!ids.empty() && (i == n || (dev && raw + frames[i].nbytes > kSlabBytes))) {
      rc = decode_slab(ctx, s, sg, frames, walks, ids, (uint8_t*)dst, flags, &ms);
      ids.clear();
      raw = 0;
    }
    if (dev) {
      ids.push_back(i);
      raw += frames[i].nbytes;
    }
  }
  if (hipStreamSynchronize(s) != hipSuccess || sg.failed) rc = rc == ZH_OK ? ZH_EHIP : rc;
  if (rc != ZH_OK) {
    (void)hipGetLastError();
    put_err(err, errlen, rc == ZH_ENOMEM ? "zh_zstd_decode_batch: out of device memory"
                                         : "zh_zstd_decode_batch: device copy or launch failed");
    return rc;
  }
  g_last_zdec_ms.store(ms);
  // flagged frames in batch order: zh_zstd_decompress's status and text, or its bytes
  for (int64_t i = 0; i < n; i++) {
    zh_zstd_frame& f = frames[i];
    if (!flags[(size_t)i]) continue;
    hostbuf.resize(std::max<size_t>(1, (size_t)f.nbytes));
    size_t nb = 0;
    char msg[256] = "";
    const int hs = zh_zstd_decompress(f.src, (size_t)f.srclen, hostbuf.data(), (size_t)f.nbytes,
                                      &nb, msg, sizeof msg);
    f.status = hs;
    if (hs != ZH_OK) {
      put_err(err, errlen, msg);
      return hs;
    }
    // the wave refused what one lane accepts: the host's bytes, and the frame says so
    if (hipMemcpy((uint8_t*)dst + f.dst_off, hostbuf.data(), (size_t)f.nbytes,
                  hipMemcpyHostToDevice) != hipSuccess) {
      put_err(err, errlen, "zh_zstd_decode_batch: device copy or launch failed");
      return ZH_EHIP;
    }
    f.where = 1;
  }
  return ZH_OK;
}

}  // extern "C"
