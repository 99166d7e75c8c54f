// zh_gzip_dec_kernels.hip — batched device decode of gzip members (zh_gzip_decode_batch).  The
// decoder is zh_gzip_dec.h, the same templates zh_gzip_decompress (zh_gzip.cpp) runs on one lane;
// that call has the status and text of a reason, and zh_gzip.cpp has the plan (the members'
// headers only).  The compressed bytes cross PCIe through the context's page-locked ring.
//   gzip_decode_kernel   one wave per member, kWaves members per workgroup, no workgroup barrier:
//           the blocks of a member share the 32 KiB window, so the member is the parallel unit.
//     tables   zh_gd::Work per wave in LDS (lookup tables of 2^10 and 2^8 x 2 B, the sorted
//              symbols, the counts, the code lengths: 3 928 B, 15 712 B a workgroup, so ten
//              workgroups fit the LDS of a CU).  The description of a dynamic block (a short
//              serial chain) is read on lane 0; the lookup tables are filled by the 64 lanes.
//     symbols  decoded wave-uniformly: every lane reads the same bit container (8 bytes per
//              refill, a broadcast load) and the same table entries, so nothing is exchanged.
//     literals lane k keeps the k-th literal of a run; a run is flushed with one coalesced store
//              when it reaches 64, before a match and at a block's end.
//     copies   match copies and stored-block copies go across the 64 lanes.
//     order    ZdLanes::order (zh_dec_lanes.h has the argument): before every match copy, which
//              reads bytes other lanes stored, and after every table build.
//     failure  the decoder's reason (zh_gd::Verdict, non-zero) goes to the member's flag with a
//              plain vector store.  The kernel also requires that the member produced the plan's
//              nbytes and ended with the frame, 8 bytes of trailer before srclen.
//   gzip_crc32_kernel (zh_gzip_enc_kernels.hip)  over the decoded members in spans of 64 KiB; the
//           host folds a member's spans and compares with the stored CRC-32.
//   host    flagged or mismatching members go through zh_gzip_decompress in batch order: a
//           failure is the call's status and text; a success is copied up and the frame's `where`
//           becomes 1; a success larger than the frame's slot is ZH_EUNSUPPORTED.
// Slabs of at most kSlabBytes of decoded bytes bound the device memory (the compressed bytes and
// small tables); a larger member is its own slab.
// Every DevFrame row is built on the host from checked sizes; the decoder checks every read
// against the member and every write against the room the plan gave it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "zh_ctx.h"
#include "zh_dec_lanes.h"
#include "zh_gzip_dec.h"
#include "zh_gzip_enc.h"
#include "zh_stager.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int64_t kSlabBytes = (int64_t)128 << 20;
constexpr int64_t kAlign = 256;
constexpr uint64_t kSpan = 64u << 10;  // bytes per job of the CRC kernel
constexpr const char* kOversize = "gzip: decoded size exceeds the planned size";
inline int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct DevFrame {
  int64_t src_off, srclen;  // in the staged compressed bytes
  int64_t dst_off, nbytes;  // in the batch destination
};
struct CrcJob {  // gzip_crc_launch's
  uint64_t src;
  uint32_t len, pad;
};

__global__ __launch_bounds__(kThreads) void gzip_decode_kernel(
    const uint8_t* __restrict__ src, uint8_t* dst, const DevFrame* __restrict__ frames,
    uint32_t nframes, uint32_t* __restrict__ flags) {
  __shared__ zh_gd::Work work[kWaves];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t f = blockIdx.x * kWaves + wave;
  if (f >= nframes) return;  // the whole wave: the kernel has no barrier
  const DevFrame r = frames[f];
  ZdLanes p;
  p.l = threadIdx.x & 63;
  uint64_t made = 0;
  size_t used = 0;
  uint32_t crc = 0;
  zh_gd::Verdict v = zh_gd::decode_member(src + r.src_off, (size_t)r.srclen, dst + r.dst_off,
                                          (uint64_t)r.nbytes, work[wave], p, &made, &used, &crc);
  // the plan's member: exactly nbytes of content, and nothing after its trailer
  if (!v && made != (uint64_t)r.nbytes) v = zh_gd::kSizeMismatch;
  if (!v && used != (size_t)r.srclen) v = zh_gd::kNotToTheEnd;
  if (p.l == 0) flags[f] = (uint32_t)v;
}

void put_err(char* err, size_t errlen, const char* msg) {
  if (err && errlen) {
    strncpy(err, msg, errlen - 1);
    err[errlen - 1] = 0;
  }
}

std::atomic<double> g_last_gdec_ms{-1.0};

// The device frames `ids` of one slab: upload, decode, hash; flags[i] != 0 afterwards for a
// member zh_gzip_decompress has to judge.
int decode_slab(zh_ctx* ctx, hipStream_t s, Stager& sg, const zh_gzip_frame* frames,
                const std::vector<int64_t>& ids, uint8_t* dst, std::vector<uint32_t>& flags,
                double* ms) {
  const size_t nf = ids.size();
  std::vector<DevFrame> rows(nf);
  std::vector<CrcJob> jobs;
  int64_t src_total = 0;
  for (size_t k = 0; k < nf; k++) {
    const zh_gzip_frame& f = frames[ids[k]];
    rows[k] = {src_total, f.srclen, f.dst_off, f.nbytes};
    src_total = up(src_total + f.srclen, 16);
    for (uint64_t o = 0; o < (uint64_t)f.nbytes; o += kSpan)
      jobs.push_back({(uint64_t)(uintptr_t)(dst + f.dst_off) + o,
                      (uint32_t)std::min<uint64_t>(kSpan, (uint64_t)f.nbytes - o), 0});
  }
  if (jobs.size() > (size_t)zh::kIntMax) return ZH_EINVAL;
  // device memory: [rows | flags | crc jobs | crc registers | compressed bytes]
  const size_t o_flags = (size_t)up((int64_t)(nf * sizeof(DevFrame)), 256);
  const size_t o_jobs = o_flags + (size_t)up((int64_t)nf * 4, 256);
  const size_t o_raw = o_jobs + (size_t)up((int64_t)(jobs.size() * sizeof(CrcJob)), 256);
  const size_t o_src = o_raw + (size_t)up((int64_t)jobs.size() * 4, 256);
  const size_t need = o_src + (size_t)src_total + 256;
  void* dmem = nullptr;
  size_t got = 0;
  if (zh::ctx_alloc(ctx, need, &dmem, &got) != hipSuccess) {
    (void)hipGetLastError();
    return ZH_ENOMEM;
  }
  uint8_t* d8 = (uint8_t*)dmem;
  std::vector<uint32_t> fl(nf, 1u);  // a member whose wave never ran stays flagged
  std::vector<uint32_t> raw(jobs.size(), 0);
  sg.begin(d8);
  sg.append((const uint8_t*)rows.data(), nf * sizeof(DevFrame));
  sg.skip(o_flags - nf * sizeof(DevFrame));
  sg.append((const uint8_t*)fl.data(), nf * 4);
  sg.skip(o_jobs - o_flags - nf * 4);
  sg.append((const uint8_t*)jobs.data(), jobs.size() * sizeof(CrcJob));
  sg.skip(o_src - o_jobs - jobs.size() * sizeof(CrcJob));
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
  hipLaunchKernelGGL(gzip_decode_kernel, dim3((unsigned)((nf + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, s, d8 + o_src, dst, (const DevFrame*)d8, (uint32_t)nf,
                     (uint32_t*)(d8 + o_flags));
  if (hipGetLastError() != hipSuccess || sg.failed) rc = ZH_EHIP;
  if (rc == ZH_OK)
    rc = zh::gzip_crc_launch(s, d8 + o_jobs, (uint32_t)jobs.size(), (uint32_t*)(d8 + o_raw));
  if (ev[1]) (void)hipEventRecord(ev[1], s);
  if (rc == ZH_OK &&
      (hipMemcpyAsync(fl.data(), d8 + o_flags, nf * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (!jobs.empty() && hipMemcpyAsync(raw.data(), d8 + o_raw, jobs.size() * 4,
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
  // the spans of a member folded, against the CRC-32 in front of its last four bytes
  const uint32_t x_span = zh_gz::xpow8(kSpan);
  size_t j = 0;
  for (size_t k = 0; k < nf; k++) {
    const zh_gzip_frame& f = frames[ids[k]];
    uint32_t r = 0;
    for (uint64_t o = 0; o < (uint64_t)f.nbytes; o += kSpan, j++)
      r = zh_gz::crc_append(r, raw[j], jobs[j].len == kSpan ? x_span : zh_gz::xpow8(jobs[j].len));
    const uint32_t want = zh_gd::rd_le((const uint8_t*)f.src + f.srclen - 8, 4);
    if (!fl[k] && zh_gz::crc_finish(r, (uint64_t)f.nbytes) != want) fl[k] = zh_gd::kCrcMismatch;
  }
  for (size_t k = 0; k < nf; k++) flags[(size_t)ids[k]] = fl[k];
  return ZH_OK;
}

}  // namespace

extern "C" {

double zh_debug_gzip_decode_kernel_ms(void) { return g_last_gdec_ms.load(); }

int zh_gzip_decode_batch(zh_ctx* ctx, zh_gzip_frame* frames, int64_t n, void* dst, int64_t dstcap,
                         void* stream_v, char* err, size_t errlen) {
  if (!ctx) return ZH_EINVAL;
  int64_t total = 0;
  int st = zh::gzip_plan(frames, n, &total, err, errlen);
  if (st != ZH_OK) return st;
  if (total > dstcap || (total > 0 && !dst)) {
    put_err(err, errlen, "gzip destination too small");
    return ZH_EINVAL;
  }
  if (n == 0) return ZH_OK;
  if (n > zh::kIntMax) {
    put_err(err, errlen, "zh_gzip_decode_batch: too many frames in one batch");
    return ZH_EINVAL;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_v ? (hipStream_t)stream_v : ctx->stream;
  Stager sg;
  int rc = sg.init(ctx, s);
  std::vector<uint32_t> flags((size_t)n, 0);  // set: zh_gzip_decompress names the verdict
  std::vector<uint8_t> hostbuf;
  double ms = 0;
  // host-decoded frames: zh_gzip_decompress, then one copy
  for (int64_t i = 0; i < n && rc == ZH_OK; i++) {
    zh_gzip_frame& f = frames[i];
    if (f.where != 1) continue;
    hostbuf.resize(std::max<size_t>(1, (size_t)f.nbytes));
    size_t nb = 0;
    char msg[256] = "";
    f.status = zh_gzip_decompress(f.src, (size_t)f.srclen, hostbuf.data(), (size_t)f.nbytes, &nb,
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
      rc = decode_slab(ctx, s, sg, frames, ids, (uint8_t*)dst, flags, &ms);
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
    put_err(err, errlen, rc == ZH_ENOMEM   ? "zh_gzip_decode_batch: out of device memory"
                         : rc == ZH_EINVAL ? "zh_gzip_decode_batch: too many spans in a slab"
                                           : "zh_gzip_decode_batch: device copy or launch failed");
    return rc;
  }
  g_last_gdec_ms.store(ms);
  // flagged frames in batch order: zh_gzip_decompress's status and text, or its bytes
  bool oversize = false;
  for (int64_t i = 0; i < n; i++) {
    zh_gzip_frame& f = frames[i];
    if (!flags[(size_t)i]) continue;
    size_t nb = 0;
    char msg[256] = "";
    int hs = zh_gzip_decompress(f.src, (size_t)f.srclen, nullptr, 0, &nb, msg, sizeof msg);
    const size_t slot = (size_t)up(f.nbytes, kAlign);
    if (hs == ZH_OK && nb > slot) {  // the last four bytes were not this member's size
      f.status = ZH_EUNSUPPORTED;
      oversize = true;
      continue;
    }
    if (hs == ZH_OK) {
      hostbuf.resize(std::max<size_t>(1, nb));
      hs = zh_gzip_decompress(f.src, (size_t)f.srclen, hostbuf.data(), nb, &nb, msg, sizeof msg);
    }
    f.status = hs;
    if (hs != ZH_OK) {
      put_err(err, errlen, msg);
      return hs;
    }
    // the wave refused what one lane accepts: the host's bytes, and the frame says so
    if (nb && hipMemcpy((uint8_t*)dst + f.dst_off, hostbuf.data(), nb, hipMemcpyHostToDevice) !=
                  hipSuccess) {
      put_err(err, errlen, "zh_gzip_decode_batch: device copy or launch failed");
      return ZH_EHIP;
    }
    f.nbytes = (int64_t)nb;
    f.where = 1;
  }
  if (oversize) {
    put_err(err, errlen, kOversize);
    return ZH_EUNSUPPORTED;
  }
  return ZH_OK;
}

}  // extern "C"
