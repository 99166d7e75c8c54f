// zh_stager.h — the upload lane of the batched frame decoders (zh_blosc_kernels.hip,
// zh_zstd_dec_kernels.hip).  Included by .hip files only, each of which gets its own copy
// (anonymous namespace).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "zh_ctx.h"

namespace {

// Page-locked ring of the context as a staging lane for one stream: `append` packs bytes bound
// for consecutive device addresses into the current slot, `copy` sends one host range.  A slot
// is reused once the copy that read it has finished.
struct Stager {
  zh_ctx* ctx;
  hipStream_t s;
  std::vector<hipEvent_t> ev;
  std::vector<char> busy;
  size_t slot_bytes = 0, fill = 0;
  int cur = 0;
  uint8_t* ddst = nullptr;  // device address of byte 0 of the current slot
  bool failed = false;

  int init(zh_ctx* c, hipStream_t st) {
    ctx = c;
    s = st;
    int lanes;
    int64_t window;
    int rc = zh::pipe_out_ring(ctx, &lanes, &window);
    if (rc != ZH_OK) return rc;
    slot_bytes = (size_t)window;
    ev.assign(ctx->ring_in.size(), nullptr);
    busy.assign(ctx->ring_in.size(), 0);
    for (auto& e : ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ZH_EHIP;
    return ZH_OK;
  }
  ~Stager() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  uint8_t* slot() {
    if (busy[cur]) {
      if (hipEventSynchronize(ev[cur]) != hipSuccess) failed = true;
      busy[cur] = 0;
    }
    return (uint8_t*)ctx->ring_in[(size_t)cur];
  }
  void send(uint8_t* d, size_t n) {  // the first n bytes of the current slot -> d
    if (n) {
      if (hipMemcpyAsync(d, ctx->ring_in[(size_t)cur], n, hipMemcpyHostToDevice, s) !=
              hipSuccess ||
          hipEventRecord(ev[cur], s) != hipSuccess)
        failed = true;
      busy[cur] = 1;
    }
    cur = (cur + 1) % (int)ev.size();
  }
  void begin(uint8_t* d) {
    ddst = d;
    fill = 0;
  }
  void append(const uint8_t* h, size_t n) {
    while (n) {
      uint8_t* sl = slot();
      const size_t take = std::min(n, slot_bytes - fill);
      memcpy(sl + fill, h, take);
      fill += take;
      h += take;
      n -= take;
      if (fill == slot_bytes) flush();
    }
  }
  void skip(size_t n) {  // padding between frames (its bytes are never read)
    while (n) {
      (void)slot();
      const size_t take = std::min(n, slot_bytes - fill);
      fill += take;
      n -= take;
      if (fill == slot_bytes) flush();
    }
  }
  void flush() {
    const size_t n = fill;
    send(ddst, n);
    ddst += n;
    fill = 0;
  }
  void copy(uint8_t* d, const uint8_t* h, size_t n) {
    while (n) {
      uint8_t* sl = slot();
      const size_t take = std::min(n, slot_bytes);
      memcpy(sl, h, take);
      send(d, take);
      d += take;
      h += take;
      n -= take;
    }
  }
};

}  // namespace
