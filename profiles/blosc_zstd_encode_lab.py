"""Blosc frames with zstd streams written on the device (ZH_BLOSC_ZSTD_ENCODE=1), at a user's size.

Data: the two seeded uint16 arrays of profiles/zstd_encode_lab.py (the noisy image and the label
image), 2 GiB each, 256 chunks of 8 MiB, declared [bytes little, blosc zstd byte shuffle] on a
FilesystemStore on tmpfs.

Routes, alternating in one process, one warm-up and 5 repeats each:
  (a) memcpyed  the switch unset: MEMCPYED frames, the behaviour before the writer existed;
  (b) device    ZH_BLOSC_ZSTD_ENCODE=1: zh_blosc_encode_batch_ex with ZH_BLOSC_ENC_ZSTD;
  (c) host      the same with ZH_BLOSC_ENCODE_DEVICE=0: zh_blosc_compress_ex per chunk.
Recorded per array and route: median, min-max spread, stored over raw size, last_write_info; then
  * the kernels of the batch by device events (zh_debug_blosc_encode_kernel_ms) over 64 chunks
    resident on the device (512 MiB), GiB/s of raw input, per block-size candidate;
  * the stored size of the first SPLIT_SAMPLE_CHUNKS chunks with the split rule of the writer
    (one stream per byte plane of a block) and without it (one stream per block, as c-blosc does
    for zstd), both from zh_zstd_compress on the byte-shuffled streams: no knob of the library.

    python profiles/blosc_zstd_encode_lab.py [--gib 2] [--repeats 5] [--host-repeats 5]
                                             [--out profiles/blosc_zstd_encode/lab.json]
    python profiles/blosc_zstd_encode_lab.py --write-only --tree <checkout> --out <json>
        route (a) alone with another checkout's package (the parent commit:
        profiles/blosc_zstd_encode/parent_write.json)

The switch stays opt-in whatever the times say: it changes stored bytes ("Blosc zstd
frames encoded on the device")."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

from zstd_encode_lab import CHUNK, DATASETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES = (16 << 10, 32 << 10, 64 << 10)
SPLIT_SAMPLE_CHUNKS = 2       # the host form of the zstd writer is slow
ROUTES = {"memcpyed": {},
          "device": {"ZH_BLOSC_ZSTD_ENCODE": "1", "ZH_BLOSC_ENCODE_DEVICE": "1"},
          "host": {"ZH_BLOSC_ZSTD_ENCODE": "1", "ZH_BLOSC_ENCODE_DEVICE": "0"}}
SWITCHES = ("ZH_BLOSC_ZSTD_ENCODE", "ZH_BLOSC_ENCODE_DEVICE")


def spread(xs):
    return max(xs) - min(xs)


def set_route(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=None,
                    help="repeats of route (c), when fewer than --repeats (it is slow)")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "blosc_zstd_encode", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--write-only", action="store_true", help="route (a) alone")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z

    routes = ["memcpyed"] if a.write_only else list(ROUTES)
    reps = {r: a.repeats for r in routes}
    if a.host_repeats is not None and "host" in reps:
        reps["host"] = min(a.repeats, a.host_repeats)
    nchunks = max(1, int(a.gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))
    rec = {"chunks": nchunks, "chunk_bytes": CHUNK[0] * CHUNK[1] * 2, "tmpfs": bool(a.tmp),
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)", "repeats": reps, "arrays": {}}
    data = np.empty((nchunks * CHUNK[0], CHUNK[1]), np.uint16)
    for name, make in DATASETS.items():
        for k in range(nchunks):
            data[k * CHUNK[0]:(k + 1) * CHUNK[0]] = make(k)
        r = rec["arrays"][name] = {"raw_bytes": data.nbytes, "routes": {}}
        root = tempfile.mkdtemp(prefix="zh_blosc_zstd_enc_lab_", dir=a.tmp)
        try:
            meta = (z.ArrayMetadataBuilder().withShape(*data.shape).withChunkShape(*CHUNK)
                    .withDataType(z.DataType.UINT16).withFillValue(0)
                    .withCodecs(lambda c: c.withBytes("LITTLE").withBlosc("zstd", "shuffle"))
                    .build())
            arrs = {rt: z.Array.create(z.FilesystemStore(os.path.join(root, rt)).resolve(name),
                                       meta) for rt in routes}
            times = {rt: [] for rt in routes}
            for rep in range(-1, a.repeats):       # -1: the warm-up; the routes alternate
                for rt in routes:
                    if rep >= reps[rt]:
                        continue
                    set_route(ROUTES[rt])
                    t = time.perf_counter()
                    arrs[rt].write(None, data)
                    dt = time.perf_counter() - t
                    if rep >= 0:
                        times[rt].append(dt)
                    print(name, rt, "write rep", rep, round(dt * 1e3, 1), "ms", flush=True)
            for rt in routes:
                set_route(ROUTES[rt])
                stored = sum(os.path.getsize(os.path.join(dp, f))
                             for dp, _, fs in os.walk(os.path.join(root, rt))
                             for f in fs if not f.startswith(".") and f != "zarr.json")
                ts = times[rt]
                r["routes"][rt] = {
                    "env": ROUTES[rt], "ms": [round(x * 1e3, 2) for x in ts],
                    "median_ms": round(statistics.median(ts) * 1e3, 2),
                    "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2),
                    "spread_ms": round(spread(ts) * 1e3, 2),
                    "raw_GiB_per_s": round(data.nbytes / (1 << 30) / statistics.median(ts), 3),
                    "stored_bytes": stored, "stored_over_raw": round(stored / data.nbytes, 4),
                    "info": getattr(arrs[rt], "last_write_info", None)}
                back = z.Array.open(arrs[rt].storeHandle).read([0, 0], list(CHUNK))
                assert np.array_equal(back, data[:CHUNK[0]]), "the array does not read back"
            if not a.write_only:
                dv, mc, ho = (r["routes"][k] for k in ("device", "memcpyed", "host"))
                r["verdict"] = verdict(dv, mc, ho)
                set_route({})
                r["kernels"] = kernel_rates(data, a.repeats)
                r["split"] = split_sizes(data)
        finally:
            set_route({})
            shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


def verdict(dv, mc, ho):
    """The rule DESIGN.md applies to ZH_BLOSC_DEVICE: (b) beats a route when its median is lower
    by more than the larger of the two min-max spreads."""
    def beats(other):
        margin = max(dv["spread_ms"], other["spread_ms"])
        return {"median_gain_ms": round(other["median_ms"] - dv["median_ms"], 2),
                "margin_ms": margin, "beats": other["median_ms"] - dv["median_ms"] > margin}
    return {"device_vs_memcpyed": beats(mc), "device_vs_host": beats(ho)}


def kernel_rates(data, repeats, nchunks=64):
    """The kernels of zh_blosc_encode_batch_ex with ZH_BLOSC_ENC_ZSTD (device events) over chunks
    resident on the device, one frame per chunk, and the stored size, per block-size candidate."""
    from zarrhip import _lib
    from zarrhip.array import device
    dev, L, out = device(), _lib.lib(), {}
    nchunks = min(nchunks, data.shape[0] // CHUNK[0])
    cb = CHUNK[0] * CHUNK[1] * 2
    ptr = dev.malloc(nchunks * cb)
    try:
        dev.memcpy(ptr, data.ctypes.data, nchunks * cb, 0)
        srcs = [(ptr + k * cb, cb) for k in range(nchunks)]
        for bs in CANDIDATES:
            ms, t_call = [], []
            for rep in range(-1, repeats):
                t = time.perf_counter()
                _, rows = dev.blosc_encode_batch_raw(srcs, 2, 1, bs, zstd=True)
                dt = time.perf_counter() - t
                if rep >= 0:
                    ms.append(L.zh_debug_blosc_encode_kernel_ms())
                    t_call.append(dt * 1e3)
            stored = sum(n for _, n in rows)
            out[str(bs)] = {"raw_bytes": nchunks * cb, "stored_bytes": stored,
                            "stored_over_raw": round(stored / (nchunks * cb), 4),
                            "kernel_ms": [round(x, 3) for x in ms],
                            "call_ms": [round(x, 2) for x in t_call],
                            "raw_GiB_per_s": round(nchunks * cb / (1 << 30) /
                                                   (statistics.median(ms) / 1e3), 2)}
            print("kernels", bs, out[str(bs)], flush=True)
    finally:
        dev.free(ptr)
    return out


def split_sizes(data, nchunks=SPLIT_SAMPLE_CHUNKS, bs=16 << 10):
    """Stored bytes of the first chunks' streams (csize word and payload, zstd or raw) at the
    default block size: one stream per byte plane (the writer's split rule) against one stream
    per block."""
    from zarrhip import _lib

    def stored(s):
        return 4 + min(len(s), len(_lib.zstd_compress(s, False, 64 << 10)))
    split = whole = raw = 0
    for k in range(min(nchunks, data.shape[0] // CHUNK[0])):
        b = np.frombuffer(data[k * CHUNK[0]:(k + 1) * CHUNK[0]].tobytes(), np.uint8)
        for blk in b.reshape(-1, bs // 2, 2):
            planes = np.ascontiguousarray(blk.T)
            split += sum(stored(planes[j].tobytes()) for j in range(2))
            whole += stored(planes.tobytes())
        raw += b.size
    out = {"chunks": nchunks, "blocksize": bs, "raw_bytes": raw, "split_stream_bytes": split,
           "unsplit_stream_bytes": whole, "split_over_raw": round(split / raw, 4),
           "unsplit_over_raw": round(whole / raw, 4)}
    print("split", out, flush=True)
    return out


if __name__ == "__main__":
    main()
