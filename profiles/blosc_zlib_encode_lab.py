"""Blosc frames with zlib streams written on the device (ZH_BLOSC_ZLIB_ENCODE=1 or 2), at a user's
size.

Data: the two seeded uint16 arrays of profiles/zstd_encode_lab.py (the noisy image and the label
image), 2 GiB each, declared [bytes little, blosc zlib byte shuffle] on a FilesystemStore on tmpfs,
once as 256 chunks of 8 MiB and once as 32 768 chunks of 64 KiB.

Routes, alternating in one process, one warm-up and --repeats timed writes each (the host routes:
--host-repeats, without a warm-up: they take seconds, and nothing of them is lazily created):
  memcpyed  the switch unset: MEMCPYED frames, the behaviour before the writer existed;
  device1   ZH_BLOSC_ZLIB_ENCODE=1: zh_blosc_encode_batch_ex with ZH_BLOSC_ENC_ZLIB;
  device2   ZH_BLOSC_ZLIB_ENCODE=2: with ZH_BLOSC_ENC_DYNAMIC as well;
  host1, host2   the same with ZH_BLOSC_ENCODE_DEVICE=0: zh_blosc_compress_ex per chunk.
Recorded per array, chunking and route: every time, median, min-max spread, stored over raw size,
last_write_info; then the kernels of a batch by device events (zh_debug_blosc_encode_kernel_ms)
over 64 chunks of 8 MiB resident on the device (512 MiB) for both flag words, with the shuffle
kernel, the gzip kernels and the gather apart (zh_debug_blosc_zlib_encode_parts_ms).  The record is
written after every array and chunking, so a run that is cut short leaves what it measured.

    python profiles/blosc_zlib_encode_lab.py [--gib 2] [--repeats 5] [--host-repeats 1]
                                             [--out profiles/blosc_zlib_encode/lab.json]
    python profiles/blosc_zlib_encode_lab.py --write-only --tree <checkout> --out <json>
        the memcpyed route alone with another checkout's package (the parent commit:
        profiles/blosc_zlib_encode/parent_write.json)

The switch stays opt-in whatever the times say: it changes stored bytes ("Blosc frames
with zlib streams encoded on the device")."""
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
CHUNKINGS = {"8MiB": CHUNK, "64KiB": (16, CHUNK[1])}
ROUTES = {"memcpyed": {},
          "device1": {"ZH_BLOSC_ZLIB_ENCODE": "1", "ZH_BLOSC_ENCODE_DEVICE": "1"},
          "device2": {"ZH_BLOSC_ZLIB_ENCODE": "2", "ZH_BLOSC_ENCODE_DEVICE": "1"},
          "host1": {"ZH_BLOSC_ZLIB_ENCODE": "1", "ZH_BLOSC_ENCODE_DEVICE": "0"},
          "host2": {"ZH_BLOSC_ZLIB_ENCODE": "2", "ZH_BLOSC_ENCODE_DEVICE": "0"}}
SWITCHES = ("ZH_BLOSC_ZLIB_ENCODE", "ZH_BLOSC_ENCODE_DEVICE")


def spread(xs):
    return max(xs) - min(xs)


def set_route(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


def save(rec, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--chunkings", default=",".join(CHUNKINGS))
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "blosc_zlib_encode", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--write-only", action="store_true", help="the memcpyed route alone")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z

    routes = ["memcpyed"] if a.write_only else list(ROUTES)
    reps = {r: (a.host_repeats if r.startswith("host") else a.repeats) for r in routes}
    rows = max(CHUNK[0], int(a.gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2) * CHUNK[0])
    rec = {"raw_bytes": rows * CHUNK[1] * 2, "tmpfs": bool(a.tmp),
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)", "repeats": reps, "arrays": {}}
    data = np.empty((rows, CHUNK[1]), np.uint16)
    for name, make in DATASETS.items():
        for k in range(rows // CHUNK[0]):
            data[k * CHUNK[0]:(k + 1) * CHUNK[0]] = make(k)
        r = rec["arrays"][name] = {"chunkings": {}}
        for cname in a.chunkings.split(","):
            r["chunkings"][cname] = write_routes(z, a, name, data, CHUNKINGS[cname], routes, reps)
            save(rec, a.out)
        if not a.write_only:
            set_route({})
            r["kernels"] = kernel_rates(data, a.repeats)
            save(rec, a.out)
    print(json.dumps(rec), flush=True)


def write_routes(z, a, name, data, chunk, routes, reps):
    """Array.write of `data` over every route: {"chunks", "routes": {route: record}, "verdict"}."""
    out = {"chunk_shape": list(chunk), "chunks": data.shape[0] // chunk[0], "routes": {}}
    root = tempfile.mkdtemp(prefix="zh_blosc_zlib_enc_lab_", dir=a.tmp)
    try:
        meta = (z.ArrayMetadataBuilder().withShape(*data.shape).withChunkShape(*chunk)
                .withDataType(z.DataType.UINT16).withFillValue(0)
                .withCodecs(lambda c: c.withBytes("LITTLE").withBlosc("zlib", "shuffle"))
                .build())
        arrs = {rt: z.Array.create(z.FilesystemStore(os.path.join(root, rt)).resolve(name), meta)
                for rt in routes}
        times = {rt: [] for rt in routes}
        for rep in range(-1, max(reps.values())):       # -1: the warm-up; the routes alternate
            for rt in routes:
                if rep >= reps[rt] or (rep < 0 and rt.startswith("host")):
                    continue
                set_route(ROUTES[rt])
                t = time.perf_counter()
                arrs[rt].write(None, data)
                dt = time.perf_counter() - t
                if rep >= 0:
                    times[rt].append(dt)
                print(name, chunk, rt, "write rep", rep, round(dt * 1e3, 1), "ms", flush=True)
        for rt in routes:
            set_route(ROUTES[rt])
            stored = sum(os.path.getsize(os.path.join(dp, f))
                         for dp, _, fs in os.walk(os.path.join(root, rt))
                         for f in fs if not f.startswith(".") and f != "zarr.json")
            ts = times[rt]
            out["routes"][rt] = {
                "env": ROUTES[rt], "ms": [round(x * 1e3, 2) for x in ts],
                "median_ms": round(statistics.median(ts) * 1e3, 2),
                "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2),
                "spread_ms": round(spread(ts) * 1e3, 2),
                "raw_GiB_per_s": round(data.nbytes / (1 << 30) / statistics.median(ts), 3),
                "stored_bytes": stored, "stored_over_raw": round(stored / data.nbytes, 4),
                "info": getattr(arrs[rt], "last_write_info", None)}
            back = z.Array.open(arrs[rt].storeHandle).read([0, 0], list(CHUNK))
            assert np.array_equal(back, data[:CHUNK[0]]), "the array does not read back"
        if len(routes) > 1:
            rr = out["routes"]
            out["verdict"] = {f"device{m}": verdict(rr[f"device{m}"], rr["memcpyed"],
                                                    rr[f"host{m}"]) for m in "12"}
    finally:
        set_route({})
        shutil.rmtree(root, ignore_errors=True)
    return out


def verdict(dv, mc, ho):
    """The rule DESIGN.md applies to ZH_BLOSC_DEVICE: the device route beats a route when its
    median is lower by more than the larger of the two min-max spreads (a route timed once has no
    spread of its own: the device route's counts)."""
    def beats(other):
        margin = max(dv["spread_ms"], other["spread_ms"])
        return {"median_gain_ms": round(other["median_ms"] - dv["median_ms"], 2),
                "margin_ms": margin, "beats": other["median_ms"] - dv["median_ms"] > margin}
    return {"device_vs_memcpyed": beats(mc), "device_vs_host": beats(ho)}


def kernel_rates(data, repeats, nchunks=64):
    """The kernels of zh_blosc_encode_batch_ex with ZH_BLOSC_ENC_ZLIB, and with
    ZH_BLOSC_ENC_DYNAMIC (device events: shuffle, match, coder and gather of every slab), over
    chunks of 8 MiB resident on the device, one frame per chunk, and the stored size."""
    from zarrhip import _lib
    from zarrhip.array import device
    dev, L, out = device(), _lib.lib(), {}
    nchunks = min(nchunks, data.shape[0] // CHUNK[0])
    cb = CHUNK[0] * CHUNK[1] * 2
    ptr = dev.malloc(nchunks * cb)
    try:
        dev.memcpy(ptr, data.ctypes.data, nchunks * cb, 0)
        srcs = [(ptr + k * cb, cb) for k in range(nchunks)]
        for flags in (4, 12):
            ms, t_call, parts = [], [], []
            for rep in range(-1, repeats):
                t = time.perf_counter()
                _, rows = dev.blosc_encode_batch_raw(srcs, 2, 1, 0, flags=flags)
                dt = time.perf_counter() - t
                if rep >= 0:
                    ms.append(L.zh_debug_blosc_encode_kernel_ms())
                    t_call.append(dt * 1e3)
                    parts.append(_lib.blosc_zlib_encode_parts_ms())
            stored = sum(n for _, n in rows)
            out[str(flags)] = {"raw_bytes": nchunks * cb, "stored_bytes": stored,
                               "stored_over_raw": round(stored / (nchunks * cb), 4),
                               "kernel_ms": [round(x, 3) for x in ms],
                               "call_ms": [round(x, 2) for x in t_call],
                               # the shuffle kernel is the route's extra write and read of a slab
                               "parts_ms": {k: [round(p[k], 3) for p in parts]
                                            for k in ("shuffle", "segments", "gather")},
                               "raw_GiB_per_s": round(nchunks * cb / (1 << 30) /
                                                      (statistics.median(ms) / 1e3), 2)}
            print("kernels", flags, out[str(flags)], flush=True)
    finally:
        dev.free(ptr)
    return out


if __name__ == "__main__":
    main()
