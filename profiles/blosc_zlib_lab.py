"""Blosc frames with zlib streams on the device against the two routes there were, at a user's size.

Data: the two seeded uint16 arrays of profiles/zstd_encode_lab.py (`image`: a smooth field plus
noise in the low 4 bits; `labels`: piecewise constant) as v2 arrays whose chunks are blosc frames
as c-blosc writes them for cname zlib: byte shuffle, unsplit blocks of 256 KiB (a 64 KiB chunk is
one block), every stream zlib.compress(..., 5) (compress2's stream) or stored raw where that is not
smaller.  Two layouts on a FilesystemStore on tmpfs:
  * large   chunks of 8 MiB (2048 x 2048), `--gib` GiB in all (2 GiB: 256 chunks, 8192 streams);
  * small   chunks of 64 KiB (128 x 256), `--small-gib` GiB in all (2 GiB: 32 768 chunks).

Timed, in one process, alternating, after one warm-up of each route, `--repeats` times:
  (a) Array.read of the whole array with ZH_BLOSC_DEVICE=0 (zh_blosc_decompress per chunk on
      host threads, raw bytes over PCIe);
  (b) ZH_BLOSC_DEVICE=1, ZH_BLOSC_ZLIB_DEVICE=0 (one batch call that decodes every frame with
      zh_blosc_decompress on one thread: the default);
  (c) ZH_BLOSC_DEVICE=1, ZH_BLOSC_ZLIB_DEVICE=1 (one zh_blosc_decode_batch_ex, compressed bytes
      over PCIe, both kernels), with the kernels' time by device events
      (zh_debug_blosc_kernel_ms).
Clocks: a route's time is time.perf_counter around Array.read, which returns after the device
has been synchronised and the result copied back to host memory; the kernel time is
hipEventElapsedTime between events recorded on the stream before the first and after the last
kernel of each slab, summed over the slabs.

    python profiles/blosc_zlib_lab.py [--gib 2] [--small-gib 2] [--repeats 5]
                                      [--out profiles/blosc_zlib_device/lab.json]
    python profiles/blosc_zlib_lab.py --parent --tree <checkout> --out <json>
        routes (a) and (b) alone with another checkout's package (the parent commit:
        profiles/blosc_zlib_device/parent_host.json)

The default rule ("Blosc zlib streams on the device"): the switch may default to "1"
only if on every array route (c)'s median beats the better of (a) and (b) by more than the larger
min-max spread of the two."""
import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from zstd_encode_lab import CHUNK, DATASETS  # noqa: E402

BLOCK = 256 << 10
SMALL = (128, 256)            # uint16: 64 KiB
LEVEL = 5
ROUTES = {"a": ("0", "0"), "b": ("1", "0"), "c": ("1", "1")}   # ZH_BLOSC_DEVICE, ..._ZLIB_DEVICE


def spread(xs):
    return max(xs) - min(xs)


def blosc_zlib_frame(chunk):
    """One chunk as c-blosc 1.x writes it for zlib: typesize 2, byte shuffle, unsplit blocks."""
    raw = np.ascontiguousarray(chunk).astype("<u2").tobytes()
    bs = min(BLOCK, len(raw))
    nblocks = -(-len(raw) // bs)
    base, body, starts = 16 + 4 * nblocks, bytearray(), []
    for k in range(nblocks):
        blk = np.frombuffer(raw[k * bs:(k + 1) * bs], np.uint8)
        part = blk.reshape(-1, 2).T.tobytes()
        c = zlib.compress(part, LEVEL)
        if len(c) >= len(part):
            c = part
        starts.append(base + len(body))
        body += struct.pack("<i", len(c)) + c
    flags = (3 << 5) | 0x10 | 0x01
    hdr = struct.pack("<BBBBIII", 2, 1, flags, 2, len(raw), bs, base + len(body))
    return hdr + struct.pack("<%di" % nblocks, *starts) + bytes(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--small-gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blosc_zlib_device", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--parent", action="store_true", help="routes (a) and (b) only")
    ap.add_argument("--layouts", default="large,small")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z
    from zarrhip import _lib, v2
    L = _lib.lib()
    routes = ["a", "b"] if a.parent else ["a", "b", "c"]
    rec = {"tmpfs": bool(a.tmp), "repeats": a.repeats,
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)",
           "frames": "blosc1, zlib streams by zlib.compress level %d (zlib %s), byte shuffle, "
                     "unsplit blocks of 256 KiB" % (LEVEL, zlib.ZLIB_RUNTIME_VERSION),
           "clocks": {"route": "time.perf_counter around Array.read of the whole array into host "
                               "memory (ends after the device synchronise and the copy back)",
                      "kernel": "hipEventElapsedTime around both kernels of each slab, summed "
                                "(zh_debug_blosc_kernel_ms), route (c)"},
           "routes": {"a": "ZH_BLOSC_DEVICE=0", "b": "ZH_BLOSC_DEVICE=1 ZH_BLOSC_ZLIB_DEVICE=0",
                      "c": "ZH_BLOSC_DEVICE=1 ZH_BLOSC_ZLIB_DEVICE=1"},
           "arrays": {}}
    for name, make in DATASETS.items():
        for layout, cshape, gib in (("large", CHUNK, a.gib), ("small", SMALL, a.small_gib)):
            if layout not in a.layouts.split(","):
                continue
            nrows = max(1, int(gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))   # 8 MiB bands
            key = f"{name}-{layout}"
            root = tempfile.mkdtemp(prefix="zh_blosc_zlib_lab_", dir=a.tmp)
            try:
                meta = (v2.Array.metadataBuilder().withShape(nrows * CHUNK[0], CHUNK[1])
                        .withChunks(*cshape).withDataType(v2.DataType.of("<u2")).withFillValue(0)
                        .withBloscCompressor("zlib", "shuffle", LEVEL, BLOCK).build())
                h = z.FilesystemStore(root).resolve(key)
                arr = v2.Array.create(h, meta)
                data = np.empty((nrows * CHUNK[0], CHUNK[1]), np.uint16)
                for k in range(nrows):
                    data[k * CHUNK[0]:(k + 1) * CHUNK[0]] = make(k)
                t = time.perf_counter()
                coords = arr._chunk_coords([0, 0], list(data.shape))

                def put(c):
                    f = blosc_zlib_frame(data[c[0] * cshape[0]:(c[0] + 1) * cshape[0],
                                              c[1] * cshape[1]:(c[1] + 1) * cshape[1]])
                    arr._handle(c).set(f)
                    return len(f)
                with ThreadPoolExecutor(max_workers=16) as ex:
                    stored = sum(ex.map(put, coords))
                r = rec["arrays"][key] = {
                    "chunks": len(coords), "chunk_bytes": cshape[0] * cshape[1] * 2,
                    "decoded_bytes": data.nbytes, "stored_bytes": stored,
                    "stored_over_raw": round(stored / data.nbytes, 4),
                    "encode_s": round(time.perf_counter() - t, 2)}
                print(key, json.dumps(r), flush=True)
                arr = v2.Array.open(h)
                times = {x: [] for x in routes}
                kms, frames = [], {}
                for rep in range(-1, a.repeats):       # -1: the warm-up of each route
                    for x in routes:
                        os.environ["ZH_BLOSC_DEVICE"], os.environ["ZH_BLOSC_ZLIB_DEVICE"] = ROUTES[x]
                        t = time.perf_counter()
                        out = arr.read()
                        dt = time.perf_counter() - t
                        if rep < 0:
                            assert np.array_equal(out, data), f"route {x} decodes wrongly"
                            frames[x] = {k: v for k, v in arr.last_read_timing.items()
                                         if k.startswith("blosc_")}
                        else:
                            times[x].append(dt)
                            if x == "c":
                                kms.append(L.zh_debug_blosc_kernel_ms())
                        del out
                        print(key, "route", x, "rep", rep, round(dt * 1e3, 1), "ms", flush=True)
                gibs = data.nbytes / (1 << 30)
                for x in routes:
                    r["route_" + x] = {
                        "ms": [round(v * 1e3, 2) for v in times[x]],
                        "median_ms": round(statistics.median(times[x]) * 1e3, 2),
                        "min_ms": round(min(times[x]) * 1e3, 2),
                        "max_ms": round(max(times[x]) * 1e3, 2),
                        "spread_ms": round(spread(times[x]) * 1e3, 2),
                        "decoded_GiB_per_s": round(gibs / statistics.median(times[x]), 3),
                        "frames": frames[x]}
                if not a.parent:
                    best = min(("a", "b"), key=lambda x: r["route_" + x]["median_ms"])
                    bm, cm = r["route_" + best]["median_ms"], r["route_c"]["median_ms"]
                    margin = max(r["route_" + best]["spread_ms"], r["route_c"]["spread_ms"])
                    r["best_of_a_b"] = best
                    r["device_wins"] = bool(bm - cm > margin)
                    r["rule"] = ("route (%s) median - route (c) median = %.2f ms against a margin "
                                 "of %.2f ms" % (best, bm - cm, margin))
                    r["kernel"] = {"ms": [round(v, 3) for v in kms],
                                   "decoded_GiB_per_s": round(
                                       gibs / (statistics.median(kms) / 1e3), 3)}
                am, bmed = r["route_a"]["median_ms"], r["route_b"]["median_ms"]
                margin = max(r["route_a"]["spread_ms"], r["route_b"]["spread_ms"])
                r["b_slower_than_a"] = bool(bmed - am > margin)
                del data
            finally:
                shutil.rmtree(root, ignore_errors=True)
            # the record grows array by array: a run cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(rec, fh, indent=1)
    if not a.parent:
        rec["rule_met"] = all(r.get("device_wins") for r in rec["arrays"].values())
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
