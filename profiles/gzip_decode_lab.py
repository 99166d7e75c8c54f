"""Gzip members on the device against the host decoder (zlib), at a user's size.

Data: the two seeded uint16 arrays of profiles/zstd_encode_lab.py (`image`: a smooth field plus
noise in the low 4 bits; `labels`: piecewise constant), 2 GiB each, on a FilesystemStore on tmpfs,
declared [bytes little, gzip level 5], in two layouts and from two writers:
  * sharded    1024^3 elements in shards of 256^3 with inner chunks of 32^3 and gzip inside:
               32 768 members of 64 KiB of content (many small members);
  * chunked    256 unsharded chunks of 8 MiB (few large members);
  * zlib       every member compressed by zlib as GzipCodec.encode does (gzip.compress, level 5,
               mtime 0), on a thread pool, store keys set here;
  * own        the array written by Array.write with ZH_GZIP_ENCODE_DEVICE=1
               (zh_gzip_encode_batch).

Timed, in one process, alternating, after one warm-up of each route, `--repeats` times:
  * Array.read of the whole array with ZH_GZIP_DEVICE=0 (the host route: zlib per member on host
    threads, raw bytes over PCIe);
  * the same read with ZH_GZIP_DEVICE=2 (one zh_gzip_decode_batch, compressed bytes over PCIe);
  * the decode and CRC-32 kernels of that batch by device events
    (zh_debug_gzip_decode_kernel_ms), as decoded GiB/s and as a share of the read.

    python profiles/gzip_decode_lab.py [--gib 2] [--repeats 5] [--out profiles/gzip_decode/lab.json]
    python profiles/gzip_decode_lab.py --host-only --tree <checkout> --out <json>
        the host route alone with another checkout's package (the parent commit:
        profiles/gzip_decode/parent_host.json)

The default rule ("Gzip members on the device"): a layout goes to the device by default
only if, on every array of that layout, the device route's median beats the host route's by more
than the larger min-max spread of the two."""
import argparse
import gzip
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from zstd_encode_lab import CHUNK, DATASETS  # noqa: E402

SHARD, INNER, LEVEL = 256, 32, 5


def spread(xs):
    return max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_decode", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--layouts", default="sharded,chunked")
    ap.add_argument("--threads", type=int, default=16, help="of the zlib writer")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z
    from zarrhip import _lib
    L = _lib.lib()
    pool = ThreadPoolExecutor(a.threads)

    def member(b):
        return gzip.compress(b, compresslevel=LEVEL, mtime=0)

    nchunks = max(1, int(a.gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))
    nshards = max(1, nchunks * CHUNK[0] * CHUNK[1] // SHARD ** 3)
    rec = {"tmpfs": bool(a.tmp), "repeats": a.repeats,
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)", "arrays": {}}
    routes = ["0"] if a.host_only else ["0", "2"]
    data2 = np.empty((nchunks * CHUNK[0], CHUNK[1]), np.uint16)

    def chunked_meta():
        return (z.ArrayMetadataBuilder().withShape(*data2.shape).withChunkShape(*CHUNK)
                .withDataType(z.DataType.UINT16).withFillValue(0)
                .withCodecs(lambda c: c.withBytes("LITTLE").withGzip(LEVEL)).build())

    def sharded_meta():
        return (z.ArrayMetadataBuilder().withShape(nshards * SHARD, SHARD, SHARD)
                .withChunkShape(SHARD, SHARD, SHARD).withDataType(z.DataType.UINT16)
                .withFillValue(0).withCodecs(lambda c: c.withSharding(
                    [INNER] * 3, lambda c1: c1.withBytes("LITTLE").withGzip(LEVEL))).build())

    def fill_zlib(arr, data, sharded):
        if not sharded:
            frames = pool.map(lambda k: member(data[k * CHUNK[0]:(k + 1) * CHUNK[0]].tobytes()),
                              range(nchunks))
            for k, f in enumerate(frames):
                arr._handle((k, 0)).set(f)
            return
        g = SHARD // INNER
        for s in range(nshards):
            blk = data[s * SHARD:(s + 1) * SHARD]
            cells = [(i, j, k) for i in range(g) for j in range(g) for k in range(g)]
            frames = pool.map(lambda c: member(np.ascontiguousarray(
                blk[c[0] * INNER:(c[0] + 1) * INNER, c[1] * INNER:(c[1] + 1) * INNER,
                    c[2] * INNER:(c[2] + 1) * INNER]).tobytes()), cells)
            parts, ents, pos = [], [], 0
            for f in frames:
                ents.append(struct.pack("<QQ", pos, len(f)))
                parts.append(f)
                pos += len(f)
            ib = b"".join(ents)
            arr._handle((s, 0, 0)).set(b"".join(parts) + ib +
                                       struct.pack("<I", L.zh_crc32c(0, ib, len(ib))))

    for name, make in DATASETS.items():
        for k in range(nchunks):
            data2[k * CHUNK[0]:(k + 1) * CHUNK[0]] = make(k)
        data3 = data2.reshape(-1)[:nshards * SHARD ** 3].reshape(nshards * SHARD, SHARD, SHARD)
        for layout, data, meta in (("sharded", data3, sharded_meta()),
                                   ("chunked", data2, chunked_meta())):
            if layout not in a.layouts.split(","):
                continue
            for writer in ("zlib", "own"):
                key = f"{name}-{layout}-{writer}"
                root = tempfile.mkdtemp(prefix="zh_gzip_dec_lab_", dir=a.tmp)
                try:
                    h = z.FilesystemStore(root).resolve(key)
                    arr = z.Array.create(h, meta)
                    t = time.perf_counter()
                    if writer == "own":
                        os.environ["ZH_GZIP_ENCODE_DEVICE"] = "1"
                        arr.write(None, data)
                        os.environ.pop("ZH_GZIP_ENCODE_DEVICE")
                    else:
                        fill_zlib(arr, data, layout == "sharded")
                    stored = sum(os.path.getsize(os.path.join(dp, f))
                                 for dp, _, fs in os.walk(root) for f in fs if f != "zarr.json")
                    r = rec["arrays"][key] = {
                        "decoded_bytes": data.nbytes, "stored_bytes": stored,
                        "stored_over_raw": round(stored / data.nbytes, 4),
                        "write_s": round(time.perf_counter() - t, 2)}
                    print(key, json.dumps(r), flush=True)
                    arr = z.Array.open(h)
                    times = {x: [] for x in routes}
                    kms, frames = [], {}
                    for rep in range(-1, a.repeats):       # -1: the warm-up of each route
                        for x in routes:
                            os.environ["ZH_GZIP_DEVICE"] = x
                            t = time.perf_counter()
                            out = arr.read()
                            dt = time.perf_counter() - t
                            if rep < 0:
                                assert np.array_equal(out, data), f"route {x} decodes wrongly"
                                frames[x] = {k: v for k, v in arr.last_read_timing.items()
                                             if k.startswith("gzip_")}
                            else:
                                times[x].append(dt)
                                if x == "2":
                                    kms.append(L.zh_debug_gzip_decode_kernel_ms())
                            del out
                            print(key, "route", x, "rep", rep, round(dt * 1e3, 1), "ms", flush=True)
                    gib = data.nbytes / (1 << 30)
                    for x in routes:
                        r["host_route" if x == "0" else "device_route"] = {
                            "ms": [round(v * 1e3, 2) for v in times[x]],
                            "median_ms": round(statistics.median(times[x]) * 1e3, 2),
                            "spread_ms": round(spread(times[x]) * 1e3, 2),
                            "decoded_GiB_per_s": round(gib / statistics.median(times[x]), 3),
                            "frames": frames[x]}
                    if not a.host_only:
                        hm, dm = r["host_route"]["median_ms"], r["device_route"]["median_ms"]
                        margin = max(r["host_route"]["spread_ms"], r["device_route"]["spread_ms"])
                        r["device_wins"] = bool(hm - dm > margin)
                        r["rule"] = ("host median - device median = %.2f ms against a margin of "
                                     "%.2f ms" % (hm - dm, margin))
                        r["kernel"] = {"ms": [round(v, 3) for v in kms],
                                       "decoded_GiB_per_s": round(
                                           gib / (statistics.median(kms) / 1e3), 3),
                                       "share_of_read": round(statistics.median(kms) / dm, 3)}
                finally:
                    shutil.rmtree(root, ignore_errors=True)
                # the record grows array by array: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as fh:
                    json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
