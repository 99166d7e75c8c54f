"""Zstd frames written on the device, at a user's size.

Data: two seeded uint16 arrays of 2 GiB, 256 chunks of 8 MiB, declared [bytes little, zstd] on a
FilesystemStore on tmpfs:
  * image    the synthetic image of profiles/blosc_encode_lab.py (a smooth field plus noise in the
             low 4 bits).  Unshuffled, LZ without entropy coding gains little on it: the cost of
             the writer when nothing compresses;
  * labels   a piecewise-constant label image (tiles of 32 x 64 pixels, one seeded label each).

Recorded per array, after one warm-up:
  * Array.write of the whole array, 5 repeats: median, min-max spread, last_write_info;
  * the kernels of zh_zstd_encode_batch by device events (zh_debug_zstd_encode_kernel_ms) over 64
    chunks resident on the device (512 MiB), GiB/s of raw input, per block-size candidate;
  * stored over raw size per candidate.

    python profiles/zstd_encode_lab.py [--gib 2] [--repeats 5] [--out profiles/zstd_encode/lab.json]
    python profiles/zstd_encode_lab.py --write-only --tree <checkout> --out <json>
        the same writes timed with another checkout's package (the parent commit stores raw
        blocks: profiles/zstd_encode/parent_write.json)

The default ("Zstd frames encoded on the device") stays 1 whatever the times say: a
stored size below 100 % is what the codec was asked for."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = (2048, 2048)          # uint16: 8 MiB
CANDIDATES = (16 << 10, 32 << 10, 64 << 10)


def image_chunk(k, rows=CHUNK[0], cols=CHUNK[1]):
    """Chunk k of the image: a smooth field plus seeded noise in the low 4 bits."""
    y = (np.arange(rows, dtype=np.float32) + k * rows)[:, None]
    x = np.arange(cols, dtype=np.float32)[None, :]
    field = 20000 + 9000 * np.sin(y / 700.0) * np.cos(x / 500.0) + 3000 * np.sin((x + y) / 90.0)
    noise = np.random.default_rng(1000 + k).integers(0, 16, (rows, cols), dtype=np.uint16)
    return (field.astype(np.uint16) & 0xFFF0) | noise


def labels_chunk(k, rows=CHUNK[0], cols=CHUNK[1]):
    """Chunk k of the label image: tiles of 32 x 64 pixels, one seeded label (1..4999) each."""
    t = np.random.default_rng(5000 + k).integers(1, 5000, (rows // 32, cols // 64), dtype=np.uint16)
    return np.repeat(np.repeat(t, 32, axis=0), 64, axis=1)


DATASETS = {"image": image_chunk, "labels": labels_chunk}


def spread(xs):
    return max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_encode", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z

    nchunks = max(1, int(a.gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))
    rec = {"chunks": nchunks, "chunk_bytes": CHUNK[0] * CHUNK[1] * 2, "tmpfs": bool(a.tmp),
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)", "arrays": {}}
    data = np.empty((nchunks * CHUNK[0], CHUNK[1]), np.uint16)
    for name, make in DATASETS.items():
        for k in range(nchunks):
            data[k * CHUNK[0]:(k + 1) * CHUNK[0]] = make(k)
        r = rec["arrays"][name] = {"raw_bytes": data.nbytes}
        root = tempfile.mkdtemp(prefix="zh_zstd_enc_lab_", dir=a.tmp)
        try:
            meta = (z.ArrayMetadataBuilder().withShape(*data.shape).withChunkShape(*CHUNK)
                    .withDataType(z.DataType.UINT16).withFillValue(0)
                    .withCodecs(lambda c: c.withBytes("LITTLE").withZstd()).build())
            h = z.FilesystemStore(root).resolve(name)
            arr = z.Array.create(h, meta)
            times = []
            for rep in range(-1, a.repeats):       # -1: the warm-up
                t = time.perf_counter()
                arr.write(None, data)
                dt = time.perf_counter() - t
                if rep >= 0:
                    times.append(dt)
                print(name, "write rep", rep, round(dt * 1e3, 1), "ms", flush=True)
            stored = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(root)
                         for f in fs if not f.startswith(".") and f != "zarr.json")
            r["write"] = {"ms": [round(x * 1e3, 2) for x in times],
                          "median_ms": round(statistics.median(times) * 1e3, 2),
                          "spread_ms": round(spread(times) * 1e3, 2),
                          "raw_GiB_per_s": round(data.nbytes / (1 << 30) / statistics.median(times),
                                                 3),
                          "stored_bytes": stored,
                          "stored_over_raw": round(stored / data.nbytes, 4),
                          "info": getattr(arr, "last_write_info", None)}
            back = z.Array.open(h).read([0, 0], list(CHUNK))
            assert np.array_equal(back, data[:CHUNK[0]]), "the array does not read back"
            if not a.write_only:
                r["kernels"] = kernel_rates(data, a.repeats)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


def kernel_rates(data, repeats, nchunks=64):
    """The kernels of zh_zstd_encode_batch (device events) over chunks resident on the device,
    one frame per chunk, and the stored size, per block-size candidate."""
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
            ms, t_call, plain = [], [], []
            for rep in range(-1, repeats):
                t = time.perf_counter()
                _, rows = dev.zstd_encode_batch_raw(srcs, True, bs)
                dt = time.perf_counter() - t
                if rep >= 0:
                    ms.append(L.zh_debug_zstd_encode_kernel_ms())
                    t_call.append(dt * 1e3)
                dev.zstd_encode_batch_raw(srcs, False, bs)   # without the hash kernel
                if rep >= 0:
                    plain.append(L.zh_debug_zstd_encode_kernel_ms())
            stored = sum(n for _, n in rows)
            out[str(bs)] = {"raw_bytes": nchunks * cb, "stored_bytes": stored,
                            "stored_over_raw": round(stored / (nchunks * cb), 4),
                            "kernel_ms": [round(x, 3) for x in ms],
                            "kernel_ms_without_checksum": [round(x, 3) for x in plain],
                            "call_ms": [round(x, 2) for x in t_call],
                            "raw_GiB_per_s": round(nchunks * cb / (1 << 30) /
                                                   (statistics.median(ms) / 1e3), 2)}
            print("kernels", bs, out[str(bs)], flush=True)
    finally:
        dev.free(ptr)
    return out


if __name__ == "__main__":
    main()
