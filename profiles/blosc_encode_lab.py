"""Blosc LZ4 frames written on the device, at a user's size.

Data: the seeded synthetic uint16 "image" of profiles/blosc_device_lab.py (a smooth field plus
noise in the low 4 bits; image_chunk below is that function), 2 GiB as a v2 array of 8 MiB chunks
declared blosc, cname lz4, byte shuffle, on a FilesystemStore on tmpfs.

Recorded, after one warm-up:
  * Array.write of the whole array, 5 repeats: median, min-max spread, last_write_info;
  * the two kernels of zh_blosc_encode_batch by device events (zh_debug_blosc_encode_kernel_ms)
    over 64 chunks resident on the device (512 MiB), GiB/s of raw input, per block-size candidate;
  * stored over raw size per candidate, next to liblz4 (pyarrow's lz4_raw) on the same
    byte-shuffled streams of the first 2 chunks (the host form of the writer is slow).

    python profiles/blosc_encode_lab.py [--gib 2] [--repeats 5] [--out profiles/blosc_encode/lab.json]
    python profiles/blosc_encode_lab.py --write-only --tree <checkout> --out <json>
        the same write timed with another checkout's package (the parent commit stores the 2 GiB
        uncompressed: profiles/blosc_encode/parent_write.json)

The default ("Blosc frames encoded on the device") stays 1 whatever the times say:
the stored size is what the codec was asked for."""
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


def spread(xs):
    return max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blosc_encode", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--blocksize", type=int, default=0, help="the codec's configured blocksize")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z
    from zarrhip import v2

    nchunks = max(1, int(a.gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))
    data = np.empty((nchunks * CHUNK[0], CHUNK[1]), np.uint16)
    for k in range(nchunks):
        data[k * CHUNK[0]:(k + 1) * CHUNK[0]] = image_chunk(k)
    rec = {"chunks": nchunks, "chunk_bytes": CHUNK[0] * CHUNK[1] * 2, "raw_bytes": data.nbytes,
           "configured_blocksize": a.blocksize, "tmpfs": bool(a.tmp),
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)"}
    root = tempfile.mkdtemp(prefix="zh_blosc_enc_lab_", dir=a.tmp)
    try:
        meta = (v2.Array.metadataBuilder().withShape(*data.shape).withChunks(*CHUNK)
                .withDataType(v2.DataType.of("<u2")).withFillValue(0)
                .withBloscCompressor("lz4", "shuffle", 5, a.blocksize).build())
        h = z.FilesystemStore(root).resolve("img")
        arr = v2.Array.create(h, meta)
        times = []
        for rep in range(-1, a.repeats):       # -1: the warm-up
            t = time.perf_counter()
            arr.write(None, data)
            dt = time.perf_counter() - t
            if rep >= 0:
                times.append(dt)
            print("write rep", rep, round(dt * 1e3, 1), "ms", flush=True)
        stored = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(root)
                     for f in fs if not f.startswith("."))
        rec["write"] = {"ms": [round(x * 1e3, 2) for x in times],
                        "median_ms": round(statistics.median(times) * 1e3, 2),
                        "spread_ms": round(spread(times) * 1e3, 2),
                        "raw_GiB_per_s": round(data.nbytes / (1 << 30) / statistics.median(times), 3),
                        "stored_bytes": stored,
                        "stored_over_raw": round(stored / data.nbytes, 4),
                        "info": getattr(arr, "last_write_info", None)}
        back = v2.Array.open(h).read([0, 0], list(CHUNK))
        assert np.array_equal(back, data[:CHUNK[0]]), "the array does not read back"
        if not a.write_only:
            rec["kernels"] = kernel_rates(data, a.repeats)
            rec["sizes"] = sizes_against_liblz4(data)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


def kernel_rates(data, repeats, nchunks=64):
    """Both kernels of zh_blosc_encode_batch (device events) over chunks resident on the device,
    one frame per chunk, per block-size candidate."""
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
                _, rows = dev.blosc_encode_batch_raw(srcs, 2, 1, bs)
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


def sizes_against_liblz4(data, nchunks=2):
    """Stream bytes (csize words and headers left out) of zh_blosc_compress and of liblz4 on the
    same byte-shuffled streams, per block-size candidate, over the first chunks."""
    try:
        import pyarrow as pa
    except ImportError:
        return None
    from zarrhip import _lib
    lz = pa.Codec("lz4_raw")
    out = {}
    for bs in CANDIDATES:
        ours = ref = raw = 0
        for k in range(min(nchunks, data.shape[0] // CHUNK[0])):
            b = data[k * CHUNK[0]:(k + 1) * CHUNK[0]].tobytes()
            f = _lib.blosc_compress(b, 2, 1, bs)
            ours += sum(r[2] for r in _lib.blosc_streams(f) if r[0] == 1)
            planes = np.frombuffer(b, np.uint8).reshape(-1, bs // 2, 2)
            for blk in planes:
                for j in range(2):
                    s = np.ascontiguousarray(blk[:, j]).tobytes()
                    ref += min(len(s), len(lz.compress(s, asbytes=True)))
            raw += len(b)
        out[str(bs)] = {"raw_bytes": raw, "zh_stream_bytes": ours, "liblz4_stream_bytes": ref,
                        "zh_over_raw": round(ours / raw, 4), "liblz4_over_raw": round(ref / raw, 4),
                        "zh_over_liblz4": round(ours / ref, 4)}
        print("sizes", bs, out[str(bs)], flush=True)
    return out


if __name__ == "__main__":
    main()
