"""Blosc frames on the device against the host decoder, at a user's size.

Data: a seeded synthetic uint16 "image" — a smooth field plus noise in the low 4 bits — as a v2
array of 8 MiB chunks, each one blosc LZ4 + byte shuffle frame of 256 KiB blocks whose streams
liblz4 made (pyarrow's lz4_raw; without pyarrow the tests' own encoder at a reduced size).

Timed, in one process, alternating, after a warm-up of each route:
  * Array.read of the whole array from a FilesystemStore on tmpfs with ZH_BLOSC_DEVICE=0 (the
    host route: zh_blosc_decompress per chunk on host threads, raw bytes over PCIe);
  * the same read with ZH_BLOSC_DEVICE=1 (one zh_blosc_decode_batch, compressed bytes over PCIe);
  * the decode kernel alone by device events (zh_debug_blosc_kernel_ms), bytes written / time,
    for unsplit / split x no / byte / bit shuffle.

    python profiles/blosc_device_lab.py [--gib 2] [--repeats 5] [--out profiles/blosc_device/lab.json]
    python profiles/blosc_device_lab.py --host-only     (any checkout: the host route alone)

The default rule ("Blosc frames on the device"): the device route becomes the default
only if its median beats the host route's by more than the larger min-max spread of the two."""
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
for p in (os.path.join(ROOT, "zarr-java_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import spec_blosc as sb  # noqa: E402
import zarrhip as z  # noqa: E402
from zarrhip import v2  # noqa: E402

CHUNK = (2048, 2048)          # uint16: 8 MiB
BLOCK = 256 << 10


def image_chunk(k, rows=CHUNK[0], cols=CHUNK[1]):
    """Chunk k of the image: a smooth field plus seeded noise in the low 4 bits."""
    y = (np.arange(rows, dtype=np.float32) + k * rows)[:, None]
    x = np.arange(cols, dtype=np.float32)[None, :]
    field = 20000 + 9000 * np.sin(y / 700.0) * np.cos(x / 500.0) + 3000 * np.sin((x + y) / 90.0)
    noise = np.random.default_rng(1000 + k).integers(0, 16, (rows, cols), dtype=np.uint16)
    return (field.astype(np.uint16) & 0xFFF0) | noise


def use_liblz4():
    try:
        import pyarrow as pa
    except ImportError:
        return False
    codec = pa.Codec("lz4_raw")
    sb.lz4_compress = lambda b: codec.compress(bytes(b), asbytes=True)
    return True


def spread(xs):
    return max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blosc_device", "lab.json"))
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    a = ap.parse_args()
    liblz4 = use_liblz4()
    gib = a.gib if liblz4 else min(a.gib, 0.125)   # the Python encoder is slow
    nchunks = max(1, int(gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))
    root = tempfile.mkdtemp(prefix="zh_blosc_lab_", dir=a.tmp)
    rec = {"encoder": "liblz4 (pyarrow lz4_raw)" if liblz4 else "tests/spec_blosc.py",
           "chunks": nchunks, "chunk_bytes": CHUNK[0] * CHUNK[1] * 2, "block_bytes": BLOCK,
           "tmpfs": bool(a.tmp)}
    try:
        meta = (v2.Array.metadataBuilder().withShape(nchunks * CHUNK[0], CHUNK[1])
                .withChunks(*CHUNK).withDataType(v2.DataType.of("<u2")).withFillValue(0)
                .withBloscCompressor("lz4", "shuffle", 5, BLOCK).build())
        h = z.FilesystemStore(root).resolve("img")
        arr = v2.Array.create(h, meta)
        t = time.perf_counter()
        cbytes, first = 0, None
        for k in range(nchunks):
            data = image_chunk(k)
            f = sb.frame(data.tobytes(), 2, BLOCK, "lz4", True, True)
            cbytes += len(f)
            arr._handle((k, 0)).set(f)
            if k == 0:
                first = data
        rec["decoded_bytes"] = nchunks * rec["chunk_bytes"]
        rec["compressed_bytes"] = cbytes
        rec["ratio"] = round(rec["decoded_bytes"] / cbytes, 3)
        rec["encode_s"] = round(time.perf_counter() - t, 2)
        print("data:", json.dumps(rec), flush=True)

        arr = v2.Array.open(h)
        routes = ["0"] if a.host_only else ["0", "1"]
        times = {r: [] for r in routes}
        frames = {}
        for rep in range(-1, a.repeats):       # -1: the warm-up of each route
            for r in routes:
                os.environ["ZH_BLOSC_DEVICE"] = r
                t = time.perf_counter()
                out = arr.read()
                dt = time.perf_counter() - t
                if rep < 0:
                    assert np.array_equal(out[:CHUNK[0]], first), "route %s decodes wrongly" % r
                    rec["checksum_route_" + r] = int(out[::97, ::89].astype(np.uint64).sum())
                    frames[r] = {k: v for k, v in arr.last_read_timing.items()
                                 if k.startswith("blosc_")}
                else:
                    times[r].append(dt)
                del out
                print("route", r, "rep", rep, round(dt * 1e3, 1), "ms", flush=True)
        gibs = rec["decoded_bytes"] / (1 << 30)
        for r in routes:
            name = "host_route" if r == "0" else "device_route"
            rec[name] = {"ms": [round(x * 1e3, 2) for x in times[r]],
                         "median_ms": round(statistics.median(times[r]) * 1e3, 2),
                         "spread_ms": round(spread(times[r]) * 1e3, 2),
                         "decoded_GiB_per_s": round(gibs / statistics.median(times[r]), 3),
                         "frames": frames[r]}
        if not a.host_only:
            hm, dm = rec["host_route"]["median_ms"], rec["device_route"]["median_ms"]
            margin = max(rec["host_route"]["spread_ms"], rec["device_route"]["spread_ms"])
            rec["device_default"] = bool(hm - dm > margin)
            rec["rule"] = "host median - device median = %.2f ms against a margin of %.2f ms" % (
                hm - dm, margin)
            rec["kernel"] = kernel_rates(a.repeats)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


def kernel_rates(repeats):
    """The decode kernel alone (device events), bytes written / kernel time, per frame kind:
    8 distinct chunks, 8 times each in one batch (512 MiB decoded)."""
    from zarrhip import _lib
    from zarrhip.array import device
    dev, L, out = device(), _lib.lib(), {}
    kinds = [("unsplit", False), ("split", True)]
    shuf = [("noshuffle", dict(shuffle=False)), ("byte", dict(shuffle=True)),
            ("bit", dict(shuffle=False, bitshuffle=True))]
    for sname, split in kinds:
        for hname, kw in shuf:
            fr = [sb.frame(image_chunk(k).tobytes(), 2, BLOCK, "lz4", split=split, **kw)
                  for k in range(8)] * 8
            views = [np.frombuffer(f, np.uint8) for f in fr]
            args = [(int(v.ctypes.data), len(f)) for v, f in zip(views, fr)]
            ms = []
            for rep in range(-1, repeats):
                ptr, rows = dev.blosc_decode_batch(args)
                dev.free(ptr)
                if rep >= 0:
                    ms.append(L.zh_debug_blosc_kernel_ms())
            nb = sum(r[1] for r in rows)
            out[f"{sname}-{hname}"] = {
                "decoded_bytes": nb, "compressed_bytes": sum(len(f) for f in fr),
                "kernel_ms": [round(x, 3) for x in ms],
                "GiB_per_s": round(nb / (1 << 30) / (statistics.median(ms) / 1e3), 2)}
            print("kernel", sname, hname, out[f"{sname}-{hname}"], flush=True)
    return out


if __name__ == "__main__":
    main()
