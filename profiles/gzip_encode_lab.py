"""Gzip members written on the device, at a user's size.

Data: the two seeded uint16 arrays of profiles/zstd_encode_lab.py (`image`, `labels`; 2 GiB, 256
chunks of 8 MiB), declared [bytes little, gzip level 5] on a FilesystemStore on tmpfs.

Recorded per array, after one warm-up:
  * Array.write of the whole array with ZH_GZIP_ENCODE_DEVICE=1 (or --switch), 5 repeats:
    median, min-max spread, last_write_info, stored over raw size;
  * the kernels of zh_gzip_encode_batch by device events, per kernel (match, coder, CRC-32,
    gather: zh_debug_gzip_encode_kernel_parts_ms), over 64 chunks resident on the device
    (512 MiB), per block-size candidate, and the stored size per candidate.

    python profiles/gzip_encode_lab.py [--gib 2] [--repeats 5] [--out profiles/gzip_encode/lab.json]
    python profiles/gzip_encode_lab.py --write-only --tree <checkout> --out <json>
        the same writes timed with another checkout's package (the parent commit compresses
        with zlib on one host thread: profiles/gzip_encode/parent_write.json)
    python profiles/gzip_encode_lab.py --switch 2
        the same with ZH_GZIP_ENCODE_DEVICE=2 and dynamic = 1 in the kernel runs:
        dynamic-Huffman segments in the per-block choice
    python profiles/gzip_encode_lab.py --switch 1,2 --out profiles/gzip_encode/lab_dynamic.json
        both in one process, in alternation (a repeat writes with 1, then with 2; a kernel
        repeat runs dynamic 0, then 1): the record keeps them under "by_switch".  Times of the
        two are compared within such a record only: the machine differs from run to run.

The write with the switch at 1 is compared with the parent's write of the same array only.  The
default ("Gzip members encoded on the device") stays 0 whatever the times say: the
stored size on data that LZ alone does not compress is larger than zlib's."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from zstd_encode_lab import CHUNK, DATASETS, spread  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES = (16 << 10, 32 << 10)
LEVEL = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_encode", "lab.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--arrays", default="labels,image")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--switch", choices=("1", "2", "1,2"), default="1",
                    help="ZH_GZIP_ENCODE_DEVICE; 1,2: both in alternation")
    a = ap.parse_args()
    switches = a.switch.split(",")
    os.environ["ZH_GZIP_ENCODE_DEVICE"] = switches[0]   # the parent commit has no such switch
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "zarr-java_amd"))
    import zarrhip as z

    nchunks = max(1, int(a.gib * (1 << 30)) // (CHUNK[0] * CHUNK[1] * 2))
    rec = {"chunks": nchunks, "chunk_bytes": CHUNK[0] * CHUNK[1] * 2, "tmpfs": bool(a.tmp),
           "codecs": f"[bytes little, gzip level {LEVEL}]", "ZH_GZIP_ENCODE_DEVICE": a.switch,
           "package": "this checkout" if os.path.abspath(a.tree) == ROOT else
           "another checkout (--tree)", "arrays": {}}
    data = np.empty((nchunks * CHUNK[0], CHUNK[1]), np.uint16)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.arrays.split(","):
        make = DATASETS[name]
        for k in range(nchunks):
            data[k * CHUNK[0]:(k + 1) * CHUNK[0]] = make(k)
        r = rec["arrays"][name] = {"raw_bytes": data.nbytes}
        root = tempfile.mkdtemp(prefix="zh_gzip_enc_lab_", dir=a.tmp)
        try:
            meta = (z.ArrayMetadataBuilder().withShape(*data.shape).withChunkShape(*CHUNK)
                    .withDataType(z.DataType.UINT16).withFillValue(0)
                    .withCodecs(lambda c: c.withBytes("LITTLE").withGzip(LEVEL)).build())
            arrs = {sw: z.Array.create(z.FilesystemStore(os.path.join(root, sw)).resolve(name),
                                       meta) for sw in switches}
            times = {sw: [] for sw in switches}
            for rep in range(-1, a.repeats):       # -1: the warm-up
                for sw in switches:
                    os.environ["ZH_GZIP_ENCODE_DEVICE"] = sw
                    t = time.perf_counter()
                    arrs[sw].write(None, data)
                    dt = time.perf_counter() - t
                    if rep >= 0:
                        times[sw].append(dt)
                    print(name, "switch", sw, "write rep", rep, round(dt * 1e3, 1), "ms",
                          flush=True)
            by = {}
            for sw in switches:
                stored = sum(os.path.getsize(os.path.join(dp, f))
                             for dp, _, fs in os.walk(os.path.join(root, sw))
                             for f in fs if not f.startswith(".") and f != "zarr.json")
                ts = times[sw]
                by[sw] = {"write": {
                    "ms": [round(x * 1e3, 2) for x in ts],
                    "median_ms": round(statistics.median(ts) * 1e3, 2),
                    "spread_ms": round(spread(ts) * 1e3, 2),
                    "raw_GiB_per_s": round(data.nbytes / (1 << 30) / statistics.median(ts), 3),
                    "stored_bytes": stored,
                    "stored_over_raw": round(stored / data.nbytes, 4),
                    "info": getattr(arrs[sw], "last_write_info", None)}}
                back = z.Array.open(arrs[sw].storeHandle).read([0, 0], list(CHUNK))
                assert np.array_equal(back, data[:CHUNK[0]]), "the array does not read back"
            if not a.write_only:
                for sw, k in kernel_rates(data, a.repeats, switches).items():
                    by[sw]["kernels"] = k
            if len(switches) == 1:
                r.update(by[switches[0]])
            else:
                r["by_switch"] = by
        finally:
            shutil.rmtree(root, ignore_errors=True)
        with open(a.out, "w") as fh:               # after every array: a long run keeps its part
            json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


def kernel_rates(data, repeats, switches=("1",), nchunks=64):
    """The kernels of zh_gzip_encode_batch (device events, per kernel) over chunks resident on
    the device, one member per chunk, and the stored size, per block-size candidate: {switch:
    {block size: record}}; switch 2 runs with dynamic = 1, and a repeat runs every switch."""
    from zarrhip import _lib
    from zarrhip.array import device
    dev, out = device(), {sw: {} for sw in switches}
    nchunks = min(nchunks, data.shape[0] // CHUNK[0])
    cb = CHUNK[0] * CHUNK[1] * 2
    ptr = dev.malloc(nchunks * cb)
    try:
        dev.memcpy(ptr, data.ctypes.data, nchunks * cb, 0)
        srcs = [(ptr + k * cb, cb) for k in range(nchunks)]
        for bs in CANDIDATES:
            parts = {sw: [] for sw in switches}
            t_call = {sw: [] for sw in switches}
            stored = {}
            for rep in range(-1, repeats):
                for sw in switches:
                    kw = {"dynamic": True} if sw == "2" else {}
                    t = time.perf_counter()
                    _, rows = dev.gzip_encode_batch_raw(srcs, bs, **kw)
                    dt = time.perf_counter() - t
                    stored[sw] = sum(n for _, n in rows)
                    if rep >= 0:
                        parts[sw].append(_lib.gzip_encode_kernel_parts_ms())
                        t_call[sw].append(dt * 1e3)
            for sw in switches:
                ps = parts[sw]
                med = {k: round(statistics.median(p[k] for p in ps), 3) for k in ps[0]}
                total = statistics.median(sum(p.values()) for p in ps)
                out[sw][str(bs)] = {
                    "raw_bytes": nchunks * cb, "stored_bytes": stored[sw],
                    "stored_over_raw": round(stored[sw] / (nchunks * cb), 4),
                    "kernel_ms_median": med,
                    "kernel_ms_spread": {k: round(spread([p[k] for p in ps]), 3) for k in ps[0]},
                    "kernel_ms_total_median": round(total, 3),
                    "call_ms": [round(x, 2) for x in t_call[sw]],
                    "raw_GiB_per_s": round(nchunks * cb / (1 << 30) / (total / 1e3), 2)}
                print("kernels", "switch", sw, bs, out[sw][str(bs)], flush=True)
    finally:
        dev.free(ptr)
    return out


if __name__ == "__main__":
    main()
