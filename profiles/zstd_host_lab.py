"""zh_zstd_decompress of two builds of the library on the same frames, one thread, no device.

Frames: libzstd (pyarrow) levels 1 and 3 of 8 MiB each of seeded word text, an int16 random walk
and a uint16 label image.  The two libraries decode every frame in turn, `--repeats` times each
after one warm-up; both must return the same bytes.  The rule: the median MB/s of `--lib` must not
be below that of `--parent-lib` by more than the larger min-max spread of the two.

    python profiles/zstd_host_lab.py --parent-lib <libzarrhip.so of the parent commit>
        [--lib zarr-java_amd/zarrhip/libzarrhip.so] [--repeats 7]
        [--out profiles/zstd_decode/host_unify.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import time

import numpy as np
import pyarrow as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8 << 20


def datasets():
    rng = np.random.default_rng(20240607)
    vocab = [b"zarr", b"chunk", b"shard", b"codec", b"the", b"of", b"array", b"index", b"bytes",
             b"wave", b"lane", b"frame", b"block"]
    words = b" ".join(vocab[i] for i in rng.integers(0, 13, N // 4))[:N]
    walk = np.cumsum(rng.integers(-3, 4, N // 2)).astype("<i2").tobytes()
    t = rng.integers(1, 5000, (64, 32), dtype=np.uint16)
    labels = np.repeat(np.repeat(t, 32, axis=0), 64, axis=1).astype("<u2").tobytes()
    return {"words": words, "walk": walk, "labels": labels}


def load(path):
    L = C.CDLL(os.path.abspath(path))
    L.zh_zstd_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    return L


def decode(L, frame, out):
    n, err = C.c_size_t(), C.create_string_buffer(256)
    t = time.perf_counter()
    st = L.zh_zstd_decompress(frame, len(frame), out, len(out), C.byref(n), err, 256)
    dt = time.perf_counter() - t
    assert st == 0 and n.value == len(out), err.value
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "zarr-java_amd", "zarrhip", "libzarrhip.so"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_decode",
                                                  "host_unify.json"))
    a = ap.parse_args()
    libs = {"parent": load(a.parent_lib), "new": load(a.lib)}
    rec = {"repeats": a.repeats, "content_bytes": N, "threads": 1, "frames": {}}
    holds = True
    for name, data in datasets().items():
        assert len(data) >= N
        for level in (1, 3):
            frame = pa.Codec("zstd", compression_level=level).compress(data, asbytes=True)
            out = {w: C.create_string_buffer(len(data)) for w in libs}
            rate = {w: [] for w in libs}
            for rep in range(-1, a.repeats):
                for w, L in libs.items():
                    dt = decode(L, frame, out[w])
                    if rep >= 0:
                        rate[w].append(len(data) / dt / 1e6)
            assert out["parent"].raw == out["new"].raw == data
            r = {w: {"MB_per_s": [round(v, 1) for v in rate[w]],
                     "median": round(statistics.median(rate[w]), 1),
                     "spread": round(max(rate[w]) - min(rate[w]), 1)} for w in libs}
            r["stored_over_raw"] = round(len(frame) / len(data), 4)
            r["holds"] = r["new"]["median"] >= r["parent"]["median"] - max(
                r["new"]["spread"], r["parent"]["spread"])
            holds = holds and r["holds"]
            rec["frames"][f"{name} L{level}"] = r
            print(name, level, r["parent"]["median"], r["new"]["median"], r["holds"], flush=True)
    rec["holds"] = holds
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
