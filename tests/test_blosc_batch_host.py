"""The host half of the batched device blosc decode (zarr-java_amd/csrc/zh_blosc_streams.h,
zh_blosc_batch_plan, zh_debug_blosc_streams): the batch plan against zh_blosc_decompress's size
query, the stream table against a walk written here, and the shared parser's serial form under
AddressSanitizer + UBSan in a stand-alone program over valid, mutated and corrupt frames.  No
GPU."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import blosc_frames as bf
import spec_blosc as sb
from helpers import GOLDEN
from zarrhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OME_BLOSC = [("v0.4/0", "0.0.0.0.0"), ("v0.4/0", "0.1.0.0.0"), ("v0.4/1", "0.0.0.0.0"),
             ("v0.4/1", "0.1.0.0.0"), ("v0.4/labels/nuclei/0", "0.0.0"),
             ("v0.4_hcs/A/1/0/0", "0.0.0.0.0"), ("v0.4_hcs/A/1/0/0", "0.1.0.0.0")]


def ome_frames():
    return [open(os.path.join(GOLDEN, "ome_blosc", *a.split("/"), k), "rb").read()
            for a, k in OME_BLOSC]


# ---- the plan --------------------------------------------------------------------------------
def test_plan_matches_the_size_query():
    data = np.arange(3000, dtype="<i4").tobytes()
    good = sb.frame(data, 4, 4096, "lz4")
    absurd = bytearray(good)
    absurd[4:8] = struct.pack("<I", 0xFFFFFFF0)          # nbytes no codec could expand to
    zero_bs = bytearray(good)
    zero_bs[8:12] = struct.pack("<I", 0)
    many = bytearray(good)
    many[8:12] = struct.pack("<I", 1)                    # more block starts than the frame holds
    cb = bytearray(good)
    cb[12:16] = struct.pack("<I", len(good) + 1)         # cbytes beyond the frame
    memc = bytearray(struct.pack("<BBBBIII", 2, 1, 0x02, 1, 64, 64, 80) + bytes(64))
    memc_short = bytes(memc[:50])
    frames = [good, good[:0], good[:10], good[:15], good[:16], good[:17], bytes(absurd),
              bytes(zero_bs), bytes(many), bytes(cb), bytes(memc), memc_short,
              sb.frame(b"", 4, 256, "lz4")]
    for f in frames:
        st, nb, msg = bf.size_query(f)
        if st == bf.ZH_OK:
            total, rows = _lib.blosc_batch_plan([f])
            assert rows[0][1] == nb and rows[0][0] == 0 and total == -(-nb // 256) * 256
        else:
            with pytest.raises(_lib.ZhError) as e:
                _lib.blosc_batch_plan([f])
            assert (e.value.status, str(e.value)) == (st, msg), f[:16]
    # every mutated frame: the same verdict as the size query
    for comp in ("lz4", "blosclz"):
        for f in bf.mutations(comp, True):
            st, nb, msg = bf.size_query(f)
            try:
                got = (bf.ZH_OK, _lib.blosc_batch_plan([f])[1][0][1], "")
            except _lib.ZhError as e:
                got = (e.status, 0, str(e))
            assert got == (st, nb if st == bf.ZH_OK else 0, msg)


def test_plan_where_and_offsets():
    data = np.arange(2000, dtype="<i4").tobytes()
    memc = struct.pack("<BBBBIII", 2, 1, 0x02, 1, 64, 64, 80) + bytes(range(64))
    frames = [sb.frame(data, 4, 4096, "lz4"), sb.frame(data, 4, 4096, "blosclz"),
              sb.frame(data, 4, 4096, "zlib"), sb.frame(data, 4, 4096, "zstd"), memc,
              sb.frame(b"", 4, 256, "lz4"), sb.frame(data[:100], 4, 4096, "lz4")]
    total, rows = _lib.blosc_batch_plan(frames)
    assert [r[2] for r in rows] == [0, 0, 1, 1, 2, 0, 0]
    assert [r[1] for r in rows] == [8000, 8000, 8000, 8000, 64, 0, 100]
    pos = 0
    for off, nb, _ in rows:
        assert off == pos and off % 256 == 0
        pos = -(-(pos + nb) // 256) * 256
    assert total == pos
    # the first bad frame in batch order is the one reported
    with pytest.raises(_lib.ZhError) as e:
        _lib.blosc_batch_plan([frames[0], frames[0][:10], frames[0][:40]])
    assert str(e.value) == "blosc frame shorter than its 16-byte header"


# ---- the stream table ------------------------------------------------------------------------
def independent_rows(frame):
    """The block / stream rows of a frame by a walk written here (the walk of
    test_blosc.independent_blosc_lz4, with the split rule read from the flags)."""
    ver, _, flags, ts = frame[0], frame[1], frame[2], frame[3]
    nbytes, blocksize, cbytes = struct.unpack("<III", frame[4:16])
    assert cbytes == len(frame) and not flags & 0x02
    comp = flags >> 5
    assert comp in (0, 1)
    nblocks = -(-nbytes // blocksize) if nbytes else 0
    bstarts = struct.unpack(f"<{nblocks}I", frame[16:16 + 4 * nblocks])
    if flags & 0x04 and not flags & 0x01:
        shuffle = 2 if ver <= 2 else 3
    else:
        shuffle = 1 if flags & 0x01 and ts > 1 else 0
    rows = []
    for b in range(nblocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        nsplits = 1 if flags & 0x10 or bsize < blocksize else ts
        rows.append((0, b * blocksize, bsize, ts, shuffle, nsplits))
        pos = bstarts[b]
        for s in range(nsplits):
            (cs,) = struct.unpack("<i", frame[pos:pos + 4])
            pos += 4
            want = bsize // nsplits
            rows.append((1, pos, cs, s * want, want, 0 if cs == want else 2 - comp))
            pos += cs
    return rows


def test_stream_table_matches_an_independent_walk():
    kinds = set()
    for label, f in bf.matrix():
        rows = _lib.blosc_streams(f)
        assert rows == independent_rows(f), label
        for r in rows:
            kinds.add(("block", r[3], r[4], r[5] > 1) if r[0] == 0 else ("stream", r[5]))
    # the matrix reached what it is there for: every typesize, split and unsplit blocks, every
    # shuffle kind, and raw, LZ4 and BloscLZ streams
    assert {k[1] for k in kinds if k[0] == "block"} == {1, 2, 3, 4, 8, 16}
    assert {k[2] for k in kinds if k[0] == "block"} == {0, 1, 2, 3}
    assert {k[3] for k in kinds if k[0] == "block"} == {True, False}
    assert {k[1] for k in kinds if k[0] == "stream"} == {0, 1, 2}
    # a leftover block is never split
    f = sb.frame(bytes(range(256)) * 40, 4, 4096, "blosclz", True, True)
    rows = [r for r in _lib.blosc_streams(f) if r[0] == 0]
    assert [r[5] for r in rows] == [4, 4, 1] and rows[-1][2] == 10240 - 8192


def test_stream_table_of_the_ome_fixtures():
    for f in ome_frames():
        rows = _lib.blosc_streams(f)
        assert rows == independent_rows(f)
        assert sum(r[2] for r in rows if r[0] == 0) == struct.unpack("<I", f[4:8])[0]


def test_stream_table_refuses_what_the_device_does_not_decode():
    data = np.arange(2000, dtype="<i4").tobytes()
    memc = struct.pack("<BBBBIII", 2, 1, 0x02, 1, 64, 64, 80) + bytes(64)
    for f in (sb.frame(data, 4, 4096, "zlib"), memc):
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_streams(f)
        assert e.value.status == bf.ZH_EUNSUPPORTED
    good = sb.frame(data, 4, 4096, "lz4")
    with pytest.raises(_lib.ZhError) as e:
        _lib.blosc_streams(good[:-7])          # cbytes beyond the frame
    assert (e.value.status, str(e.value)) == (bf.ZH_EDATA, "blosc frame truncated")
    cut = bytearray(good)
    cut[12:16] = struct.pack("<I", len(good) - 7)
    with pytest.raises(_lib.ZhError) as e:
        _lib.blosc_streams(bytes(cut[:-7]))    # the csize chain runs past the frame
    assert (e.value.status, str(e.value)) == (bf.ZH_EDATA, "blosc frame truncated")


# ---- the shared parser under sanitizers ------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/blosc_stream_check built with AddressSanitizer + UBSan: a stand-alone host
    program, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "blosc_stream_check.cpp")
    exe = str(tmp_path_factory.mktemp("blosc_check") / "blosc_stream_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    tried = []
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path is None:
            continue
        for static in (["-static-libasan"], []):  # gcc: the runtime inside the program
            r = subprocess.run([path] + flags + static + ["-o", exe, src], capture_output=True,
                               text=True)
            if r.returncode == 0:
                return exe
            tried.append(f"{path}: {r.stderr[-400:]}")
    pytest.fail("no C++ compiler built the sanitizer checker:\n" + "\n".join(tried))


def run_checker(exe, frames, tmp_path):
    p = tmp_path / "frames.bin"
    with open(p, "wb") as fh:
        for f in frames:
            fh.write(struct.pack("<I", len(f)) + f)
    r = subprocess.run([exe, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames)
    return [(int(ln.split(" ", 2)[0]), int(ln.split(" ", 2)[1], 16)) for ln in lines]


def test_shared_parser_under_sanitizers(checker, tmp_path):
    L = _lib.lib()
    frames = [f for _, f in bf.matrix()] + ome_frames()
    n_valid = len(frames)
    for comp in ("lz4", "blosclz"):
        for split in (True, False):
            frames += bf.mutations(comp, split)
    corrupt = [f for _, f in bf.corrupt_frames()]
    frames += corrupt
    got = run_checker(checker, frames, tmp_path)
    accepted = 0
    for k, (f, (st, h)) in enumerate(zip(frames, got)):
        hst, out, _ = bf.host_decode(f)
        assert st == hst, (k, st, hst)
        if st == bf.ZH_OK:
            assert h == L.zh_xxh64(out, len(out), 0), k
            accepted += 1
        if k < n_valid:
            assert st == bf.ZH_OK, k
    assert accepted > n_valid          # some mutations still decode
    # the twelve corrupt frames of the GPU test are rejected here first
    assert all(st == bf.ZH_EDATA for st, _ in got[-12:])
    texts = [bf.host_decode(f)[2] for f in corrupt]
    assert texts.count("blosc frame truncated") == 2
    assert texts.count("corrupt blosc block") == 10
