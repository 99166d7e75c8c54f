"""The host half of the gzip member writer (zarr-java_amd/csrc/zh_gzip_enc.h, zh_gzip_compress):
every member of the input matrix decodes with zlib and with Python's gzip; header, CRC-32 and
ISIZE are as specified; the bound is reported and kept; both segment forms, every length code
and the last distance code are reached; zh_crc32 chains as zlib.crc32; sizes against zlib; and
the lane-loop form under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gzip_enc_inputs as gi
from zarrhip import _lib
from zarrhip.codecs import GzipCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = gi.matrix()


@pytest.fixture(scope="module")
def members():
    return [_lib.gzip_compress(d, bs) for _, d, bs in MATRIX]


def by_label(members):
    return {r[0]: f for r, f in zip(MATRIX, members)}


def test_members_decode_to_their_input(members):
    for (label, data, bs), f in zip(MATRIX, members):
        assert zlib.decompress(f, 31) == data, label
        assert gzip.decompress(f) == data, label
        assert f[:10] == gi.HEADER, label
        assert f[-10:-8] == b"\x03\x00", label
        assert struct.unpack("<II", f[-8:]) == (zlib.crc32(data), len(data) % 2 ** 32), label
        assert f == _lib.gzip_compress(data, bs), label           # twice: the same bytes
    # zlib does verify the trailer
    f = bytearray(by_label(members)["labels-b0"])
    f[-5] ^= 1
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(f), 31)


def test_empty_member():
    """Header + 03 00 + trailer.  Python writes XFL 0 at the codec's default level 5 (and at
    every level but 1 and 9, Python's own default, where byte 8 is 4 or 2)."""
    f = _lib.gzip_compress(b"")
    assert len(f) == 20 and f == gi.HEADER + b"\x03\x00" + bytes(8)
    assert f == gzip.compress(b"", 5, mtime=0)
    py = gzip.compress(b"", mtime=0)
    assert f[:8] + f[9:] == py[:8] + py[9:] and py[8] == 2


def test_the_bound(members):
    L = _lib.lib()
    for (label, data, bs), f in zip(MATRIX, members):
        prm = _lib.A.zh_gzip_enc_params(bs)
        n = C.c_size_t()
        assert L.zh_gzip_compress(data, len(data), C.byref(prm), None, 0, C.byref(n), None, 0) == 0
        assert n.value == gi.bound(len(data), bs), label
        assert len(f) <= n.value, label
        if label.startswith("random") or label.startswith("high_bytes"):
            assert len(f) == n.value, label                       # every block stored
            assert {s[0] for s in gi.segments(f)} <= {"stored"}, label


def test_segment_forms(members):
    """Blocks are cut at the block size and coded on their own; both forms occur; the length
    codes, the split rule and the last distance code are reached."""
    by = by_label(members)
    data = gi.labels()
    f = by["labels-b0"]
    assert len(f) < gi.bound(len(data), 0) // 20
    segs = gi.segments(f)
    assert [s[:2] for s in segs] == [("fixed", gi.DEFAULT_BLOCK)] * 16
    segs = gi.segments(by["labels-b1024"])
    assert len(segs) == 256 and all(s[0] == "fixed" and s[2] < 1024 for s in segs)
    # mixed: the first 19 blocks of 1 KiB are noise, the rest zeros
    segs = gi.segments(by["mix-b1024"])
    assert [s[0] for s in segs] == ["stored"] * 19 + ["fixed"] * 13
    assert all(s[2] == s[1] + 5 for s in segs[:19])
    assert sum(s[1] for s in segs) == len(gi.mix())
    # 9-bit literals between matches
    assert {s[0] for s in gi.segments(by["high_text-b0"])} == {"fixed"}
    # far(): the second piece is one match of 600 bytes at 30 600 (distance code 29), split
    (seg,) = gi.segments(by[f"far-b{gi.MAX_BLOCK}"])
    assert seg[0] == "fixed" and seg[3][-3:] == [(258, 30600, 0), (258, 30600, 0), (84, 30600, 0)]
    assert len(by[f"far-b{gi.MAX_BLOCK}"]) < 1000
    # every length code, on both sides of its first length
    for bs in (0, gi.MAX_BLOCK):
        lens = {ln for s in gi.segments(by[f"length_codes-b{bs}"]) if s[3] for ln, _, _ in s[3]}
        want = {n for b in gi.LENGTH_BASES for n in (b - 1, b, b + 1) if 4 <= n <= 258}
        assert want <= lens, sorted(want - lens)
    # the split rule: no piece over 258 or under 3; a run of 258 k + r zeros is one match of
    # 258 k + r - 1 bytes at distance 1
    (seg,) = gi.segments(by["zero_runs-b0"])
    assert all(3 <= ln <= 258 for ln, _, _ in seg[3])

    def split(n):
        out = []
        while n > 258:
            out.append(258 if n - 258 >= 3 else n - 3)
            n -= out[-1]
        return out + [n]
    runs = []                                     # the pieces of each match: no literal between
    for ln, _, nlit in seg[3]:
        if nlit:
            runs.append([])
        runs[-1].append(ln)
    for want in (258 * k + r - 1 for k in (1, 2, 3) for r in (0, 1, 2, 3, 4)):
        assert split(want) in runs, want
    assert split(259) == [256, 3] and split(260) == [257, 3] and split(261) == [258, 3]


def test_params():
    data = gi.labels()
    # block sizes are advice: below 1 KiB is 1 KiB, above 32 KiB is 32 KiB
    assert _lib.gzip_compress(data, 1) == _lib.gzip_compress(data, 1024)
    assert _lib.gzip_compress(data, 1 << 20) == _lib.gzip_compress(data, 32 << 10)
    assert _lib.gzip_compress(data, 0) == _lib.gzip_compress(data, gi.DEFAULT_BLOCK)
    L = _lib.lib()
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    prm = _lib.A.zh_gzip_enc_params(-1)
    assert L.zh_gzip_compress(data, len(data), C.byref(prm), None, 0, C.byref(n), err,
                              256) == _lib.A.ZH_EINVAL
    assert err.value == b"zh_gzip_compress: blocksize >= 0"
    # a destination smaller than the bound is refused
    prm = _lib.A.zh_gzip_enc_params(0)
    assert L.zh_gzip_compress(data, len(data), C.byref(prm), None, 0, C.byref(n), None, 0) == 0
    out = (C.c_char * n.value)()
    assert L.zh_gzip_compress(data, len(data), C.byref(prm), out, n.value - 1, C.byref(n), err,
                              256) == _lib.A.ZH_EINVAL
    assert err.value == b"zh_gzip_compress: destination smaller than the bound"
    with pytest.raises(_lib.ZhError):
        _lib.gzip_compress(data, -5)


def test_crc32_chains_as_zlib():
    data = gi.random_bytes(70001, 31)
    assert _lib.crc32(b"") == 0 and _lib.crc32(b"", 77) == 77
    assert _lib.lib().zh_crc32(123, None, 0) == 0
    for n in (1, 3, 4, 255, 256, 257, 65536, 70001):
        assert _lib.crc32(data[:n]) == zlib.crc32(data[:n]), n
    for cut in (0, 1, 100, 65536, 70001):
        assert _lib.crc32(data[cut:], _lib.crc32(data[:cut])) == zlib.crc32(data), cut
    assert _lib.crc32(data, 0xDEADBEEF) == zlib.crc32(data, 0xDEADBEEF)


def test_codec_object_stays_zlib():
    data = gi.labels()
    for level in (1, 5, 9):
        c = GzipCodec(level)
        assert c.encode(data) == gzip.compress(data, compresslevel=level, mtime=0)
        assert c.decode(_lib.gzip_compress(data)) == data
        assert c.to_json()["configuration"] == {"level": level}


def noisy_image(n=1 << 18):
    """A random walk as <u2: the high bytes repeat, the low bytes are noise."""
    rng = np.random.default_rng(12)
    return np.cumsum(rng.integers(-40, 41, n // 2)).astype("<u2").tobytes()


def test_sizes_against_zlib():
    """Member bytes of zh_gzip_compress at the default block size against zlib levels 1 and 5 on
    the same bytes.  Measured (the table of DESIGN.md, "Gzip members encoded on the device"):
      labels   262 144 B:   8 664 B; zlib level 1   4 964 B (1.7454), level 5   6 260 B (1.3840)
      text      69 237 B:  24 085 B; zlib level 1  14 278 B (1.6869), level 5  10 467 B (2.3010)
      zeros    262 144 B:   1 812 B; zlib level 1   1 179 B (1.5369), level 5     289 B (6.2699)
      noisy    262 144 B: 262 244 B; zlib level 1 195 961 B (1.3382), level 5 195 237 B (1.3432)
    Asserted on labels and text: the measured worst ratio to zlib level 1, 1.7454, plus 0.10 of
    headroom for a later retune of the hash and nothing else.  The writer has fixed-Huffman
    blocks only, so what LZ alone does not shrink (the noisy image) is stored."""
    worst = 0.0
    for name, data in (("labels", gi.labels()), ("text", gi.text()), ("zeros", bytes(1 << 18)),
                       ("noisy", noisy_image())):
        ours = len(_lib.gzip_compress(data))
        z1, z5 = len(gzip.compress(data, 1, mtime=0)), len(gzip.compress(data, 5, mtime=0))
        print(f"{name}: raw {len(data)} B, zh_gzip_compress {ours} B, zlib level 1 {z1} B "
              f"(ratio {ours / z1:.4f}), zlib level 5 {z5} B (ratio {ours / z5:.4f})")
        if name in ("labels", "text"):
            worst = max(worst, ours / z1)
            assert ours <= z1 * 1.8454, (name, ours, z1)
    print(f"worst ratio to zlib level 1 on labels and text: {worst:.4f}")


# ---- the lane loop under sanitizers ----------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/gzip_enc_check built with AddressSanitizer + UBSan, as test_zstd_encode_host.py
    builds zstd_enc_check: stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "gzip_enc_check.cpp")
    exe = str(tmp_path_factory.mktemp("gzip_enc_check") / "gzip_enc_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    tried = []
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path is None:
            continue
        for static in (["-static-libasan"], []):  # gcc: the runtime inside the program
            r = subprocess.run([path] + flags + static + ["-o", exe, src, "-lz"],
                               capture_output=True, text=True)
            if r.returncode == 0:
                return exe
            tried.append(f"{path}: {r.stderr[-400:]}")
    pytest.fail("no C++ compiler built the sanitizer checker:\n" + "\n".join(tried))


def test_writer_under_sanitizers(checker, members, tmp_path):
    src, dst = tmp_path / "buffers.bin", tmp_path / "members.bin"
    with open(src, "wb") as fh:
        for _, data, bs in MATRIX:
            fh.write(struct.pack("<II", len(data), bs) + data)
    r = subprocess.run([checker, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(MATRIX) and all(ln.endswith(" ok") for ln in lines)
    raw = open(dst, "rb").read()
    pos = 0
    for (label, *_), f in zip(MATRIX, members):
        (n,) = struct.unpack("<I", raw[pos:pos + 4])
        assert raw[pos + 4:pos + 4 + n] == f, label   # the library's build gives the same bytes
        pos += 4 + n
    assert pos == len(raw)
