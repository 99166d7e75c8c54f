"""The host half of the zstd frame writer (zarr-java_amd/csrc/zh_zstd_enc.h, zh_zstd_compress):
every frame of the input matrix decodes with libzstd (which verifies the checksum) and with the
library's decoder; frames in which nothing compresses are zh_zstd_compress_raw's, byte for byte,
and none is larger; the codec object; sizes against liblz4; and the lane-loop form under
AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import zstd_enc_inputs as zi
from zarrhip import _lib
from zarrhip.codecs import ZstdCodec

pa = pytest.importorskip("pyarrow")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = zi.matrix()


def raw_frame(data, checksum):
    L = _lib.lib()
    n = C.c_size_t()
    assert L.zh_zstd_compress_raw(data, len(data), int(checksum), None, 0, C.byref(n)) == 0
    out = (C.c_char * n.value)()
    assert L.zh_zstd_compress_raw(data, len(data), int(checksum), out, n.value, C.byref(n)) == 0
    return bytes(out)


@pytest.fixture(scope="module")
def frames():
    return [_lib.zstd_compress(d, cs, bs) for _, d, cs, bs in MATRIX]


def test_frames_decode_to_their_input(frames):
    zd, ours = pa.Codec("zstd"), ZstdCodec()
    for (label, data, cs, _), f in zip(MATRIX, frames):
        assert zi.content_size(f) == len(data) and bool(f[4] & 4) == cs, label
        got = zd.decompress(f, decompressed_size=len(data), asbytes=True) if data else b""
        assert got == data, label
        assert ours.decode(f) == data, label
    # libzstd does verify the checksum
    label, data, cs, _ = MATRIX[[r[0] for r in MATRIX].index("labels-b0-c1")]
    f = bytearray(_lib.zstd_compress(data, True, 0))
    f[-1] ^= 1
    with pytest.raises(Exception):
        zd.decompress(bytes(f), decompressed_size=len(data), asbytes=True)


def test_raw_frames_and_the_bound(frames):
    for (label, data, cs, _), f in zip(MATRIX, frames):
        raw = raw_frame(data, cs)
        assert len(f) <= len(raw), label
        if label.startswith("random"):
            assert f == raw, label


def test_block_forms(frames):
    """Blocks are cut at the block size and compressed on their own; the high length and offset
    codes and the 2-byte sequence count are reached; raw runs are merged up to 128 KiB."""
    by = {r[0]: f for r, f in zip(MATRIX, frames)}
    bl = zi.blocks(by["labels-b1024-c1"])
    assert len(bl) == 256 and all(t == 2 and s < 1024 for t, s, _ in bl)
    bl = zi.blocks(by["text-b0-c1"])
    assert all(t == 2 for t, _, _ in bl) and max(n for _, _, n in bl) > 128
    f = by[f"mix-b{zi.ONE_BLOCK}-c0"]
    assert zi.blocks(f) == [(2, len(f) - 16, 1)]
    f = by[f"far-b{zi.ONE_BLOCK}-c1"]
    assert zi.blocks(f) == [(2, len(f) - 20, 2)] and len(f) < 700   # the second piece: one match
    # mixed: the first 19 blocks of 1 KiB are noise (one raw run), the rest compress
    bl = zi.blocks(by["mix-b1024-c1"])
    assert bl[0] == (0, 19 * 1024, None) and all(t == 2 for t, _, _ in bl[1:])
    n = 3 * zi.RAW_BLOCK + 56789
    assert zi.blocks(_lib.zstd_compress(zi.random_bytes(n), False, 0)) == \
        [(0, zi.RAW_BLOCK, None)] * 3 + [(0, 56789, None)]


def test_params():
    data = zi.labels()
    # block sizes are advice: below 1 KiB is 1 KiB, above 64 KiB is 64 KiB
    assert _lib.zstd_compress(data, True, 1) == _lib.zstd_compress(data, True, 1024)
    assert _lib.zstd_compress(data, True, 1 << 20) == _lib.zstd_compress(data, True, 64 << 10)
    assert _lib.zstd_compress(data, True, 0) == _lib.zstd_compress(data, True, zi.DEFAULT_BLOCK)
    for cs, bs in ((2, 0), (1, -1)):
        prm = _lib.A.zh_zstd_enc_params(cs, bs)
        n = C.c_size_t()
        assert _lib.lib().zh_zstd_compress(data, len(data), C.byref(prm), None, 0, C.byref(n),
                                           None, 0) == _lib.A.ZH_EINVAL
    # dst == NULL: the bound is the raw-block frame; a smaller destination is refused
    prm = _lib.A.zh_zstd_enc_params(1, 0)
    n = C.c_size_t()
    assert _lib.lib().zh_zstd_compress(data, len(data), C.byref(prm), None, 0, C.byref(n),
                                       None, 0) == 0
    assert n.value == len(raw_frame(data, True))
    out = (C.c_char * n.value)()
    assert _lib.lib().zh_zstd_compress(data, len(data), C.byref(prm), out, n.value - 1,
                                       C.byref(n), None, 0) == _lib.A.ZH_EINVAL


def test_codec_object():
    data = zi.labels()
    for level, cs in ((1, True), (5, False), (19, True), (-3, False)):
        c = ZstdCodec(level, cs)
        f = c.encode(data)
        assert f == _lib.zstd_compress(data, cs) and c.decode(f) == data
        assert c.to_json()["configuration"] == {"level": level, "checksum": cs}
    assert len(ZstdCodec().encode(data)) < len(data) // 10


def test_sizes_against_liblz4():
    """Frame bytes of zh_zstd_compress at the default block size against liblz4 (pyarrow's
    lz4_raw, default settings) on the same bytes: the same class of compressor (greedy LZ,
    literals not entropy-coded).  Asserted factor: 1.384 = the measured worst ratio 1.284
    (labels: 10 485 B against liblz4's 8 166 B; text: 0.831; zeros: 0.232) plus 0.10 of headroom
    for a later retune of the hash and nothing else: the ratio table of DESIGN.md, "Zstd frames
    encoded on the device"."""
    lz, z1 = pa.Codec("lz4_raw"), pa.Codec("zstd", 1)
    for name, data in (("labels", zi.labels()), ("text", zi.text()), ("zeros", bytes(1 << 18))):
        ours = len(_lib.zstd_compress(data, True, 0))
        ref = len(lz.compress(data, asbytes=True))
        print(f"{name}: zh_zstd_compress {ours} B, liblz4 {ref} B, libzstd level 1 "
              f"{len(z1.compress(data, asbytes=True))} B, ratio {ours / ref:.4f}")
        assert ours <= ref * 1.384, (name, ours, ref)


# ---- the lane loop under sanitizers ----------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/zstd_enc_check built with AddressSanitizer + UBSan, as test_blosc_encode_host.py
    builds blosc_enc_check: stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "zstd_enc_check.cpp")
    exe = str(tmp_path_factory.mktemp("zstd_enc_check") / "zstd_enc_check")
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


def test_writer_under_sanitizers(checker, frames, tmp_path):
    src, dst = tmp_path / "buffers.bin", tmp_path / "frames.bin"
    with open(src, "wb") as fh:
        for _, data, cs, bs in MATRIX:
            fh.write(struct.pack("<III", len(data), int(cs), bs) + data)
    r = subprocess.run([checker, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(MATRIX) and all(ln.endswith(" ok") for ln in lines)
    raw = open(dst, "rb").read()
    pos = 0
    for (label, *_), f in zip(MATRIX, frames):
        (n,) = struct.unpack("<I", raw[pos:pos + 4])
        assert raw[pos + 4:pos + 4 + n] == f, label   # the library's build gives the same bytes
        pos += 4 + n
    assert pos == len(raw)
