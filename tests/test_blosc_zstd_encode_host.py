"""The host half of the blosc frame writer with zstd streams (zarr-java_amd/csrc/zh_blosc_enc.h
over ZstdCoder, zh_blosc_compress_ex with ZH_BLOSC_ENC_ZSTD): every frame of the input matrix
equals the frame built in Python around zh_zstd_compress (blosc_zstd_enc_inputs.expected), decodes
with the library's decoder, has its streams decoded by libzstd and is planned for the device
decoder; the flags of the call; the block-size thresholds; the codec object behind
ZH_BLOSC_ZSTD_ENCODE; and the lane-loop form under AddressSanitizer + UBSan in a stand-alone
program.  No GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import blosc_enc_inputs as bi
import blosc_frames as bf
import blosc_zstd_enc_inputs as be
import blosc_zstd_inputs as bz
from zarrhip import _abi as A
from zarrhip import _lib
from zarrhip.codecs import BloscCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = be.matrix()


def compress_ex(data, ts, sh, bs, flags, cap=None, query=False):
    """zh_blosc_compress_ex as it is: (status, frame or None, *cbytes)."""
    L = _lib.lib()
    data = bytes(data)
    prm = A.zh_blosc_enc_params(ts, sh, bs)
    cap = len(data) + 16 if cap is None else cap
    out = None if query else C.create_string_buffer(max(1, cap))
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    st = L.zh_blosc_compress_ex(data, len(data), C.byref(prm), flags, out, cap, C.byref(n), err,
                                256)
    return st, (out.raw[:n.value] if st == bf.ZH_OK and not query else None), n.value


@pytest.fixture(scope="module")
def frames():
    return [_lib.blosc_compress(d, ts, sh, bs, zstd=True) for _, d, ts, sh, bs, _ in MATRIX]


def test_matrix_equals_the_python_built_frames(frames):
    kinds = {"zstd": 0, "raw": 0, "frames": 0, "memcpyed": 0}
    for (label, data, ts, sh, bs, want), f in zip(MATRIX, frames):
        assert f == want, label
        st, out, msg = bf.host_decode(f)
        assert (st, out) == (bf.ZH_OK, data), (label, msg)
        assert len(f) <= len(data) + 16 and struct.unpack("<I", f[12:16])[0] == len(f), label
        assert f[0] == 2 and f[1] == 1 and f[2] >> 5 == 4, label
        name = be.name_of(label)
        if name in be.COMPRESSED:       # a writer that stores everything plain does not pass
            assert not f[2] & 0x02, label
        if name in be.MEMCPYED:
            assert f[2] & 0x02 and f[16:] == data, label
        if f[2] & 0x02:
            kinds["memcpyed"] += 1
            continue
        kinds["frames"] += 1
        for r in _lib.blosc_streams(f, bz.FLAG):
            if r[0] == 1:
                kinds["zstd" if r[5] == bz.KZSTD else "raw"] += 1
    # the counts of the construction over blosc_enc_inputs.matrix()
    assert kinds == {"zstd": 331, "raw": 41, "frames": 157, "memcpyed": 113}


def test_libzstd_decodes_the_streams_and_the_device_decoder_takes_the_frames(frames):
    pa = pytest.importorskip("pyarrow")
    zs = pa.Codec("zstd")
    seen = 0
    for (label, data, ts, sh, bs, _), f in zip(MATRIX, frames):
        if f[2] & 0x02:
            continue
        assert _lib.blosc_batch_plan([f], bz.FLAG)[1][0][2] == 0, label     # where = 0
        b, split = be.layout(len(data), ts, sh, bs)
        raw = [s for blk in bz.shuffled_streams(data, ts, b, be.SHUFFLE_NAME[sh], split)
               for s in blk]
        rows = [r for r in _lib.blosc_streams(f, bz.FLAG) if r[0] == 1]
        assert len(rows) == len(raw), label
        for r, want in zip(rows, raw):
            assert r[4] == len(want), label
            payload = f[r[1]:r[1] + r[2]]
            if r[2] == r[4]:
                assert r[5] == 0 and payload == want, label
                continue
            assert r[5] == bz.KZSTD and r[2] < r[4], label
            assert zs.decompress(payload, decompressed_size=r[4], asbytes=True) == want, label
            seen += 1
    assert seen == 331


def test_flags():
    data, ts, sh, bs = bi.img(), 2, 1, bi.BLOCK
    st, f, n = compress_ex(data, ts, sh, bs, 0)
    assert st == bf.ZH_OK and f == _lib.blosc_compress(data, ts, sh, bs) and f[2] >> 5 == 1
    st, f, n = compress_ex(data, ts, sh, bs, be.FLAG)
    assert st == bf.ZH_OK and f == be.expected(data, ts, sh, bs) and f[2] >> 5 == 4
    for flags in (2, 3, 0x80000000):
        assert compress_ex(data, ts, sh, bs, flags)[0] == bf.ZH_EINVAL
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_compress(data, ts, sh, bs, flags=flags)
        assert e.value.status == bf.ZH_EINVAL
    for flags in (0, be.FLAG):
        assert compress_ex(data, ts, sh, bs, flags, query=True) == (bf.ZH_OK, None, len(data) + 16)
        assert compress_ex(data, ts, sh, bs, flags, cap=len(data) + 15)[0] == bf.ZH_EINVAL
        assert compress_ex(data, 0, sh, bs, flags)[0] == bf.ZH_EINVAL
    assert _lib.blosc_compress(b"", 4, 1, zstd=True) == \
        struct.pack("<BBBBIII", 2, 1, 0x83, 4, 0, 0, 16)


def test_sizes_of_the_issue():
    """The 64 KiB image as uint16 under the byte and the bit shuffle with the default block size:
    the sizes the pieces gave when they were put together on the CPU (the LZ4 writer: 31 635 B
    and 30 870 B; MEMCPYED: 65 552 B)."""
    assert len(_lib.blosc_compress(bi.img(), 2, 1, zstd=True)) == 28188
    assert len(_lib.blosc_compress(bi.img(), 2, 2, zstd=True)) == 20788


def test_every_block_capacity():
    buffers = [bi.img(), bi.ramp(), bi.smooth(100001), bytes(70000)]
    for bs in (16 << 10, (16 << 10) + 4, 32 << 10, (32 << 10) + 4, 64 << 10):
        for ts, sh in ((2, 1), (4, 2), (1, 0)):
            for k, data in enumerate(buffers):
                f = _lib.blosc_compress(data, ts, sh, bs, zstd=True)
                assert f == be.expected(data, ts, sh, bs), (bs, ts, sh, k)
                assert bf.host_decode(f)[1] == data, (bs, ts, sh, k)
                if k >= 2:      # a period of 15 bytes and a run: compressed under every shuffle
                    assert not f[2] & 0x02 and len(f) < len(data) // 2, (bs, ts, sh, k)
            # the zeros: at most 9 streams, each a header, one sequence and a few literals
            assert len(f) < 70000 // 100, (bs, ts, sh)


def test_codec_object(monkeypatch):
    ramp = bi.ramp()
    for shuffle, code in (("noshuffle", 0), ("shuffle", 1), ("bitshuffle", 2)):
        c = BloscCodec("zstd", 5, shuffle, 4)
        monkeypatch.delenv("ZH_BLOSC_ZSTD_ENCODE", raising=False)
        g = c.encode(ramp)
        assert g[2] & 0x02 and g[16:] == ramp and len(g) == len(ramp) + 16
        monkeypatch.setenv("ZH_BLOSC_ZSTD_ENCODE", "0")
        assert c.encode(ramp) == g
        monkeypatch.setenv("ZH_BLOSC_ZSTD_ENCODE", "1")
        f = c.encode(ramp)
        assert f == _lib.blosc_compress(ramp, 4, code, zstd=True) == be.expected(ramp, 4, code, 0)
        assert f[2] >> 5 == 4 and c.decode(f) == ramp and c.decode(g) == ramp
        if code:    # shuffled, the ramp's high bytes are runs; as it is, it has no repeats
            assert not f[2] & 0x02 and len(f) < len(ramp) // 2
        # the switch is zstd's alone
        assert BloscCodec("lz4", 5, shuffle, 4).encode(ramp) == _lib.blosc_compress(ramp, 4, code)
        for cname in ("blosclz", "zlib", "snappy"):
            h = BloscCodec(cname, 5, shuffle, 4).encode(ramp)
            assert h[2] & 0x02 and h[16:] == ramp


# ---- the lane loop under sanitizers ----------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/blosc_zstd_enc_check built with AddressSanitizer + UBSan, as the checker fixture of
    test_blosc_encode_host.py builds its program: stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "blosc_zstd_enc_check.cpp")
    exe = str(tmp_path_factory.mktemp("blosc_zstd_enc_check") / "blosc_zstd_enc_check")
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
        for _, data, ts, sh, bs, _ in MATRIX:
            fh.write(struct.pack("<IIII", len(data), ts, sh, bs) + data)
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
