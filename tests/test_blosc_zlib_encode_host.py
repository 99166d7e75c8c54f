"""The host half of the blosc frame writer with zlib streams (zarr-java_amd/csrc/zh_blosc_enc.h
over ZlibCoder, zh_blosc_compress_ex with ZH_BLOSC_ENC_ZLIB and ZH_BLOSC_ENC_DYNAMIC): every frame
of the input matrix equals the frame built in Python around zh_gzip_compress
(blosc_zlib_enc_inputs.expected), decodes with the library's decoder, has its streams inflated by
Python's zlib and is planned for the device decoder; streams of several 16 KiB segments; the flags
of the call; the codec object behind ZH_BLOSC_ZLIB_ENCODE; and the writer under AddressSanitizer +
UBSan in a stand-alone program that inflates every stream with libz.  No GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import blosc_enc_inputs as bi
import blosc_frames as bf
import blosc_zlib_enc_inputs as be
import blosc_zlib_inputs as bz
from zarrhip import _abi as A
from zarrhip import _lib
from zarrhip.codecs import BloscCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def check_frame(f, data, ts, sh, bs, label):
    """One frame of the writer: the header, the library's decoder, the device decoder's plan, and
    Python's zlib on every compressed stream.  Returns the (method, raw stream) pairs."""
    st, out, msg = bf.host_decode(f)
    assert (st, out) == (bf.ZH_OK, data), (label, msg)
    assert len(f) <= len(data) + 16 and struct.unpack("<I", f[12:16])[0] == len(f), label
    assert f[0] == 2 and f[1] == 1 and f[2] >> 5 == 3, label
    if f[2] & 0x02:
        assert f[16:] == data, label
        return []
    assert _lib.blosc_batch_plan([f], bz.FLAG)[1][0][2] == 0, label      # where = 0
    raw = be.raw_streams(data, ts, sh, bs)
    rows = [r for r in _lib.blosc_streams(f, bz.FLAG) if r[0] == 1]
    assert len(rows) == len(raw), label
    seen = []
    for r, want in zip(rows, raw):
        assert r[4] == len(want), label
        payload = f[r[1]:r[1] + r[2]]
        if r[2] == r[4]:
            assert r[5] == 0 and payload == want, label
            seen.append(("raw", want))
            continue
        assert r[5] == bz.KZLIB and r[2] < r[4] and payload[:2] == b"\x78\x01", label
        assert zlib.decompress(payload) == want, label
        seen.append(("zlib", want))
    return seen


@pytest.mark.parametrize("flags", be.FLAGS)
def test_matrix_equals_the_python_built_frames(flags):
    dynamic = flags == be.FLAG_DYN
    kinds = {"zlib": 0, "raw": 0, "frames": 0, "memcpyed": 0}
    forms = set()
    for label, data, ts, sh, bs, want in be.matrix(flags):
        f = _lib.blosc_compress(data, ts, sh, bs, flags=flags)
        assert f == want, label
        name = be.name_of(label)
        # a writer that stores everything plain does not pass
        if name in (be.COMPRESSED_DYNAMIC if dynamic else be.COMPRESSED):
            assert not f[2] & 0x02, label
        if name in be.MEMCPYED:
            assert f[2] & 0x02, label
        seen = check_frame(f, data, ts, sh, bs, label)
        kinds["memcpyed" if f[2] & 0x02 else "frames"] += 1
        for method, stream in seen:
            kinds[method] += 1
            if method == "zlib":
                forms |= be.segment_forms(stream, dynamic)
    assert all(v > 0 for v in kinds.values()), kinds
    # (a stored segment inside a compressed stream: test_multi_segment_streams)
    if dynamic:
        assert "dynamic" in forms
        assert any(a[5] != b[5] for a, b in zip(be.matrix(be.FLAG), be.matrix(be.FLAG_DYN)))
    else:
        assert "dynamic" not in forms and "fixed" in forms


@pytest.mark.parametrize("flags", be.FLAGS)
def test_multi_segment_streams(flags):
    dynamic = flags == be.FLAG_DYN
    forms = {}
    for label, data, ts, sh, bs in be.multi_segment():
        f = _lib.blosc_compress(data, ts, sh, bs, flags=flags)
        assert f == be.expected(data, ts, sh, bs, flags), label
        seen = check_frame(f, data, ts, sh, bs, label)
        forms[label] = [be.segment_forms(s, dynamic) for m, s in seen if m == "zlib"]
    # four segments in a 64 KiB stream; a stored and a fixed (or dynamic) segment in one stream
    assert len(be.segments(b"\xff" * (64 << 10), dynamic)) == 4
    for label in ("stored+fixed", "fixed+stored"):
        (got,) = forms[label]
        assert "stored" in got and len(got) == 2, (label, got)
    assert forms["ff-64k"] and forms["text-bs65536-sh0"]


def test_flags():
    data, ts, sh, bs = bi.img(), 2, 1, bi.BLOCK
    for flags in be.FLAGS:
        st, f, n = compress_ex(data, ts, sh, bs, flags)
        assert st == bf.ZH_OK and f == be.expected(data, ts, sh, bs, flags) and f[2] >> 5 == 3
        assert compress_ex(data, ts, sh, bs, flags, query=True) == (bf.ZH_OK, None, len(data) + 16)
        assert compress_ex(data, ts, sh, bs, flags, cap=len(data) + 15)[0] == bf.ZH_EINVAL
        assert compress_ex(data, 0, sh, bs, flags)[0] == bf.ZH_EINVAL
    for flags in be.BAD_FLAGS:
        assert compress_ex(data, ts, sh, bs, flags)[0] == bf.ZH_EINVAL, flags
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_compress(data, ts, sh, bs, flags=flags)
        assert e.value.status == bf.ZH_EINVAL and "ZH_BLOSC_ENC_ZLIB" in str(e.value)
    # 0 and 1 are the writers of before, byte for byte
    assert compress_ex(data, ts, sh, bs, 0)[1] == _lib.blosc_compress(data, ts, sh, bs, zstd=False)
    assert compress_ex(data, ts, sh, bs, 1)[1] == _lib.blosc_compress(data, ts, sh, bs, zstd=True)
    assert compress_ex(data, ts, sh, bs, 0)[1][2] >> 5 == 1
    assert compress_ex(data, ts, sh, bs, 1)[1][2] >> 5 == 4
    # the keywords are the flag words
    assert _lib.blosc_compress(data, ts, sh, bs, zlib=True) == compress_ex(data, ts, sh, bs, 4)[1]
    assert _lib.blosc_compress(data, ts, sh, bs, zlib=True, dynamic=True) == \
        compress_ex(data, ts, sh, bs, 12)[1]
    with pytest.raises(_lib.ZhError):
        _lib.blosc_compress(data, ts, sh, bs, dynamic=True)
    assert _lib.blosc_compress(b"", 4, 1, zlib=True) == \
        struct.pack("<BBBBIII", 2, 1, 0x63, 4, 0, 0, 16)


def test_codec_object(monkeypatch):
    ramp = bi.ramp()
    for shuffle, code in (("noshuffle", 0), ("shuffle", 1), ("bitshuffle", 2)):
        c = BloscCodec("zlib", 5, shuffle, 4)
        monkeypatch.delenv("ZH_BLOSC_ZLIB_ENCODE", raising=False)
        assert not c.zlib_enc() and not c.compressed()
        g = c.encode(ramp)
        assert g[2] & 0x02 and g[16:] == ramp and len(g) == len(ramp) + 16
        for off in ("0", "3", ""):
            monkeypatch.setenv("ZH_BLOSC_ZLIB_ENCODE", off)
            assert c.encode(ramp) == g
        for mode, flags in (("1", be.FLAG), ("2", be.FLAG_DYN)):
            monkeypatch.setenv("ZH_BLOSC_ZLIB_ENCODE", mode)
            assert c.zlib_enc() == flags and c.compressed()
            f = c.encode(ramp)
            assert f == _lib.blosc_compress(ramp, 4, code, flags=flags) == \
                be.expected(ramp, 4, code, 0, flags)
            assert f[2] >> 5 == 3 and c.decode(f) == ramp and c.decode(g) == ramp
            if code:    # shuffled, the ramp's high bytes are runs; as it is, it has no repeats
                assert not f[2] & 0x02 and len(f) < len(ramp) // 2
            # the switch is zlib's alone
            assert BloscCodec("lz4", 5, shuffle, 4).encode(ramp) == \
                _lib.blosc_compress(ramp, 4, code)
            for cname in ("blosclz", "snappy", "zstd"):
                h = BloscCodec(cname, 5, shuffle, 4).encode(ramp)
                assert h[2] & 0x02 and h[16:] == ramp


# ---- the writer under sanitizers -------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/blosc_zlib_enc_check built with AddressSanitizer + UBSan, as the checker fixture of
    test_blosc_zstd_encode_host.py builds its program (and with libz): stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "blosc_zlib_enc_check.cpp")
    exe = str(tmp_path_factory.mktemp("blosc_zlib_enc_check") / "blosc_zlib_enc_check")
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


def random_inputs():
    """Seeded buffers of every kind of content under random parameters."""
    rng = np.random.default_rng(2027)
    out = []
    for k in range(60):
        n = int(rng.integers(0, 150000 if k % 6 == 0 else 9000))
        kind = k % 4
        if kind == 0:
            a = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            a = (np.arange(n) // (1 + k % 9) % (2 + k % 31)).astype(np.uint8)
        elif kind == 2:
            a = rng.integers(0, 4, n, dtype=np.uint8) * 61
        else:
            a = np.where(rng.random(n) < 0.9, 0, rng.integers(0, 256, n)).astype(np.uint8)
        ts = int(rng.choice([1, 2, 3, 4, 8, 16, 17]))
        bs = int(rng.choice([0, 0, 300, 4096, 20000, 65536, 1 << 20]))
        out.append((f"random{k}", a.tobytes(), ts, int(rng.integers(0, 3)), bs))
    return out


@pytest.mark.parametrize("flags", be.FLAGS)
def test_writer_under_sanitizers(checker, flags, tmp_path):
    cases = [c[:5] for c in be.matrix(flags)] + be.multi_segment() + random_inputs()
    src, dst = tmp_path / "buffers.bin", tmp_path / "frames.bin"
    with open(src, "wb") as fh:
        for _, data, ts, sh, bs in cases:
            fh.write(struct.pack("<IIII", len(data), ts, sh, bs) + data)
    r = subprocess.run([checker, str(src), str(dst), str(flags)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) and all(ln.endswith(" ok") for ln in lines)
    raw = open(dst, "rb").read()
    pos = 0
    for label, data, ts, sh, bs in cases:
        (n,) = struct.unpack("<I", raw[pos:pos + 4])
        # the library's build gives the same bytes
        assert raw[pos + 4:pos + 4 + n] == _lib.blosc_compress(data, ts, sh, bs, flags=flags), label
        pos += 4 + n
    assert pos == len(raw)
