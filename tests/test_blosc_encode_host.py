"""The host half of the blosc LZ4 frame writer (zarr-java_amd/csrc/zh_blosc_enc.h,
zh_blosc_compress): every frame of the input matrix decodes with the library's decoder and with
liblz4, tiles exactly, and stays within nbytes + 16; sizes against liblz4 on the same streams;
the codec object; and the lane-loop form under AddressSanitizer + UBSan in a stand-alone
program.  No GPU."""
import os
import shutil
import struct
import subprocess

import pytest

import blosc_enc_inputs as bi
import blosc_frames as bf
import test_blosc as tb
from zarrhip import _lib
from zarrhip.codecs import BloscCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = bi.matrix()


@pytest.fixture(scope="module")
def frames():
    return [_lib.blosc_compress(d, ts, sh, bs) for _, d, ts, sh, bs in MATRIX]


def test_frames_decode_to_their_input(frames):
    for (label, data, *_), f in zip(MATRIX, frames):
        st, out, msg = bf.host_decode(f)
        assert (st, out) == (bf.ZH_OK, data), (label, msg)
        assert len(f) <= len(data) + 16, label
        assert struct.unpack("<I", f[12:16])[0] == len(f), label
        assert f[0] == 2 and f[1] == 1 and f[2] >> 5 == 1, label


def test_liblz4_decodes_the_streams(frames):
    """test_blosc.independent_blosc_lz4 (liblz4 through pyarrow enforces the LZ4 end rules)
    wherever it applies: LZ4 flag, not memcpyed, byte or no shuffle."""
    walked = 0
    for (label, data, ts, sh, _), f in zip(MATRIX, frames):
        if sh == 2 or f[2] & 0x02:
            continue
        assert tb.independent_blosc_lz4(f) == data, label
        walked += 1
    assert walked > len(MATRIX) // 3


def test_rows_tile_the_frame(frames):
    kinds = set()
    for (label, data, ts, sh, _), f in zip(MATRIX, frames):
        if f[2] & 0x02:
            assert len(f) == len(data) + 16 and f[16:] == data, label
            continue
        rows = _lib.blosc_streams(f)
        blocks = [r for r in rows if r[0] == 0]
        nblocks = len(blocks)
        starts = struct.unpack(f"<{nblocks}I", f[16:16 + 4 * nblocks])
        pos, raw, k = 16 + 4 * nblocks, 0, -1
        for r in rows:
            if r[0] == 0:
                k += 1
                assert r[1] == raw and starts[k] == pos, label
                raw += r[2]
                left = r[2]
                kinds.add((r[4], r[5] > 1))
                continue
            assert r[1] == pos + 4 and 0 < r[2] <= r[4], label   # never longer than raw
            assert r[5] == (0 if r[2] == r[4] else 1), label
            pos += 4 + r[2]
            left -= r[4]
            assert left >= 0
        assert raw == len(data) and pos == len(f), label
        # the split rule: byte shuffle, typesize <= 16, blocksize / typesize >= 128; a leftover
        # block is never split
        bs = struct.unpack("<I", f[8:12])[0]
        split = sh == 1 and ts <= 16 and bs // ts >= 128
        assert bool(f[2] & 0x10) == (not split), label
        assert [b[5] for b in blocks] == [ts if split and b[2] == bs else 1 for b in blocks]
        assert bs <= bi.BLOCK and (bs % ts == 0 or bs < ts or nblocks == 1), label
    assert kinds >= {(0, False), (1, True), (1, False), (2, False)}


def test_edge_cases():
    assert _lib.blosc_compress(b"", 4, 1) == struct.pack("<BBBBIII", 2, 1, 0x23, 4, 0, 0, 16)
    for ts in (0, 256, -1):
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_compress(b"abcd" * 8, ts, 1)
        assert e.value.status == bf.ZH_EINVAL
    # a configured block size above 64 KiB is clamped (blosc treats it as advice)
    data = bi.smooth(200000)
    f = _lib.blosc_compress(data, 4, 1, 1 << 20)
    assert struct.unpack("<I", f[8:12])[0] == bi.BLOCK and bf.host_decode(f)[1] == data
    # a leftover of 128 elements or more is still one stream
    assert [r[5] for r in _lib.blosc_streams(f) if r[0] == 0] == [4, 4, 4, 1]
    # tiny blocks: the block starts alone would pass nbytes + 16
    f = _lib.blosc_compress(data[:1000], 1, 0, 2)
    assert f[2] & 0x02 and len(f) == 1016 and bf.host_decode(f)[1] == data[:1000]


def test_derived_sizes(frames):
    seen = 0
    for (label, data, ts, sh, _), f in zip(MATRIX, frames):
        if label.startswith("zeros"):
            # a run costs one byte per 255 (LZ4's floor) and a dozen bytes of frame: every
            # stream of 4 KiB or more is far below rawsize / 64
            for r in _lib.blosc_streams(f):
                if r[0] == 1 and r[4] >= 4096:
                    assert r[2] <= r[4] // 64, label
                    seen += 1
        if label.startswith("random"):
            assert f[2] & 0x02 or all(r[5] == 0 for r in _lib.blosc_streams(f) if r[0] == 1), label
            seen += 1
    assert seen >= 2 * len(bi.TYPESIZES) * len(bi.SHUFFLES)


def test_sizes_against_liblz4():
    """Stream bytes of zh_blosc_compress against liblz4 (pyarrow's lz4_raw, default settings) on
    the same byte-shuffled streams of one 64 KiB block.  Asserted factor: 1.17 = the measured
    worst ratio 1.063 (img: 25 788 B against liblz4's 24 261 B; ramp: 806 B against 806 B) plus
    10 % headroom for a later retune of the hash and nothing else — the ratio table of
    DESIGN.md, "Blosc frames encoded on the device"."""
    pa = pytest.importorskip("pyarrow")
    lz = pa.Codec("lz4_raw")
    for name, data, ts in (("img", bi.img(), 2), ("ramp", bi.ramp(), 4)):
        f = _lib.blosc_compress(data, ts, 1, bi.BLOCK)
        rows = [r for r in _lib.blosc_streams(f) if r[0] == 1]
        assert [r[4] for r in rows] == [len(data) // ts] * ts
        ours = sum(r[2] for r in rows)
        ref = sum(min(len(s), len(lz.compress(s, asbytes=True)))
                  for s in bi.shuffled_streams(data, ts))
        print(f"{name}: zh_blosc_compress {ours} B, liblz4 {ref} B, ratio {ours / ref:.4f}")
        assert ours <= ref * 1.17, (name, ours, ref)


def test_codec_object_compresses_lz4():
    ramp = bi.ramp()
    c = BloscCodec("lz4", 5, "shuffle", 4)
    f = c.encode(ramp)
    assert not f[2] & 0x02 and len(f) < len(ramp) // 10
    assert f == _lib.blosc_compress(ramp, 4, 1) and c.decode(f) == ramp
    assert BloscCodec("lz4hc", 9, "bitshuffle", 2).encode(ramp) == _lib.blosc_compress(ramp, 2, 2)
    # clevel is not honoured, an unset typesize is 1
    assert BloscCodec("lz4", 0, "noshuffle").encode(ramp) == _lib.blosc_compress(ramp, 1, 0)
    # every other cname keeps writing MEMCPYED frames
    for cname in ("zstd", "blosclz", "zlib"):
        g = BloscCodec(cname, 5, "shuffle", 4).encode(ramp)
        assert g[2] & 0x02 and g[16:] == ramp


# ---- the lane loop under sanitizers ----------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/blosc_enc_check built with AddressSanitizer + UBSan, as the checker fixture of
    test_blosc_batch_host.py builds its program: stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "blosc_enc_check.cpp")
    exe = str(tmp_path_factory.mktemp("blosc_enc_check") / "blosc_enc_check")
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
        for _, data, ts, sh, bs in MATRIX:
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
